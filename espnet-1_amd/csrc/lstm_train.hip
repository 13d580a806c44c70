// LSTM training steps of SequentialRNNLM (torch.nn.LSTM inside espnet2/lm/seq_rnn_lm.py:92-104,
// unrolled over time by the host): ea_lstm_cell_fwd and ea_lstm_cell_bwd, one plain launch per
// time step per layer.  The input projection of all time steps (X . W_ih^T + b_ih + b_hh) and
// every product of the backward that is not recurrent (dW_hh, dW_ih, dX, the bias sums) are
// ordinary GEMMs / column sums over all T * B rows; only the recurrence is here.
//
//   forward   gates = xproj[t] + h_{t-1} . W_hh^T                    K = Hp, N = 4H
//             c_t = sigmoid(f) c_{t-1} + sigmoid(i) tanh(g);  h_t = sigmoid(o) tanh(c_t)
//             writes h_t, c_t, the four ACTIVATED gates (the backward never recomputes them)
//             and, for the bf16 path, a bf16 h_t (the next step's and the dW_hh GEMM's operand)
//   backward  dh = dh_out[t] + dgates[t+1] . W_hh                    K = 4H (padded), N = H
//             then the cell's gradient on the block's own hidden units (see ea_lstm_cell_bwd in
//             include/espnet_amd.h); the first launch (t = T - 1) has no dgates[t+1] and skips
//             the product.
//
// Both are the weight-stream shape of rnn_lm.hip's lstm_step_kernel with B a training batch: a
// block owns up to 64 rows (MT row tiles) x NJ column tiles and ALL of K; its 8 waves split K
// slice-wise, each keeping U slices of loads in flight, operands go global -> registers in MFMA
// fragment order (the weight is used once per block, nothing is shared between waves), the
// waves' partial tiles are summed through LDS and the epilogue runs on the sums in f32.  Rows
// beyond 64 go to further block rows (grid.y); those re-read the weights, from L2 / MALL for
// every block row but the first.  The forward's column tile is 4 hidden units x 4 gates (so the
// cell update is local to the tile), the backward's is 16 hidden units.  No block waits for
// another: the time loop is the host's.
//
// Packs (espnet_amd/lm/seq_rnn_lm.py pack_lstm_hh / pack_lstm_hh_t, layout in the header).
#include "common.h"

namespace {

constexpr int LT_W = 8;  // waves per block (K split)

template <bool BF> struct Frag;
template <> struct Frag<false> { typedef f32x4 T; typedef float W; };
template <> struct Frag<true> { typedef bf16x8 T; typedef bf16 W; };

// the lane's AN operand elements k .. k + AN - 1 of a row; elements >= lim are 0.
// `fast` (wave-uniform): the whole slice lies below lim and the row is 16-B aligned.
template <bool BF>
EA_DEV typename Frag<BF>::T load_a(const typename Frag<BF>::W* __restrict__ row, int k, int lim, bool fast) {
  constexpr int AN = BF ? 8 : 4;
  typedef typename Frag<BF>::T frag;
  if (fast) return *(const frag*)(row + k);
  frag out;
#pragma unroll
  for (int e = 0; e < AN; ++e) {
    if (k + e < lim)
      out[e] = row[k + e];
    else
      out[e] = (typename Frag<BF>::W)0.f;
  }
  return out;
}

EA_DEV float sigmoid_exact(float x) { return 1.f / (1.f + expf(-x)); }

// acc = A(rows of the block, K) . pack(column tiles t0 .. t0 + NJ - 1)^T summed over the block's
// waves: on return red[q][row][col], q < LT_W / 2, hold four partial sums of every element
// (the epilogue adds them).  ar[i]: the lane's operand row of row tile i.
template <bool BF, int MT, int NJ, int U>
EA_DEV void block_product(const typename Frag<BF>::W* const (&ar)[MT], int lim, bool avec, const void* wpack, int nks,
                          int t0, int ntiles, float (*red)[16 * MT][16 * NJ + 4]) {
  typedef typename Frag<BF>::W WT;
  typedef typename Frag<BF>::T frag;
  constexpr int SL = BF ? 32 : 16;  // K depth of one slice (one 16-B load per lane)
  constexpr int AN = BF ? 8 : 4;    // operand elements per lane per slice
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lr = lane & 15, g = lane >> 4;
  const WT* bp[NJ];
  bool bok[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    bok[j] = t0 + j < ntiles;
    bp[j] = (const WT*)wpack + ((long)(bok[j] ? t0 + j : 0) * nks * 16 + lr) * SL + g * AN;
  }
  f32x4 acc[MT][NJ];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const frag zero = {};

  for (int s0 = w; s0 < nks; s0 += LT_W * U) {
    frag a[U][MT], b[U][NJ];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int s = s0 + u * LT_W;
      const bool in = s < nks;
#pragma unroll
      for (int j = 0; j < NJ; ++j) b[u][j] = in && bok[j] ? *(const frag*)(bp[j] + (long)s * 16 * SL) : zero;
      const bool fast = avec && (s + 1) * SL <= lim;
#pragma unroll
      for (int i = 0; i < MT; ++i) a[u][i] = in ? load_a<BF>(ar[i], s * SL + g * AN, lim, fast) : zero;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          if constexpr (BF) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u][i], b[u][j], acc[i][j], 0, 0, 0);
          } else {
            // four 4-deep steps: step e takes element e of every lane's 16-B chunk (the same
            // k permutation on both operands)
#pragma unroll
            for (int e = 0; e < 4; ++e)
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][i][e], b[u][j][e], acc[i][j], 0, 0, 0);
          }
        }
  }

  // waves 4-7 through LDS into waves 0-3 (D layout: the lane holds rows 4 * (lane >> 4) + r of
  // column lane & 15)
  if (w >= LT_W / 2) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[w - LT_W / 2][i * 16 + 4 * g + r][j * 16 + lr] = acc[i][j][r];
  }
  __syncthreads();
  if (w < LT_W / 2) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float* q = &red[w][i * 16 + 4 * g + r][j * 16 + lr];
          *q = acc[i][j][r] + *q;
        }
  }
  __syncthreads();
}

// ------------------------------------------------------------------ forward
struct CellFwdP {
  int n, H, Hp;
  const void* w;
  const float* xproj;
  long ldx;
  const void* hp;  // f32, or bf16 with the bf16 pack
  const float* cp;
  long ldp;
  float* ho;
  float* co;
  long ldo;
  bf16* hb;
  float* gates;
  long ldg;
  int hvec;
};

template <bool BF, int MT, int NJ, int U>
__global__ __launch_bounds__(64 * LT_W) void lstm_cell_fwd_kernel(CellFwdP p) {
  typedef typename Frag<BF>::W WT;
  constexpr int SL = BF ? 32 : 16;
  constexpr int BR = 16 * MT, LD = 16 * NJ + 4;
  __shared__ __attribute__((aligned(16))) float red[LT_W / 2][BR][LD];
  const int lr = threadIdx.x & 15;
  const int r0 = blockIdx.y * BR, t0 = blockIdx.x * NJ;
  const int ntiles = (p.H + 3) / 4;

  const WT* hr[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int row = r0 + i * 16 + lr;
    hr[i] = (const WT*)p.hp + (long)(row < p.n ? row : 0) * p.ldp;  // rows >= n are never stored
  }
  block_product<BF, MT, NJ, U>(hr, p.H, p.hvec, p.w, p.Hp / SL, t0, ntiles, red);

  constexpr int CELLS = BR * NJ * 4;  // (row, hidden unit) pairs of the block
  for (int ci = threadIdx.x; ci < CELLS; ci += 64 * LT_W) {
    const int lrow = ci / (NJ * 4), cu = ci % (NJ * 4);  // cu = 4 * (tile in block) + unit in tile
    const int row = r0 + lrow, unit = t0 * 4 + cu;
    if (row >= p.n || unit >= p.H) continue;
    float4 s = *(const float4*)&red[0][lrow][cu * 4];
#pragma unroll
    for (int q = 1; q < LT_W / 2; ++q) {
      const float4 t = *(const float4*)&red[q][lrow][cu * 4];
      s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    const float* xp = p.xproj + (long)row * p.ldx + unit;  // torch gate order: column gate * H + unit
    const float cprev = p.cp[(long)row * p.ldp + unit];
    const float gi = sigmoid_exact(s.x + xp[0]), gf = sigmoid_exact(s.y + xp[p.H]);
    const float gg = tanhf(s.z + xp[2 * (long)p.H]), go = sigmoid_exact(s.w + xp[3 * (long)p.H]);
    const float c = gf * cprev + gi * gg;
    const float h = go * tanhf(c);
    p.co[(long)row * p.ldo + unit] = c;
    p.ho[(long)row * p.ldo + unit] = h;
    if (p.hb) p.hb[(long)row * p.ldo + unit] = (bf16)h;
    *(float4*)(p.gates + (long)row * p.ldg + 4 * unit) = make_float4(gi, gf, gg, go);
  }

  // pad columns [H, ldo) of this row group: zeros (the next step, the next layer and the
  // GEMMs over the sequence read them against zero weight columns)
  if (blockIdx.x == gridDim.x - 1) {
    const int padw = (int)(p.ldo - p.H);
    const int rows = min(BR, p.n - r0);
    for (int idx = threadIdx.x; idx < rows * padw; idx += 64 * LT_W) {
      const long o = (long)(r0 + idx / padw) * p.ldo + p.H + idx % padw;
      p.ho[o] = 0.f;
      p.co[o] = 0.f;
      if (p.hb) p.hb[o] = (bf16)0.f;
    }
  }
}

template <bool BF, int MT, int NJ>
int launch_fwd(const CellFwdP& p, hipStream_t st) {
  constexpr int U = MT == 4 ? 4 : 8;
  dim3 grid(ea_cdiv((p.H + 3) / 4, NJ), ea_cdiv(p.n, 16 * MT), 1);
  hipLaunchKernelGGL((lstm_cell_fwd_kernel<BF, MT, NJ, U>), grid, dim3(64 * LT_W), 0, st, p);
  EA_LAUNCH_CHECK();
  return 0;
}

template <bool BF>
int launch_fwd_mt(const CellFwdP& p, hipStream_t st) {
  // a training batch fills 64-row blocks; the narrow row tiles serve B < 64 (the last batch of
  // an epoch, validation).  Two column tiles per block from H = 1024 up, as ea_lstm_step does.
  const bool wide = (p.H + 3) / 4 >= 256;
  if (p.n <= 16) return wide ? launch_fwd<BF, 1, 2>(p, st) : launch_fwd<BF, 1, 1>(p, st);
  if (p.n <= 32) return wide ? launch_fwd<BF, 2, 2>(p, st) : launch_fwd<BF, 2, 1>(p, st);
  return wide ? launch_fwd<BF, 4, 2>(p, st) : launch_fwd<BF, 4, 1>(p, st);
}

// ------------------------------------------------------------------ backward
struct CellBwdP {
  int n, H, G;  // G = 4H
  const void* wt;
  const void* dgn;  // dgates[t+1]: f32, or bf16 with the bf16 pack; NULL on the first launch
  long lddn;
  int avec;
  const float* dho;
  long lddh;
  const float* gates;
  long ldg;
  const float* c;
  const float* cprev;
  long ldc;
  const float* dci;
  float* dco;
  long lddc;
  float* dg;
  bf16* dgb;
  long ldd;
  float* dht;
  long ldt;
};

template <bool BF, int MT, int U>
__global__ __launch_bounds__(64 * LT_W) void lstm_cell_bwd_kernel(CellBwdP p) {
  typedef typename Frag<BF>::W WT;
  constexpr int SL = BF ? 32 : 16;
  constexpr int BR = 16 * MT, LD = 16 + 4;
  __shared__ __attribute__((aligned(16))) float red[LT_W / 2][BR][LD];
  const int lr = threadIdx.x & 15;
  const int r0 = blockIdx.y * BR, t0 = blockIdx.x;
  const int ntiles = (p.H + 15) / 16;
  const bool rec = p.dgn != nullptr;  // uniform over the launch

  if (rec) {
    const WT* ar[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int row = r0 + i * 16 + lr;
      ar[i] = (const WT*)p.dgn + (long)(row < p.n ? row : 0) * p.lddn;
    }
    const int Gp = (p.G + EA_LSTM_KG - 1) / EA_LSTM_KG * EA_LSTM_KG;
    block_product<BF, MT, 1, U>(ar, p.G, p.avec, p.wt, Gp / SL, t0, ntiles, red);
  }

  constexpr int CELLS = BR * 16;
  for (int ci = threadIdx.x; ci < CELLS; ci += 64 * LT_W) {
    const int lrow = ci / 16, cu = ci % 16;
    const int row = r0 + lrow, unit = t0 * 16 + cu;
    if (row >= p.n || unit >= p.H) continue;
    float dh = p.dho ? p.dho[(long)row * p.lddh + unit] : 0.f;
    if (rec) {
      float s = red[0][lrow][cu];
#pragma unroll
      for (int q = 1; q < LT_W / 2; ++q) s += red[q][lrow][cu];
      dh += s;
    }
    const float4 a = *(const float4*)(p.gates + (long)row * p.ldg + 4 * unit);  // i, f, g, o
    const float tc = tanhf(p.c[(long)row * p.ldc + unit]);
    const float cp = p.cprev[(long)row * p.ldc + unit];
    const float dcar = p.dci ? p.dci[(long)row * p.lddc + unit] : 0.f;
    const float d_o = dh * tc * a.w * (1.f - a.w);
    const float dc = dcar + dh * a.w * (1.f - tc * tc);
    const float d_i = dc * a.z * a.x * (1.f - a.x);
    const float d_f = dc * cp * a.y * (1.f - a.y);
    const float d_g = dc * a.x * (1.f - a.z * a.z);
    p.dco[(long)row * p.lddc + unit] = dc * a.y;
    float* o = p.dg + (long)row * p.ldd + unit;  // torch gate order: column gate * H + unit
    o[0] = d_i; o[p.H] = d_f; o[2 * (long)p.H] = d_g; o[3 * (long)p.H] = d_o;
    if (p.dgb) {
      bf16* ob = p.dgb + (long)row * p.ldd + unit;
      ob[0] = (bf16)d_i; ob[p.H] = (bf16)d_f; ob[2 * (long)p.H] = (bf16)d_g; ob[3 * (long)p.H] = (bf16)d_o;
    }
    if (p.dht) p.dht[(long)row * p.ldt + unit] = dh;
  }

  // pad columns [4H, ldd) of dgates and [H, lddc) of the carry: zeros
  if (blockIdx.x == gridDim.x - 1) {
    const int rows = min(BR, p.n - r0);
    const int padg = (int)(p.ldd - p.G), padc = (int)(p.lddc - p.H);
    for (int idx = threadIdx.x; idx < rows * padg; idx += 64 * LT_W) {
      const long o = (long)(r0 + idx / padg) * p.ldd + p.G + idx % padg;
      p.dg[o] = 0.f;
      if (p.dgb) p.dgb[o] = (bf16)0.f;
    }
    for (int idx = threadIdx.x; idx < rows * padc; idx += 64 * LT_W)
      p.dco[(long)(r0 + idx / padc) * p.lddc + p.H + idx % padc] = 0.f;
  }
}

template <bool BF, int MT>
int launch_bwd(const CellBwdP& p, hipStream_t st) {
  constexpr int U = MT == 4 ? 4 : 8;
  dim3 grid(ea_cdiv(p.H, 16), ea_cdiv(p.n, 16 * MT), 1);
  hipLaunchKernelGGL((lstm_cell_bwd_kernel<BF, MT, U>), grid, dim3(64 * LT_W), 0, st, p);
  EA_LAUNCH_CHECK();
  return 0;
}

template <bool BF>
int launch_bwd_mt(const CellBwdP& p, hipStream_t st) {
  if (p.n <= 16) return launch_bwd<BF, 1>(p, st);
  if (p.n <= 32) return launch_bwd<BF, 2>(p, st);
  return launch_bwd<BF, 4>(p, st);
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

}  // namespace

extern "C" int ea_lstm_cell_fwd(int wdtype, int n, int H, const void* wpack, const float* xproj, long ldx,
                                const void* h_prev, const float* c_prev, long ldp, float* h_out, float* c_out,
                                long ldo, void* hb_out, float* gates, long ldg, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG((wdtype == EA_F32 || wdtype == EA_BF16) && n >= 0 && H >= 1);
  EA_CHECK_ARG(wpack && xproj && h_prev && c_prev && h_out && c_out && gates && aligned16(wpack));
  EA_CHECK_ARG(ldx >= 4L * H && ldp >= H && ldo >= H && ldg >= 4L * H && ldg % 4 == 0 && aligned16(gates));
  EA_CHECK_ARG(wdtype == EA_F32 || hb_out);  // the bf16 path's next h_prev
  EA_CHECK_ARG((const void*)h_out != h_prev && c_out != c_prev && (const void*)h_out != (const void*)c_prev &&
               (const void*)c_out != h_prev && (!hb_out || (hb_out != h_prev && hb_out != (const void*)c_prev)));
  if (n == 0) return 0;
  CellFwdP p;
  p.n = n; p.H = H;
  p.Hp = ea_cdiv(H, EA_LSTM_KG) * EA_LSTM_KG;
  p.w = wpack; p.xproj = xproj; p.ldx = ldx; p.hp = h_prev; p.cp = c_prev; p.ldp = ldp;
  p.ho = h_out; p.co = c_out; p.ldo = ldo; p.hb = (bf16*)hb_out; p.gates = gates; p.ldg = ldg;
  p.hvec = aligned16(h_prev) && ldp % (wdtype == EA_BF16 ? 8 : 4) == 0;
  return wdtype == EA_BF16 ? launch_fwd_mt<true>(p, (hipStream_t)stream) : launch_fwd_mt<false>(p, (hipStream_t)stream);
}

extern "C" int ea_lstm_cell_bwd(int wdtype, int n, int H, const void* wpack_t, const void* dgates_next, long lddn,
                                const float* dh_out, long lddh, const float* gates, long ldg, const float* c,
                                const float* c_prev, long ldc, const float* dc_in, float* dc_out, long lddc,
                                float* dgates, void* dgates_b, long ldd, float* dh_tot, long ldt, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG((wdtype == EA_F32 || wdtype == EA_BF16) && n >= 0 && H >= 1);
  EA_CHECK_ARG(wpack_t && gates && c && c_prev && dc_out && dgates && aligned16(wpack_t) && aligned16(gates));
  EA_CHECK_ARG(ldg >= 4L * H && ldg % 4 == 0 && ldc >= H && lddc >= H && ldd >= 4L * H);
  EA_CHECK_ARG((!dgates_next || lddn >= 4L * H) && (!dh_out || lddh >= H) && (!dh_tot || ldt >= H));
  EA_CHECK_ARG(wdtype == EA_F32 || dgates_b);  // the bf16 path's next dgates_next
  EA_CHECK_ARG(dc_in != dc_out && dgates_next != (const void*)dgates && (!dgates_b || dgates_next != dgates_b));
  EA_CHECK_ARG(dh_tot != dh_out || !dh_tot);
  if (n == 0) return 0;
  CellBwdP p;
  p.n = n; p.H = H; p.G = 4 * H;
  p.wt = wpack_t; p.dgn = dgates_next; p.lddn = lddn;
  p.avec = dgates_next && aligned16(dgates_next) && lddn % (wdtype == EA_BF16 ? 8 : 4) == 0;
  p.dho = dh_out; p.lddh = lddh; p.gates = gates; p.ldg = ldg; p.c = c; p.cprev = c_prev; p.ldc = ldc;
  p.dci = dc_in; p.dco = dc_out; p.lddc = lddc; p.dg = dgates; p.dgb = (bf16*)dgates_b; p.ldd = ldd;
  p.dht = dh_tot; p.ldt = ldt;
  return wdtype == EA_BF16 ? launch_bwd_mt<true>(p, (hipStream_t)stream) : launch_bwd_mt<false>(p, (hipStream_t)stream);
}
