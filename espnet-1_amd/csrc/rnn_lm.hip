// Fused LSTM step (ea_lstm_step): one launch per layer per decoding step of SequentialRNNLM
// (espnet2/lm/seq_rnn_lm.py: torch.nn.LSTM over one token of every running hypothesis).
//
//   gates = x . W_ih^T + h_prev[src] . W_hh^T + (b_ih + b_hh)        (n, 4H), never leaves the block
//   c'    = sigmoid(f) * c_prev[src] + sigmoid(i) * tanh(g)
//   h'    = sigmoid(o) * tanh(c')
//
// n is the number of running hypotheses (a few dozen at most), so the launch is a weight
// stream: 4H x (I + H) elements read once, a few MFMAs per 16-B load.  A tile is 4 hidden units
// with all four gates (16 weight rows = one MFMA column tile), a block owns NJ consecutive
// tiles and ALL row tiles of up to 64 hypotheses, so for n <= 64 every weight element is loaded
// from memory exactly once per launch.  The block's 8 waves split K (wave w takes the slices w,
// w + 8, ...), each issuing the loads of U slices before its first MFMA (a two-stage register
// pipeline of half the depth measured no faster): weights go global ->
// registers in MFMA fragment order with no LDS staging (the operand is used once and is not
// shared between waves), exactly as gemm_skinny.hip does.  The partial tiles are summed through
// LDS and the cell update runs on the sums in f32.
//
// Packed weights (made on the host at prepare() time, see espnet_amd/lm/seq_rnn_lm.py
// pack_lstm_weights): K = Ip + Hp with Ip / Hp = I / H rounded up to EA_LSTM_KG and zero filled,
// [W_ih | W_hh] side by side along K; row 4 * u' + gate of tile t is gate `gate` (torch order
// i, f, g, o) of hidden unit 4 * t + u'; the tile is stored slice-major,
//     element (t, s, r, j) at ((t * nks + s) * 16 + r) * SL + j,   SL = 16 (f32) or 32 (bf16),
// so the 64 16-B loads of a wave for one slice cover one contiguous 1-KB piece.
#include "common.h"

namespace {

constexpr int LS_W = 8;  // waves per block (K split)

struct LstmP {
  int n, I, H, Ip, Hp, n_prev, V;
  const void* w;
  const float* bias;
  const float* x;
  long ldx;
  const long long* tok;
  long ldtok;
  const float* hp;
  const float* cp;
  long ldp;
  const int* src;
  float* ho;
  float* co;
  long ldo;
  bf16* hb;
  int xvec, hvec;
};

template <bool BF> struct Frag;
template <> struct Frag<false> { typedef f32x4 T; typedef float W; };
template <> struct Frag<true> { typedef bf16x8 T; typedef bf16 W; };

// the lane's AN operand elements k .. k + AN - 1 of an x / h_prev row; elements >= lim are 0.
// `fast` (wave-uniform): the whole slice lies below lim and the row is 16-B aligned.
template <bool BF>
EA_DEV typename Frag<BF>::T load_a(const float* __restrict__ row, int k, int lim, bool fast) {
  constexpr int AN = BF ? 8 : 4;
  float v[AN];
  if (fast) {
#pragma unroll
    for (int q = 0; q < AN / 4; ++q) {
      const float4 f = *(const float4*)(row + k + 4 * q);
      v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
    }
  } else {
#pragma unroll
    for (int e = 0; e < AN; ++e) v[e] = k + e < lim ? row[k + e] : 0.f;
  }
  typename Frag<BF>::T out;
#pragma unroll
  for (int e = 0; e < AN; ++e) {
    if constexpr (BF)
      out[e] = (bf16)v[e];
    else
      out[e] = v[e];
  }
  return out;
}

EA_DEV float sigmoid_exact(float x) { return 1.f / (1.f + expf(-x)); }

// MT 16-row tiles of hypotheses x NJ 16-row weight tiles per block; U slices per wave in flight
// (BF = bf16 pack; a bool so that profilers print the instantiation's name legibly)
template <bool BF, int MT, int NJ, int U>
__global__ __launch_bounds__(64 * LS_W) void lstm_step_kernel(LstmP p) {
  typedef typename Frag<BF>::W WT;
  constexpr int SL = BF ? 32 : 16;  // K depth of one slice (one 16-B load per lane)
  constexpr int AN = BF ? 8 : 4;    // operand elements per lane per slice
  constexpr int BR = 16 * MT, BC = 16 * NJ, LD = BC + 4;
  typedef typename Frag<BF>::T frag;
  __shared__ __attribute__((aligned(16))) float red[LS_W / 2][BR][LD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lr = lane & 15, g = lane >> 4;
  const int r0 = blockIdx.y * BR, t0 = blockIdx.x * NJ;
  const int ntiles = (p.H + 3) / 4;
  const int nkx = p.Ip / SL, nks = (p.Ip + p.Hp) / SL;

  const float* xr[MT];
  const float* hr[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int row = r0 + i * 16 + lr;
    const int rr = row < p.n ? row : 0;  // rows >= n compute on row 0's operands and are never stored
    long xi = rr;
    if (p.tok) {
      const long long t = p.tok[rr * p.ldtok];
      xi = t < 0 ? 0 : (t >= p.V ? p.V - 1 : t);
    }
    xr[i] = p.x + xi * p.ldx;
    int sr = rr;
    if (p.src) {
      sr = p.src[rr];
      sr = sr < 0 ? 0 : (sr >= p.n_prev ? p.n_prev - 1 : sr);
    }
    hr[i] = p.hp + (long)sr * p.ldp;
  }
  const WT* bp[NJ];
  bool bok[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    bok[j] = t0 + j < ntiles;
    bp[j] = (const WT*)p.w + ((long)(bok[j] ? t0 + j : 0) * nks * 16 + lr) * SL + g * AN;
  }
  f32x4 acc[MT][NJ];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const frag zero = {};

  for (int s0 = w; s0 < nks; s0 += LS_W * U) {
    frag a[U][MT], b[U][NJ];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int s = s0 + u * LS_W;
      const bool in = s < nks;
#pragma unroll
      for (int j = 0; j < NJ; ++j) b[u][j] = in && bok[j] ? *(const frag*)(bp[j] + (long)s * 16 * SL) : zero;
      const bool isx = s < nkx;
      const int sl = isx ? s : s - nkx;
      const int lim = isx ? p.I : p.H;
      const bool fast = (isx ? p.xvec : p.hvec) && (sl + 1) * SL <= lim;
#pragma unroll
      for (int i = 0; i < MT; ++i)
        a[u][i] = in ? load_a<BF>(isx ? xr[i] : hr[i], sl * SL + g * AN, lim, fast) : zero;
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

  // sum the 8 waves' partial tiles: waves 4-7 through LDS into waves 0-3, those into the epilogue
  // (D layout: the lane holds hypothesis rows 4 * (lane >> 4) + r of weight row lane & 15)
  if (w >= LS_W / 2) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[w - LS_W / 2][i * 16 + 4 * g + r][j * 16 + lr] = acc[i][j][r];
  }
  __syncthreads();
  if (w < LS_W / 2) {
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

  constexpr int CELLS = BR * NJ * 4;  // (hypothesis row, hidden unit) pairs of the block
  for (int ci = threadIdx.x; ci < CELLS; ci += 64 * LS_W) {
    const int lrow = ci / (NJ * 4), cu = ci % (NJ * 4);  // cu = 4 * (tile in block) + unit in tile
    const int row = r0 + lrow, unit = t0 * 4 + cu;
    if (row >= p.n || unit >= p.H) continue;
    float4 s = *(const float4*)&red[0][lrow][cu * 4];
#pragma unroll
    for (int q = 1; q < LS_W / 2; ++q) {
      const float4 t = *(const float4*)&red[q][lrow][cu * 4];
      s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    const float4 bs = *(const float4*)(p.bias + 4 * (long)unit);
    int sr = row;
    if (p.src) {
      sr = p.src[row];
      sr = sr < 0 ? 0 : (sr >= p.n_prev ? p.n_prev - 1 : sr);
    }
    const float cprev = p.cp[(long)sr * p.ldp + unit];
    const float gi = sigmoid_exact(s.x + bs.x), gf = sigmoid_exact(s.y + bs.y);
    const float gg = tanhf(s.z + bs.z), go = sigmoid_exact(s.w + bs.w);
    const float c = gf * cprev + gi * gg;
    const float h = go * tanhf(c);
    p.co[(long)row * p.ldo + unit] = c;
    p.ho[(long)row * p.ldo + unit] = h;
    if (p.hb) p.hb[(long)row * p.ldo + unit] = (bf16)h;
  }

  // pad columns [H, ldo) of this row group: zeros (the next layer and the output Linear read
  // them against zero weight columns)
  if (blockIdx.x == gridDim.x - 1) {
    const int padw = (int)(p.ldo - p.H);
    const int rows = min(BR, p.n - r0);
    for (int idx = threadIdx.x; idx < rows * padw; idx += 64 * LS_W) {
      const long o = (long)(r0 + idx / padw) * p.ldo + p.H + idx % padw;
      p.ho[o] = 0.f;
      p.co[o] = 0.f;
      if (p.hb) p.hb[o] = (bf16)0.f;
    }
  }
}

template <bool BF, int MT, int NJ>
int launch_lstm(const LstmP& p, hipStream_t st) {
  constexpr int U = MT == 4 ? 4 : 8;
  const int ntiles = (p.H + 3) / 4;
  dim3 grid(ea_cdiv(ntiles, NJ), ea_cdiv(p.n, 16 * MT), 1);
  hipLaunchKernelGGL((lstm_step_kernel<BF, MT, NJ, U>), grid, dim3(64 * LS_W), 0, st, p);
  EA_LAUNCH_CHECK();
  return 0;
}

template <bool BF>
int launch_lstm_mt(const LstmP& p, hipStream_t st) {
  // two tiles per block from H = 1024 up (>= 128 blocks): halves the blocks' re-reads of x / h,
  // which bound the wide launches (measured against one tile per block)
  const bool wide = (p.H + 3) / 4 >= 256;
  if (p.n <= 16) return wide ? launch_lstm<BF, 1, 2>(p, st) : launch_lstm<BF, 1, 1>(p, st);
  if (p.n <= 32) return wide ? launch_lstm<BF, 2, 2>(p, st) : launch_lstm<BF, 2, 1>(p, st);
  return wide ? launch_lstm<BF, 4, 2>(p, st) : launch_lstm<BF, 4, 1>(p, st);
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

}  // namespace

extern "C" int ea_lstm_step(int wdtype, int n, int I, int H, const void* wpack, const float* bias, const float* x,
                            long ldx, const long long* tok, long ldtok, int V, const float* h_prev, const float* c_prev,
                            long ldp, int n_prev, const int* src, float* h_out, float* c_out, long ldo,
                            void* hb_out, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG((wdtype == EA_F32 || wdtype == EA_BF16) && n >= 0 && I >= 1 && H >= 1);
  EA_CHECK_ARG(wpack && bias && x && h_prev && c_prev && h_out && c_out && aligned16(wpack) && aligned16(bias));
  EA_CHECK_ARG(ldx >= I && ldp >= H && ldo >= H && n_prev >= 1 && (src || n_prev >= n) && (!tok || V >= 1));
  EA_CHECK_ARG(h_out != h_prev && c_out != c_prev && h_out != c_prev && c_out != h_prev);
  if (n == 0) return 0;
  LstmP p;
  p.n = n; p.I = I; p.H = H; p.n_prev = n_prev; p.V = V;
  p.Ip = ea_cdiv(I, EA_LSTM_KG) * EA_LSTM_KG;
  p.Hp = ea_cdiv(H, EA_LSTM_KG) * EA_LSTM_KG;
  p.w = wpack; p.bias = bias; p.x = x; p.ldx = ldx; p.tok = tok; p.ldtok = ldtok;
  p.hp = h_prev; p.cp = c_prev; p.ldp = ldp; p.src = src;
  p.ho = h_out; p.co = c_out; p.ldo = ldo; p.hb = (bf16*)hb_out;
  p.xvec = aligned16(x) && ldx % 4 == 0;
  p.hvec = aligned16(h_prev) && ldp % 4 == 0;
  return wdtype == EA_BF16 ? launch_lstm_mt<true>(p, (hipStream_t)stream) : launch_lstm_mt<false>(p, (hipStream_t)stream);
}
