// The weight-stream core of the LSTM kernels: lstm_step_kernel (rnn_lm.hip), lstm_cell_fwd_kernel
// and lstm_cell_bwd_kernel (lstm_train.hip), and their two-direction, length-masked forms
// lstm_bicell_fwd_kernel and lstm_bicell_bwd_kernel (lstm_bidir.hip).
//
// A launch is rows (n hypotheses or a training batch) x a packed weight: a few MFMAs per 16-B
// weight load.  A block owns MT 16-row tiles (up to 64 rows) x NJ 16-row weight tiles and ALL of
// K, so for n <= 64 every weight element is loaded from memory once per launch; rows beyond 64
// go to further block rows (grid.y), which re-read the weights from L2 / MALL.  The block's NW
// waves split K (wave w takes the slices w, w + NW, ...), each issuing the loads of U slices
// before its first MFMA (a two-stage register pipeline of half the depth measured no faster,
// DESIGN.md section 11).  Operands go global -> registers in MFMA fragment order with no LDS
// staging (a weight is used once per block and is not shared between waves), as gemm_skinny.hip
// does.  The waves' partial tiles are summed through LDS and the epilogue runs on the sums in
// f32.  No block waits for another.
//
// Packed weights: the slice-major tile layout of include/espnet_amd.h ("LSTM weight packs"),
// made by espnet_amd/lm/lstm_pack.py; the 64 16-B loads of a wave for one slice cover one
// contiguous 1-KB piece.
#pragma once
#include <type_traits>

#include "common.h"

namespace lstm_core {

constexpr int NW = 8;  // waves per block (K split)

template <bool BF> struct Frag;
template <> struct Frag<false> { typedef f32x4 T; typedef float W; };
template <> struct Frag<true> { typedef bf16x8 T; typedef bf16 W; };

template <int N> using Int = std::integral_constant<int, N>;

EA_DEV float sigmoid_exact(float x) { return 1.f / (1.f + expf(-x)); }
inline bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

// the operand row of the lane in row tile i of the block at r0; rows >= n compute on row 0's
// operands and are never stored
EA_DEV int lane_row(int r0, int i, int n) {
  const int row = r0 + i * 16 + (threadIdx.x & 15);
  return row < n ? row : 0;
}

// the lane's AN operand elements k .. k + AN - 1 of a row of S (f32 -> f32 fragment, f32 -> bf16
// fragment rounded in registers, bf16 -> bf16 fragment); elements >= lim are 0.
// `fast` (wave-uniform): the whole slice lies below lim and the row is 16-B aligned.
template <bool BF, typename S>
EA_DEV typename Frag<BF>::T load_a(const S* __restrict__ row, int k, int lim, bool fast) {
  constexpr int AN = BF ? 8 : 4, CH = 16 / sizeof(S);
  typedef __attribute__((ext_vector_type(CH))) S chunk;
  const S* p = row + k;
  S v[AN];
  if (fast) {
#pragma unroll
    for (int q = 0; q < AN / CH; ++q) {
      const chunk f = *(const chunk*)(p + CH * q);
#pragma unroll
      for (int e = 0; e < CH; ++e) v[CH * q + e] = f[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < AN; ++e) v[e] = k + e < lim ? p[e] : (S)0.f;
  }
  typename Frag<BF>::T out;
#pragma unroll
  for (int e = 0; e < AN; ++e) out[e] = (typename Frag<BF>::W)v[e];
  return out;
}

// A operand of block_product: d = la.slice(s) is what K slice s needs that is the same for every
// row tile (taken outside the branch on s < nks, as the scalar unit's work), la(i, d, k0) the
// lane's fragment of row tile i, the elements k0 .. k0 + AN - 1 of the slice.
// RowsA: one K segment, elements [0, lim) of MT rows of S.
template <bool BF, int MT, typename S>
struct RowsA {
  const S* row[MT];
  int lim;
  bool vec;  // rows 16-B aligned
  struct Slice { int s; bool fast; };
  EA_DEV Slice slice(int s) const { return Slice{s, vec && (s + 1) * (BF ? 32 : 16) <= lim}; }
  EA_DEV typename Frag<BF>::T operator()(int i, const Slice& d, int k0) const {
    return load_a<BF>(row[i], d.s * (BF ? 32 : 16) + k0, lim, d.fast);
  }
};
// RowsXH: the two segments [x | h_prev] of the decoding step, slices [0, nkx) from x (I
// elements), the rest from h (H elements), each with its own alignment flag.
template <bool BF, int MT>
struct RowsXH {
  const float* x[MT];
  const float* h[MT];
  int nkx, I, H;
  int xvec, hvec;
  struct Slice { bool isx; int sl, lim; bool fast; };
  EA_DEV Slice slice(int s) const {
    constexpr int SL = BF ? 32 : 16;
    Slice d;
    d.isx = s < nkx;
    d.sl = d.isx ? s : s - nkx;
    d.lim = d.isx ? I : H;
    d.fast = (d.isx ? xvec : hvec) && (d.sl + 1) * SL <= d.lim;
    return d;
  }
  EA_DEV typename Frag<BF>::T operator()(int i, const Slice& d, int k0) const {
    constexpr int SL = BF ? 32 : 16;
    return load_a<BF>(d.isx ? x[i] : h[i], d.sl * SL + k0, d.lim, d.fast);
  }
};

// A(rows of the block, K) . pack(column tiles t0 .. t0 + NJ - 1)^T summed over the block's waves:
// on return red[q][row][col], q < NW / 2, hold four partial sums of every element (sum_partials
// adds them).
template <bool BF, int MT, int NJ, int U, class LoadA>
EA_DEV void block_product(const LoadA& la, const void* wpack, int nks, int t0, int ntiles,
                          float (*red)[16 * MT][16 * NJ + 4]) {
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

  for (int s0 = w; s0 < nks; s0 += NW * U) {
    frag a[U][MT], b[U][NJ];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int s = s0 + u * NW;
      const bool in = s < nks;
#pragma unroll
      for (int j = 0; j < NJ; ++j) b[u][j] = in && bok[j] ? *(const frag*)(bp[j] + (long)s * 16 * SL) : zero;
      const auto d = la.slice(s);
#pragma unroll
      for (int i = 0; i < MT; ++i) a[u][i] = in ? la(i, d, g * AN) : zero;
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
  if (w >= NW / 2) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[w - NW / 2][i * 16 + 4 * g + r][j * 16 + lr] = acc[i][j][r];
  }
  __syncthreads();
  if (w < NW / 2) {
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

// the sum of block_product's partials at (lrow, col ..): V = float, or float4 for four columns
template <typename V, int BR, int LD>
EA_DEV V sum_partials(const float (*red)[BR][LD], int lrow, int col) {
  V s = *(const V*)&red[0][lrow][col];
#pragma unroll
  for (int q = 1; q < NW / 2; ++q) s += *(const V*)&red[q][lrow][col];
  return s;
}

// zeros in the columns [c0, ld) of the block's rows (< n) of a, b and hb (b, hb: or NULL), by
// the last block of the row group: later launches read them against zero weight columns
template <int BR>
EA_DEV void zero_pad(int r0, int n, int c0, long ld, float* a, float* b, bf16* hb) {
  if (blockIdx.x != gridDim.x - 1) return;
  const int padw = (int)(ld - c0);
  const int rows = min(BR, n - r0);
  for (int idx = threadIdx.x; idx < rows * padw; idx += 64 * NW) {
    const long o = (long)(r0 + idx / padw) * ld + c0 + idx % padw;
    a[o] = 0.f;
    if (b) b[o] = 0.f;
    if (hb) hb[o] = (bf16)0.f;
  }
}

// Row masks of the cell epilogues.  AllRows: every row of the launch takes the cell update (the
// test folds away).  A mask whose operator()(row) is false makes the epilogue store zeros for
// that row in place of the update (lstm_bidir.hip: the frames past a sequence's length).
struct AllRows {
  EA_DEV bool operator()(int) const { return true; }
};

// The forward cell update on block_product's sums, a tile being 4 hidden units x the 4 gates
// (torch order i, f, g, o): gates = sums + add(row, unit) (a float4), c = sigmoid(f) *
// cprev(row, unit) + sigmoid(i) * tanh(g), h = sigmoid(o) * tanh(c).  Stores h, c, the bf16 h
// (hb or NULL) and the four activated gates (gates or NULL) and zeroes the pad columns [H, ldo).
// Rows with !active(row) store h = c = 0 and zero gates.
template <int MT, int NJ, class Add, class CPrev, class Active>
EA_DEV void cell_fwd_epilogue(const float (*red)[16 * MT][16 * NJ + 4], int r0, int t0, int n, int H, const Add& add,
                              const CPrev& cprev, float* ho, float* co, bf16* hb, long ldo, float* gates, long ldg,
                              const Active& active) {
  constexpr int CELLS = 16 * MT * NJ * 4;  // (row, hidden unit) pairs of the block
  for (int ci = threadIdx.x; ci < CELLS; ci += 64 * NW) {
    const int lrow = ci / (NJ * 4), cu = ci % (NJ * 4);  // cu = 4 * (tile in block) + unit in tile
    const int row = r0 + lrow, unit = t0 * 4 + cu;
    if (row >= n || unit >= H) continue;
    if (!active(row)) {
      co[(long)row * ldo + unit] = 0.f;
      ho[(long)row * ldo + unit] = 0.f;
      if (hb) hb[(long)row * ldo + unit] = (bf16)0.f;
      if (gates) *(float4*)(gates + (long)row * ldg + 4 * unit) = make_float4(0.f, 0.f, 0.f, 0.f);
      continue;
    }
    const float4 s = sum_partials<float4>(red, lrow, cu * 4);
    const float4 ad = add(row, unit);
    const float cp = cprev(row, unit);
    const float gi = sigmoid_exact(s.x + ad.x), gf = sigmoid_exact(s.y + ad.y);
    const float gg = tanhf(s.z + ad.z), go = sigmoid_exact(s.w + ad.w);
    const float c = gf * cp + gi * gg;
    const float h = go * tanhf(c);
    co[(long)row * ldo + unit] = c;
    ho[(long)row * ldo + unit] = h;
    if (hb) hb[(long)row * ldo + unit] = (bf16)h;
    if (gates) *(float4*)(gates + (long)row * ldg + 4 * unit) = make_float4(gi, gf, gg, go);
  }
  zero_pad<16 * MT>(r0, n, H, ldo, ho, co, hb);
}
template <int MT, int NJ, class Add, class CPrev>
EA_DEV void cell_fwd_epilogue(const float (*red)[16 * MT][16 * NJ + 4], int r0, int t0, int n, int H, const Add& add,
                              const CPrev& cprev, float* ho, float* co, bf16* hb, long ldo, float* gates, long ldg) {
  cell_fwd_epilogue<MT, NJ>(red, r0, t0, n, H, add, cprev, ho, co, hb, ldo, gates, ldg, AllRows{});
}

// The backward cell update of the block's 16 hidden units (column tile t0) on block_product's
// sums: dh = dh_out + the sums (`rec`: block-uniform, false = no recurrent term yet), then the
// cell's gradient (ea_lstm_cell_bwd in include/espnet_amd.h).  P names one step's operands: n, H,
// G = 4H, dho / lddh, gates / ldg, c, cprev / ldc, dci, dco / lddc, dg, dgb / ldd, dht / ldt.
// Stores dgates (torch gate order), their bf16 copy (dgb or NULL), the carry dc_out and dh (dht or
// NULL) and zeroes the pad columns [4H, ldd) of dgates and [H, lddc) of the carry.  Rows with
// !active(row) store zero dgates and a zero carry.
template <int MT, class P, class Active>
EA_DEV void cell_bwd_epilogue(const float (*red)[16 * MT][16 + 4], bool rec, int r0, int t0, const P& p,
                              const Active& active) {
  constexpr int CELLS = 16 * MT * 16;
  for (int ci = threadIdx.x; ci < CELLS; ci += 64 * NW) {
    const int lrow = ci / 16, cu = ci % 16;
    const int row = r0 + lrow, unit = t0 * 16 + cu;
    if (row >= p.n || unit >= p.H) continue;
    if (!active(row)) {
      float* o = p.dg + (long)row * p.ldd + unit;
      p.dco[(long)row * p.lddc + unit] = 0.f;
      o[0] = 0.f; o[p.H] = 0.f; o[2 * (long)p.H] = 0.f; o[3 * (long)p.H] = 0.f;
      if (p.dgb) {
        bf16* ob = p.dgb + (long)row * p.ldd + unit;
        ob[0] = (bf16)0.f; ob[p.H] = (bf16)0.f; ob[2 * (long)p.H] = (bf16)0.f; ob[3 * (long)p.H] = (bf16)0.f;
      }
      if (p.dht) p.dht[(long)row * p.ldt + unit] = 0.f;
      continue;
    }
    float dh = p.dho ? p.dho[(long)row * p.lddh + unit] : 0.f;
    if (rec) dh += sum_partials<float>(red, lrow, cu);
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

  // pad columns [4H, ldd) of dgates and [H, lddc) of the carry
  zero_pad<16 * MT>(r0, p.n, p.G, p.ldd, p.dg, nullptr, p.dgb);
  zero_pad<16 * MT>(r0, p.n, p.H, p.lddc, p.dco, nullptr, nullptr);
}

// Row-tile dispatch: MT = 1 / 2 / 4 row tiles per block for n <= 16 / <= 32 / more, NJ = 2 column
// tiles per block when `wide`, U = 8 slices in flight (4 with MT = 4).  kern(Int<MT>, Int<NJ>,
// Int<U>) names the instantiation; ctiles = the column tiles of the launch, nz = its grid.z (the
// directions of lstm_bidir.hip).
template <class P, class Kern>
int launch_tiles(int n, int ctiles, bool wide, const P& p, hipStream_t st, Kern kern, int nz = 1) {
  auto go = [&](auto mt, auto nj) {
    const dim3 grid(ea_cdiv(ctiles, nj()), ea_cdiv(n, 16 * mt()), nz);
    hipLaunchKernelGGL(kern(mt, nj, Int<(mt() == 4 ? 4 : 8)>()), grid, dim3(64 * NW), 0, st, p);
    EA_LAUNCH_CHECK();
    return 0;
  };
  if (n <= 16) return wide ? go(Int<1>(), Int<2>()) : go(Int<1>(), Int<1>());
  if (n <= 32) return wide ? go(Int<2>(), Int<2>()) : go(Int<2>(), Int<1>());
  return wide ? go(Int<4>(), Int<2>()) : go(Int<4>(), Int<1>());
}

}  // namespace lstm_core
