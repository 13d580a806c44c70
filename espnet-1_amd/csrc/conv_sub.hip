// The second convolution of Conv2dSubsampling2 / Conv2dSubsampling6
// (espnet/nets/pytorch_backend/transformer/subsampling.py:94-200): a valid C -> C convolution with
// kernel k and stride s over channel-last activations x1 (B, T1, F1, C), instantiated for
// (k, s) = (5, 3) and (3, 1), f32 and bf16.  DESIGN.md §19.
//
// hipcc-flags: -fno-slp-vectorize
//
//   conv_sub_gemm_kernel   implicit GEMM, no im2col.  A 128 x 64 output tile per block, K in chunks of
//                          32 through LDS; the next chunk is fetched into registers while the MFMAs of
//                          the current one run.  Two roles:
//                          forward   rows = the B*T2*F2 output pixels, K = (kt, kf, ci).  One kernel row
//                                    of a pixel is one contiguous run of k*C elements of x1, so an A row
//                                    is k runs and the gather has index arithmetic per kernel row only.
//                          dgrad     rows = the x1 pixels, grouped by stride residue (t1 mod s, f1 mod s):
//                                    a class receives the taps kt = t1, kf = f1 (mod s) only, so its
//                                    K = (taps of the class) * C.  One launch over all classes, the
//                                    longest K first; a tap whose source pixel is off the (T2, F2) grid
//                                    is predicated to zero, which also gives the rows and columns no
//                                    window covers their exact zeros.
//   conv_sub_wgrad_kernel  dW (Co, k*k*Ci) as a GEMM with K = pixels, x1 gathered by the forward's index
//                          law, split over pixel ranges into f32 partials the caller sums in range order.
// C is any multiple of 8: every 8-element vector is inside or outside a run / the channel range as a
// whole, and N and K tails are predicated.  No atomics: every output element has one owning thread.
#include "common.h"
#include "conv_tile.h"

namespace {

constexpr int BM = 128, BN = 64;  // output tile of conv_sub_gemm_kernel
constexpr int WT = 64;            // the weight gradient's tile: WT output channels x WT columns of a kernel row

template <typename T> struct alignas(16) Pack8 { T v[8]; };  // 16-B (bf16) / 2 x 16-B (f32) vector
// the same as a register vector (a chunk's prefetch lives in registers across the MFMA loop)
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef f32x8 f32x8a __attribute__((aligned(16)));
typedef bf16x8 bf16x8a __attribute__((aligned(16)));
template <typename T> struct Vec8;
template <> struct Vec8<float> { typedef f32x8a type; };
template <> struct Vec8<bf16> { typedef bf16x8a type; };

struct SubGeo { int B, T1, F1, T2, F2, C; };

// stride-residue class (rt, rf) of the input gradient: pixels t1 = i*s + rt, f1 = j*s + rf, i < nI,
// j < nJ, taps kt = rt + a*s (a < nkt), kf = rf + e*s (e < nkf); its M tiles start at tile0
struct DgradClass { int rt, rf, nkt, nkf, nI, nJ, tile0; };
struct DgradPlan { DgradClass c[9]; int ncls, ntiles; };

struct GemmArgs {
  SubGeo g;
  const void* src;    // forward: x1; dgrad: dY (B, T2, F2, C)
  const void* w;      // forward: (Co, k, k, Ci); dgrad: (Ci, k, k, Co)
  const float* bias;  // forward
  const void* aux;    // dgrad: x1, the ReLU mask of the layer below
  void* out;          // forward: x2 (B, T2, F2, C); dgrad: dx1 (B, T1, F1, C)
  DgradPlan plan;
};

template <typename T, int KS, int S, bool DGRAD>
__global__ __launch_bounds__(256) void conv_sub_gemm_kernel(GemmArgs a) {
  constexpr int LD = Lds<T>::LD, NI = BM / 64, NJ = BN / 16, KK = KS * KS;
  __shared__ __attribute__((aligned(16))) T As[BM * LD];
  __shared__ __attribute__((aligned(16))) T Bs[BN * LD];
  __shared__ long rsrc[BM], rout[BM];  // per tile row: first source element, output pixel (-1: no row)
  __shared__ int ri[BM], rj[BM];       // dgrad: the row's (i, j) within its class
  const SubGeo& g = a.g;
  const int C = g.C, T1 = g.T1, F1 = g.F1, T2 = g.T2, F2 = g.F2;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n0 = blockIdx.y * BN;

  DgradClass cls{};
  if constexpr (DGRAD) {
    int ci = 0;
    while (ci + 1 < a.plan.ncls && (int)blockIdx.x >= a.plan.c[ci + 1].tile0) ++ci;
    cls = a.plan.c[ci];
  }
  if (tid < BM) {
    long src = 0, out = -1;
    int i = 0, j = 0;
    if constexpr (DGRAD) {
      const long m = (long)(blockIdx.x - cls.tile0) * BM + tid;
      if (m < (long)g.B * cls.nI * cls.nJ) {
        j = (int)(m % cls.nJ);
        i = (int)((m / cls.nJ) % cls.nI);
        const long b = m / ((long)cls.nJ * cls.nI);
        src = ((b * T2 + i) * F2 + j) * C;
        out = (b * T1 + i * S + cls.rt) * F1 + j * S + cls.rf;
      }
    } else {
      const long m = (long)blockIdx.x * BM + tid;
      if (m < (long)g.B * T2 * F2) {
        const int f2 = (int)(m % F2), t2 = (int)((m / F2) % T2);
        const long b = m / ((long)F2 * T2);
        src = ((b * T1 + t2 * S) * F1 + f2 * S) * C;
        out = m;
      }
    }
    rsrc[tid] = src; rout[tid] = out; ri[tid] = i; rj[tid] = j;
  }
  __syncthreads();

  // this thread's share of a chunk: A rows arow and arow + 64, B row arow, eight K elements at ac
  const int arow = tid >> 2, ac = (tid & 3) * 8;
  long asrc[NI];
  bool aok[NI];
  int ai[NI], aj[NI];
#pragma unroll
  for (int h = 0; h < NI; ++h) {
    asrc[h] = rsrc[arow + 64 * h];
    aok[h] = rout[arow + 64 * h] >= 0;
    ai[h] = ri[arow + 64 * h];
    aj[h] = rj[arow + 64 * h];
  }
  const int bn = n0 + arow;
  const bool bok = bn < C;
  const T* X = (const T*)a.src;
  const T* W = (const T*)a.w + (long)bn * KK * C;

  // K = nruns runs of L elements, each run in chunks of KC
  const int nruns = DGRAD ? cls.nkt * cls.nkf : KS, L = DGRAD ? C : KS * C;
  const int nchunk = (L + KC - 1) / KC, niter = nruns * nchunk;

  typedef typename Vec8<T>::type V8;
  V8 ra[NI], rb;
  auto fetch = [&](int it) {
    const int run = it / nchunk, col = (it - run * nchunk) * KC + ac;
    const bool in = col < L;  // (L and col are multiples of 8: the vector is inside the run or outside)
    long aoff, woff;
    int da = 0, de = 0;
    if constexpr (DGRAD) {
      da = run / cls.nkf;
      de = run - da * cls.nkf;
      aoff = col - ((long)da * F2 + de) * C;
      woff = (long)((cls.rt + da * S) * KS + cls.rf + de * S) * C + col;
    } else {
      aoff = (long)run * F1 * C + col;
      woff = (long)run * KS * C + col;
    }
#pragma unroll
    for (int h = 0; h < NI; ++h) {
      bool ok = aok[h] && in;
      if constexpr (DGRAD) ok = ok && ai[h] >= da && ai[h] - da < T2 && aj[h] >= de && aj[h] - de < F2;
      ra[h] = V8{};
      if (ok) ra[h] = *(const V8*)(X + asrc[h] + aoff);
    }
    rb = V8{};
    if (bok && in) rb = *(const V8*)(W + woff);
  };

  f32x4 acc[NI][NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  for (int it = 0; it < niter; ++it) {
#pragma unroll
    for (int h = 0; h < NI; ++h) *(V8*)(As + (arow + 64 * h) * LD + ac) = ra[h];
    *(V8*)(Bs + arow * LD + ac) = rb;
    __syncthreads();
    if (it + 1 < niter) fetch(it + 1);
    // each 32-deep chunk sums into a fresh accumulator, the chunks into acc: the rounding error of a
    // K = 25 C sum grows with the chunk count + 32, not with K
    f32x4 part[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) part[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    chunk_mma<T, NI, NJ>(As, Bs, wv * (BM / 4), lane, part);
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] += part[i][j];
    __syncthreads();
  }

  // epilogue: this lane holds rows 4 * (lane >> 4) + r of each 16-row tile, column lane & 15
  T* O = (T*)a.out;
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long pix = rout[wv * (BM / 4) + i * 16 + 4 * (lane >> 4) + r];
      if (pix < 0) continue;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int n = n0 + j * 16 + (lane & 15);
        if (n >= C) continue;
        float v = acc[i][j][r];
        if constexpr (DGRAD) {
          v = to_f(((const T*)a.aux)[pix * C + n]) > 0.f ? v : 0.f;
        } else {
          v += a.bias[n];
          v = v > 0.f ? v : 0.f;
        }
        O[pix * C + n] = from_f<T>(v);
      }
    }
}

struct WgradArgs {
  SubGeo g;
  const void* x1;
  const void* dy;
  float* part;
  int chunks_per_split, ntn;  // ntn: column tiles per kernel row
};

// part[split][co][kt][kf][ci] = sum over the split's output pixels p of dY[p][co] * x1[p's window at (kt, kf)][ci]
template <typename T, int KS, int S>
__global__ __launch_bounds__(256) void conv_sub_wgrad_kernel(WgradArgs a) {
  constexpr int LD = Lds<T>::LD, NJ = WT / 16;
  __shared__ __attribute__((aligned(16))) T Ys[WT * LD];
  __shared__ __attribute__((aligned(16))) T Xs[WT * LD];
  const SubGeo& g = a.g;
  const int C = g.C, T1 = g.T1, F1 = g.F1, T2 = g.T2, F2 = g.F2, L = KS * C;
  const long P = (long)g.B * T2 * F2;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int kt = blockIdx.y / a.ntn, n0 = (blockIdx.y - kt * a.ntn) * WT, co0 = blockIdx.z * WT;
  const long p_beg = (long)blockIdx.x * a.chunks_per_split * KC;
  long p_end = p_beg + (long)a.chunks_per_split * KC;
  if (p_end > P) p_end = P;
  const T* X = (const T*)a.x1;
  const T* DY = (const T*)a.dy;
  // this thread's share of a chunk: pixel pl, eight channels / columns at c0, staged transposed
  const int pl = tid >> 3, c0 = (tid & 7) * 8;
  const bool yok = co0 + c0 < C, xok = n0 + c0 < L;

  f32x4 acc[1][NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[0][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (long p0 = p_beg; p0 < p_end; p0 += KC) {
    const long p = p0 + pl;
    Pack8<T> y{}, x{};
    if (p < p_end) {
      if (yok) y = *(const Pack8<T>*)(DY + p * C + co0 + c0);
      if (xok) {
        const int f2 = (int)(p % F2), t2 = (int)((p / F2) % T2);
        const long b = p / ((long)F2 * T2);
        x = *(const Pack8<T>*)(X + ((b * T1 + t2 * S + kt) * F1 + f2 * S) * C + n0 + c0);
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      Ys[(c0 + e) * LD + pl] = y.v[e];
      Xs[(c0 + e) * LD + pl] = x.v[e];
    }
    __syncthreads();
    chunk_mma<T, 1, NJ>(Ys, Xs, wv * 16, lane, acc);
    __syncthreads();
  }
  float* out = a.part + (long)blockIdx.x * C * KS * L;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int co = co0 + wv * 16 + 4 * (lane >> 4) + r;
    if (co >= C) continue;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int n = n0 + j * 16 + (lane & 15);
      if (n < L) out[((long)co * KS + kt) * L + n] = acc[0][j][r];
    }
  }
}

// lengths as the reference derives them from the sliced mask x_mask[:, :, :-2:2][:, :, :-(k-1):s]
// (subsampling.py:149, 200): l -> ceil(min(l, T-2) / 2) -> ceil(min(., T1-(k-1)) / s)
__global__ void subsample_lens_ks_kernel(int B, int T, int k, int s, const long long* __restrict__ ilens,
                                         long long* __restrict__ olens) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const long long T1 = (T - 1) / 2;  // len(range(0, T-2, 2))
  long long l1 = min(ilens[b], (long long)T - 2);
  l1 = l1 > 0 ? (l1 + 1) / 2 : 0;
  long long l2 = min(l1, T1 - (k - 1));
  olens[b] = l2 > 0 ? (l2 + s - 1) / s : 0;
}

bool geo_ok(int B, int T1, int F1, int C, int k, int s) {
  return B > 0 && C > 0 && C % 8 == 0 && T1 >= k && F1 >= k && ((k == 5 && s == 3) || (k == 3 && s == 1));
}

SubGeo make_geo(int B, int T1, int F1, int C, int k, int s) {
  return SubGeo{B, T1, F1, (T1 - k) / s + 1, (F1 - k) / s + 1, C};
}

// the classes that hold pixels, longest K first (ties in (rt, rf) order), with their M tiles
DgradPlan make_plan(const SubGeo& g, int k, int s) {
  DgradPlan p{};
  for (int want = k * k; want > 0; --want)
    for (int rt = 0; rt < s; ++rt)
      for (int rf = 0; rf < s; ++rf) {
        const int nkt = (k - rt + s - 1) / s, nkf = (k - rf + s - 1) / s;
        const int nI = (g.T1 - rt + s - 1) / s, nJ = (g.F1 - rf + s - 1) / s;
        if (nkt * nkf != want || nI <= 0 || nJ <= 0) continue;
        p.c[p.ncls++] = DgradClass{rt, rf, nkt, nkf, nI, nJ, p.ntiles};
        p.ntiles += (int)(((long)g.B * nI * nJ + BM - 1) / BM);
      }
  return p;
}

// the weight gradient's pixel ranges: `cps` whole 32-pixel chunks each; enough ranges to fill the
// device when the (co, kt, column) tiles alone do not, at most 128
struct WgradRanges { int nsplit, cps, ntn; };
WgradRanges wgrad_ranges(const SubGeo& g, int k) {
  const long chunks = ((long)g.B * g.T2 * g.F2 + KC - 1) / KC;
  const int ntn = (k * g.C + WT - 1) / WT;
  const long tiles = (long)((g.C + WT - 1) / WT) * k * ntn;
  long want = (2048 + tiles - 1) / tiles;
  if (want > 128) want = 128;
  if (want > chunks) want = chunks;
  const long cps = (chunks + want - 1) / want;
  return WgradRanges{(int)((chunks + cps - 1) / cps), (int)cps, ntn};
}

template <typename T, bool DGRAD>
void launch_gemm(int k, const GemmArgs& a, dim3 grid, hipStream_t st) {
  if (k == 5) conv_sub_gemm_kernel<T, 5, 3, DGRAD><<<grid, 256, 0, st>>>(a);
  else conv_sub_gemm_kernel<T, 3, 1, DGRAD><<<grid, 256, 0, st>>>(a);
}

}  // namespace

extern "C" {

int ea_conv_sub_fwd(int B, int T1, int F1, int C, int k, int s, int dtype, const void* x1, const void* w,
                    const float* bias, void* x2, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(geo_ok(B, T1, F1, C, k, s) && x1 && w && bias && x2);
  EA_CHECK_ARG(dtype == EA_F32 || dtype == EA_BF16);
  GemmArgs a{make_geo(B, T1, F1, C, k, s), x1, w, bias, nullptr, x2, DgradPlan{}};
  const long tiles = ((long)a.g.B * a.g.T2 * a.g.F2 + BM - 1) / BM;
  EA_CHECK_ARG(tiles < (1L << 31));
  const dim3 grid((unsigned)tiles, (a.g.C + BN - 1) / BN);
  if (dtype == EA_F32) launch_gemm<float, false>(k, a, grid, (hipStream_t)stream);
  else launch_gemm<bf16, false>(k, a, grid, (hipStream_t)stream);
  EA_LAUNCH_CHECK();
  return 0;
}

int ea_conv_sub_dgrad(int B, int T1, int F1, int C, int k, int s, int dtype, const void* dy, const void* wt,
                      const void* x1, void* dx1, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(geo_ok(B, T1, F1, C, k, s) && dy && wt && x1 && dx1);
  EA_CHECK_ARG(dtype == EA_F32 || dtype == EA_BF16);
  GemmArgs a{make_geo(B, T1, F1, C, k, s), dy, wt, nullptr, x1, dx1, DgradPlan{}};
  a.plan = make_plan(a.g, k, s);
  const dim3 grid(a.plan.ntiles, (a.g.C + BN - 1) / BN);
  if (dtype == EA_F32) launch_gemm<float, true>(k, a, grid, (hipStream_t)stream);
  else launch_gemm<bf16, true>(k, a, grid, (hipStream_t)stream);
  EA_LAUNCH_CHECK();
  return 0;
}

int ea_conv_sub_wgrad_splits(int B, int T1, int F1, int C, int k, int s, int* nsplit) {
  EA_CHECK_ARG(geo_ok(B, T1, F1, C, k, s) && nsplit);
  *nsplit = wgrad_ranges(make_geo(B, T1, F1, C, k, s), k).nsplit;
  return 0;
}

int ea_conv_sub_wgrad(int B, int T1, int F1, int C, int k, int s, int dtype, const void* x1, const void* dy,
                      float* part, int nsplit, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(geo_ok(B, T1, F1, C, k, s) && x1 && dy && part);
  EA_CHECK_ARG(dtype == EA_F32 || dtype == EA_BF16);
  const SubGeo g = make_geo(B, T1, F1, C, k, s);
  const WgradRanges rg = wgrad_ranges(g, k);
  EA_CHECK_ARG(nsplit == rg.nsplit);
  EA_CHECK_ARG((long)k * rg.ntn <= 65535 && (g.C + WT - 1) / WT <= 65535);
  WgradArgs a{g, x1, dy, part, rg.cps, rg.ntn};
  const dim3 grid(nsplit, k * rg.ntn, (g.C + WT - 1) / WT);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EA_F32) {
    if (k == 5) conv_sub_wgrad_kernel<float, 5, 3><<<grid, 256, 0, st>>>(a);
    else conv_sub_wgrad_kernel<float, 3, 1><<<grid, 256, 0, st>>>(a);
  } else {
    if (k == 5) conv_sub_wgrad_kernel<bf16, 5, 3><<<grid, 256, 0, st>>>(a);
    else conv_sub_wgrad_kernel<bf16, 3, 1><<<grid, 256, 0, st>>>(a);
  }
  EA_LAUNCH_CHECK();
  return 0;
}

int ea_subsample_lens_ks(int B, int T, int k, int s, const long long* ilens, long long* olens, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(B > 0 && k > 0 && s > 0 && ilens && olens);
  subsample_lens_ks_kernel<<<ea_cdiv(B, 64), 64, 0, (hipStream_t)stream>>>(B, T, k, s, ilens, olens);
  EA_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
