// VGG2L (espnet/nets/pytorch_backend/rnn/encoders.py:178-237): the four 3x3 stride-1 pad-1
// convolutions of `encoder: vgg_rnn` over channel-last activations, f32 and bf16.  DESIGN.md §16.
//
// hipcc-flags: -fno-slp-vectorize
//
//   vgg_conv_kernel   implicit GEMM, no im2col: M = pixels, N = Cout, K = 9*Cin in (tap, ci) order.
//                     f32 on v_mfma_f32_16x16x4_f32, bf16 on v_mfma_f32_16x16x32_bf16, f32 accumulate.
//                     A tile is 64 rows = 16 pooling windows x their 4 positions, so a lane's four
//                     accumulator registers are one window: bias + ReLU + 2x2 max-pool happen in
//                     registers.  The same kernel is the input gradient (flipped taps over a
//                     (Cin, 9, Cout) weight) and reads a pooled gradient through the saved decisions.
//   vgg_wgrad_kernel  dW as a GEMM with K = pixels, split over pixel ranges into partials.
//   conv1_1 (Cin = 1) vector kernels; its weight / bias gradients as block partials.
// No atomics anywhere: every output element has one owning thread and every sum a fixed order.
#include "common.h"

namespace {

constexpr int KC = 32;  // K elements per LDS chunk (channels of one tap / pixels of the wgrad)

template <typename T> struct Lds;
template <> struct Lds<float> { static constexpr int LD = KC + 4; };
template <> struct Lds<bf16> { static constexpr int LD = KC + 8; };

// decision byte of a pooled element: bits 0-1 argmax = 2*dt + df, bit 2 + pos = (pre-activation of
// window position pos > 0)
EA_DEV bool dec_pass(unsigned d, int code) { return (d & 3u) == (unsigned)code && ((d >> (2 + code)) & 1u); }

// the geometry of one launch: the geo / strides arrays of the C ABI (EA_VGG_*)
struct VggGeo {
  int B, H, W, cin, cout, src, epi, flip, out_dtype;
  long ps_b, ps_h, ps_w, ps_c, po_b, po_h, po_w, po_c;
};

struct PooledSrc {
  const float* dp;
  const unsigned char* dec;
  long sb, sh, sw, sc;
};

// eight channels c0 .. c0+7 of the full-resolution gradient at (b, h, w), scattered from the pooled
// gradient by the saved decisions
EA_DEV void pooled_load8(const PooledSrc& s, int b, int h, int w, int c0, float (&v)[8]) {
  const long base = b * s.sb + (h >> 1) * s.sh + (w >> 1) * s.sw;
  const int code = (h & 1) * 2 + (w & 1);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const long i = base + (c0 + e) * s.sc;
    v[e] = dec_pass(s.dec[i], code) ? s.dp[i] : 0.f;
  }
}

template <typename T>
EA_DEV void plain_load8(const T* p, float (&v)[8]) {
  float a[4], b[4];
  vld4(p, a);
  vld4(p + 4, b);
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
}

template <typename T>
EA_DEV void lds_store8(T* p, const float (&v)[8]) {
  const float a[4] = {v[0], v[1], v[2], v[3]}, b[4] = {v[4], v[5], v[6], v[7]};
  vst4(p, a);
  vst4(p + 4, b);
}

// one chunk's MFMAs of a wave: rows arow (NI tiles of 16) of As against NJ column tiles of Bs
template <typename T, int NI, int NJ>
EA_DEV void chunk_mma(const T* As, const T* Bs, int arow, int lane, f32x4 (&acc)[NI][NJ]) {
  constexpr int LD = Lds<T>::LD;
  const int r = lane & 15, q = lane >> 4;
  if constexpr (sizeof(T) == 2) {
    bf16x8 fa[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) fa[i] = *(const bf16x8*)(As + (arow + i * 16 + r) * LD + 8 * q);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const bf16x8 fb = *(const bf16x8*)(Bs + (j * 16 + r) * LD + 8 * q);
#pragma unroll
      for (int i = 0; i < NI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb, acc[i][j], 0, 0, 0);
    }
  } else {
#pragma unroll
    for (int ks = 0; ks < KC / 4; ++ks) {
      float fa[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) fa[i] = As[(arow + i * 16 + r) * LD + ks * 4 + q];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float fb = Bs[(j * 16 + r) * LD + ks * 4 + q];
#pragma unroll
        for (int i = 0; i < NI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb, acc[i][j], 0, 0, 0);
      }
    }
  }
}

struct ConvArgs {
  VggGeo g;
  const void* x;
  PooledSrc ps;
  const void* w;
  const float* bias;
  const void* aux;
  void* out;
  unsigned char* dec_out;
};

template <typename T, int N>
__global__ __launch_bounds__(256) void vgg_conv_kernel(ConvArgs a) {
  constexpr int LD = Lds<T>::LD, NJ = N / 16;
  __shared__ __attribute__((aligned(16))) T As[64 * LD];
  __shared__ __attribute__((aligned(16))) T Bs[N * LD];
  const VggGeo& g = a.g;
  const int H = g.H, W = g.W, Cin = g.cin, H2 = (H + 1) >> 1, W2 = (W + 1) >> 1;
  const long Q = (long)g.B * H2 * W2;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

  // this thread's A row: tile row tid >> 2 = (window, position), eight channels at 8 * (tid & 3)
  const int arow = tid >> 2, ac = (tid & 3) * 8;
  int ab = 0, ah = 0, aw = 0;
  bool avalid;
  {
    const long q = (long)blockIdx.x * 16 + (arow >> 2);
    const int pos = arow & 3;
    avalid = q < Q;
    if (avalid) {
      const int w2 = (int)(q % W2), h2 = (int)((q / W2) % H2);
      ab = (int)(q / ((long)W2 * H2));
      ah = 2 * h2 + (pos >> 1);
      aw = 2 * w2 + (pos & 1);
      avalid = ah < H && aw < W;
    }
  }
  const T* X = (const T*)a.x;
  const T* Wt = (const T*)a.w;
  const int nchunk = Cin / KC, niter = 9 * nchunk;
  constexpr int NB = N / 64;  // B rows per thread: row tid >> 2 + 64 * i

  float ra[8], rb[NB][8];
  auto fetch = [&](int it) {
    const int tap = it / nchunk, c0 = (it - tap * nchunk) * KC;
    const int hs = ah + tap / 3 - 1, ws = aw + tap % 3 - 1;
#pragma unroll
    for (int e = 0; e < 8; ++e) ra[e] = 0.f;
    if (avalid && hs >= 0 && hs < H && ws >= 0 && ws < W) {
      if (g.src == EA_VGG_SRC_POOLED)
        pooled_load8(a.ps, ab, hs, ws, c0 + ac, ra);
      else
        plain_load8(X + (((long)ab * H + hs) * W + ws) * Cin + c0 + ac, ra);
    }
    const int wtap = g.flip ? 8 - tap : tap;
#pragma unroll
    for (int i = 0; i < NB; ++i)
      plain_load8(Wt + ((long)(arow + 64 * i) * 9 + wtap) * Cin + c0 + ac, rb[i]);
  };

  f32x4 acc[1][NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[0][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  for (int it = 0; it < niter; ++it) {
    lds_store8(As + arow * LD + ac, ra);
#pragma unroll
    for (int i = 0; i < NB; ++i) lds_store8(Bs + (arow + 64 * i) * LD + ac, rb[i]);
    __syncthreads();
    if (it + 1 < niter) fetch(it + 1);
    // each 32-deep chunk sums into a fresh accumulator, the chunks into acc: the rounding error of a
    // K = 1152 sum grows with the 36 + 32 terms of the longest chain, not with 1152
    f32x4 part[1][NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) part[0][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    chunk_mma<T, 1, NJ>(As, Bs, wv * 16, lane, part);
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[0][j] += part[0][j];
    __syncthreads();
  }

  // epilogue: this lane holds window (wave, lane >> 4), positions 0..3 in its registers, column n
  const long q = (long)blockIdx.x * 16 + wv * 4 + (lane >> 4);
  if (q >= Q) return;
  const int w2 = (int)(q % W2), h2 = (int)((q / W2) % H2), b = (int)(q / ((long)W2 * H2));
  bool ok[4];
  long pix[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int h = 2 * h2 + (r >> 1), w = 2 * w2 + (r & 1);
    ok[r] = h < H && w < W;
    pix[r] = ((long)b * H + h) * W + w;
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int n = j * 16 + (lane & 15);
    const float bv = a.bias ? a.bias[n] : 0.f;
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = acc[0][j][r] + bv;
    if (g.epi == EA_VGG_EPI_POOL) {
      // torch's max_pool2d over relu(v): dt outer, df inner, strict >, so a tie keeps the first
      unsigned d = v[0] > 0.f ? 4u : 0u;
      float best = fmaxf(v[0], 0.f);
      unsigned arg = 0;
#pragma unroll
      for (int r = 1; r < 4; ++r) {
        if (!ok[r]) continue;
        if (v[r] > 0.f) d |= 4u << r;
        if (v[r] > best) { best = v[r]; arg = r; }
      }
      const long o = b * g.po_b + h2 * g.po_h + w2 * g.po_w + n * g.po_c;
      store_from_f(a.out, o, g.out_dtype, best);
      a.dec_out[o] = (unsigned char)(d | arg);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (!ok[r]) continue;
        const long o = pix[r] * N + n;
        float y = v[r];
        if (g.epi == EA_VGG_EPI_RELU) y = y > 0.f ? y : 0.f;
        if (g.epi == EA_VGG_EPI_MASK) y = to_f(((const T*)a.aux)[o]) > 0.f ? y : 0.f;
        store_from_f(a.out, o, g.out_dtype, y);
      }
    }
  }
}

struct WgradArgs {
  VggGeo g;
  const void* x;
  const void* dy;
  PooledSrc ps;
  float* part;
  int chunks_per_split;
};

// part[split][co][tap][ci] = sum over the split's pixels of dY[p][co] * X[p + tap][ci]
template <typename T, int CO, int CI>
__global__ __launch_bounds__(256) void vgg_wgrad_kernel(WgradArgs a) {
  constexpr int LD = Lds<T>::LD, NI = CO / 64, NJ = CI / 16;
  __shared__ __attribute__((aligned(16))) T Ys[CO * LD];
  __shared__ __attribute__((aligned(16))) T Xs[CI * LD];
  const VggGeo& g = a.g;
  const int H = g.H, W = g.W;
  const long P = (long)g.B * H * W;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int tap = blockIdx.y, dh = tap / 3 - 1, dw = tap % 3 - 1;
  const long p_beg = (long)blockIdx.x * a.chunks_per_split * KC;
  long p_end = p_beg + (long)a.chunks_per_split * KC;
  if (p_end > P) p_end = P;
  const T* X = (const T*)a.x;
  const T* DY = (const T*)a.dy;

  f32x4 acc[NI][NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (long p0 = p_beg; p0 < p_end; p0 += KC) {
    // transposed staging: [channel][pixel of the chunk]
    for (int t = tid; t < KC * (CO / 8); t += 256) {
      const int pl = t / (CO / 8), c0 = (t % (CO / 8)) * 8;
      const long p = p0 + pl;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
      if (p < p_end) {
        if (g.src == EA_VGG_SRC_POOLED) {
          const int w = (int)(p % W), h = (int)((p / W) % H), b = (int)(p / ((long)W * H));
          pooled_load8(a.ps, b, h, w, c0, v);
        } else {
          plain_load8(DY + p * CO + c0, v);
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) Ys[(c0 + e) * LD + pl] = from_f<T>(v[e]);
    }
    for (int t = tid; t < KC * (CI / 8); t += 256) {
      const int pl = t / (CI / 8), c0 = (t % (CI / 8)) * 8;
      const long p = p0 + pl;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
      if (p < p_end) {
        const int w = (int)(p % W), h = (int)((p / W) % H);
        const int hs = h + dh, ws = w + dw;
        if (hs >= 0 && hs < H && ws >= 0 && ws < W) plain_load8(X + (p + (long)dh * W + dw) * CI + c0, v);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) Xs[(c0 + e) * LD + pl] = from_f<T>(v[e]);
    }
    __syncthreads();
    chunk_mma<T, NI, NJ>(Ys, Xs, wv * (CO / 4), lane, acc);
    __syncthreads();
  }
  float* out = a.part + (long)blockIdx.x * CO * 9 * CI;
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = wv * (CO / 4) + i * 16 + 4 * (lane >> 4) + r, ci = j * 16 + (lane & 15);
        out[((long)co * 9 + tap) * CI + ci] = acc[i][j][r];
      }
}

// part[block][c] = sum of the pooled gradient over the block's pooled pixels whose winner is active
__global__ __launch_bounds__(256) void vgg_pool_dbias_kernel(int C, long Q, int W2, int H2, PooledSrc s, float* part,
                                                            long q_per_block) {
  __shared__ float red[256];
  const int tid = threadIdx.x, c = tid % C, sub = tid / C, nsub = 256 / C;
  const long q0 = blockIdx.x * q_per_block;
  long q1 = q0 + q_per_block;
  if (q1 > Q) q1 = Q;
  float sum = 0.f;
  for (long q = q0 + sub; q < q1; q += nsub) {
    const int w2 = (int)(q % W2), h2 = (int)((q / W2) % H2);
    const long b = q / ((long)W2 * H2);
    const long i = b * s.sb + h2 * s.sh + w2 * s.sw + c * s.sc;
    const unsigned d = s.dec[i];
    if ((d >> (2 + (d & 3u))) & 1u) sum += s.dp[i];
  }
  red[tid] = sum;
  __syncthreads();
  if (tid < C) {
    float t = 0.f;
    for (int k = 0; k < nsub; ++k) t += red[k * C + tid];
    part[(long)blockIdx.x * C + tid] = t;
  }
}

// ------------------------------------------------------------------ conv1_1 (Cin = 1)
template <typename T>
__global__ __launch_bounds__(256) void vgg_conv1_fwd_kernel(int B, int H, int W, const float* __restrict__ x,
                                                           const float* __restrict__ w,
                                                           const float* __restrict__ bias, T* __restrict__ y) {
  __shared__ float ws[9][64];
  __shared__ float bs[64];
  for (int i = threadIdx.x; i < 576; i += 256) ws[i % 9][i / 9] = w[i];
  if (threadIdx.x < 64) bs[threadIdx.x] = bias[threadIdx.x];
  __syncthreads();
  const long P = (long)B * H * W;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < P * 16; idx += (long)gridDim.x * 256) {
    const long p = idx >> 4;
    const int c0 = (int)(idx & 15) * 4;
    const int wq = (int)(p % W), h = (int)((p / W) % H);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int hs = h + t / 3 - 1, wx = wq + t % 3 - 1;
      const float xv = (hs >= 0 && hs < H && wx >= 0 && wx < W) ? x[p + (long)(t / 3 - 1) * W + (t % 3 - 1)] : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaf(xv, ws[t][c0 + e], v[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] += bs[c0 + e];
      v[e] = v[e] > 0.f ? v[e] : 0.f;
    }
    vst4(y + p * 64 + c0, v);
  }
}

// part[block][c*9 + t] = sum_p dy[p][c] x_t(p), part[block][576 + c] = sum_p dy[p][c]
template <typename T>
__global__ __launch_bounds__(256) void vgg_conv1_wgrad_kernel(int B, int H, int W, const float* __restrict__ x,
                                                             const T* __restrict__ dy, float* __restrict__ part,
                                                             long p_per_block) {
  __shared__ float red[4][10][64];
  const int c = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long P = (long)B * H * W;
  const long p0 = blockIdx.x * p_per_block;
  long p1 = p0 + p_per_block;
  if (p1 > P) p1 = P;
  float s[10];
#pragma unroll
  for (int t = 0; t < 10; ++t) s[t] = 0.f;
  for (long p = p0 + wv; p < p1; p += 4) {
    const float d = to_f(dy[p * 64 + c]);
    const int wq = (int)(p % W), h = (int)((p / W) % H);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int hs = h + t / 3 - 1, wx = wq + t % 3 - 1;
      const float xv = (hs >= 0 && hs < H && wx >= 0 && wx < W) ? x[p + (long)(t / 3 - 1) * W + (t % 3 - 1)] : 0.f;
      s[t] = fmaf(d, xv, s[t]);
    }
    s[9] += d;
  }
#pragma unroll
  for (int t = 0; t < 10; ++t) red[wv][t][c] = s[t];
  __syncthreads();
  for (int i = threadIdx.x; i < 640; i += 256) {
    const int t = i < 576 ? i % 9 : 9, cc = i < 576 ? i / 9 : i - 576;
    part[(long)blockIdx.x * 640 + i] = (red[0][t][cc] + red[1][t][cc]) + (red[2][t][cc] + red[3][t][cc]);
  }
}

bool geo_ok(const VggGeo& g) {
  return g.B > 0 && g.H > 0 && g.W > 0 && (g.cin == 64 || g.cin == 128) && (g.cout == 64 || g.cout == 128);
}

VggGeo make_geo(const int* geo, const long* st) {
  VggGeo g{};
  if (!geo) return g;  // B = 0: refused by geo_ok
  g.B = geo[EA_VGG_B]; g.H = geo[EA_VGG_H]; g.W = geo[EA_VGG_W];
  g.cin = geo[EA_VGG_CIN]; g.cout = geo[EA_VGG_COUT];
  g.src = geo[EA_VGG_SRC]; g.epi = geo[EA_VGG_EPI]; g.flip = geo[EA_VGG_FLIP]; g.out_dtype = geo[EA_VGG_OUT_DTYPE];
  if (st) {
    g.ps_b = st[EA_VGG_PS_B]; g.ps_h = st[EA_VGG_PS_H]; g.ps_w = st[EA_VGG_PS_W]; g.ps_c = st[EA_VGG_PS_C];
    g.po_b = st[EA_VGG_PO_B]; g.po_h = st[EA_VGG_PO_H]; g.po_w = st[EA_VGG_PO_W]; g.po_c = st[EA_VGG_PO_C];
  }
  return g;
}

PooledSrc pooled_src(const VggGeo& g, const float* dp, const unsigned char* dec) {
  return PooledSrc{dp, dec, g.ps_b, g.ps_h, g.ps_w, g.ps_c};
}

// the weight gradient's pixel ranges: `cps` whole 32-pixel chunks each, at most 128 ranges
struct WgradRanges { int nsplit, cps; };
WgradRanges wgrad_ranges(const VggGeo& g) {
  const long chunks = ((long)g.B * g.H * g.W + KC - 1) / KC;
  const long cps = (chunks + 127) / 128;
  return WgradRanges{(int)((chunks + cps - 1) / cps), (int)cps};
}

}  // namespace

extern "C" {

int ea_vgg_conv3x3(const int* geo, const long* strides, int dtype, const void* x, const float* dp, const unsigned char* dec,
                   const void* w, const float* bias, const void* aux, void* out, unsigned char* dec_out,
                   void* stream) {
  EA_ENTRY();
  const VggGeo gg = make_geo(geo, strides);
  const VggGeo* g = &gg;
  EA_CHECK_ARG(geo_ok(gg) && strides && w && out);
  EA_CHECK_ARG(dtype == EA_F32 || dtype == EA_BF16);
  EA_CHECK_ARG(g->out_dtype == EA_F32 || g->out_dtype == EA_BF16);
  EA_CHECK_ARG(g->src == EA_VGG_SRC_POOLED ? (dp && dec) : (g->src == EA_VGG_SRC_PLAIN && x));
  EA_CHECK_ARG(g->epi >= EA_VGG_EPI_NONE && g->epi <= EA_VGG_EPI_POOL);
  EA_CHECK_ARG(g->epi != EA_VGG_EPI_MASK || aux);
  EA_CHECK_ARG(g->epi != EA_VGG_EPI_POOL || dec_out);
  const long Q = (long)g->B * ((g->H + 1) / 2) * ((g->W + 1) / 2);
  EA_CHECK_ARG((Q + 15) / 16 < (1L << 31));
  ConvArgs a{*g, x, pooled_src(gg, dp, dec), w, bias, aux, out, dec_out};
  const dim3 grid((unsigned)((Q + 15) / 16));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EA_F32) {
    if (g->cout == 64) vgg_conv_kernel<float, 64><<<grid, 256, 0, st>>>(a);
    else vgg_conv_kernel<float, 128><<<grid, 256, 0, st>>>(a);
  } else {
    if (g->cout == 64) vgg_conv_kernel<bf16, 64><<<grid, 256, 0, st>>>(a);
    else vgg_conv_kernel<bf16, 128><<<grid, 256, 0, st>>>(a);
  }
  EA_LAUNCH_CHECK();
  return 0;
}

int ea_vgg_wgrad_splits(const int* geo, int* nsplit) {
  const VggGeo gg = make_geo(geo, nullptr);
  EA_CHECK_ARG(geo_ok(gg) && nsplit);
  *nsplit = wgrad_ranges(gg).nsplit;
  return 0;
}

int ea_vgg_wgrad(const int* geo, const long* strides, int dtype, const void* x, const void* dy, const float* dp,
                 const unsigned char* dec, float* part, int nsplit, void* stream) {
  EA_ENTRY();
  const VggGeo gg = make_geo(geo, strides);
  const VggGeo* g = &gg;
  EA_CHECK_ARG(geo_ok(gg) && strides && x && part);
  EA_CHECK_ARG(dtype == EA_F32 || dtype == EA_BF16);
  EA_CHECK_ARG(g->src == EA_VGG_SRC_POOLED ? (dp && dec) : (g->src == EA_VGG_SRC_PLAIN && dy));
  const WgradRanges rg = wgrad_ranges(gg);
  EA_CHECK_ARG(nsplit == rg.nsplit);
  WgradArgs a{*g, x, dy, pooled_src(gg, dp, dec), part, rg.cps};
  const dim3 grid(nsplit, 9);
  hipStream_t st = (hipStream_t)stream;
  const int key = (dtype == EA_BF16) * 4 + (g->cout == 128) * 2 + (g->cin == 128);
  switch (key) {
    case 0: vgg_wgrad_kernel<float, 64, 64><<<grid, 256, 0, st>>>(a); break;
    case 2: vgg_wgrad_kernel<float, 128, 64><<<grid, 256, 0, st>>>(a); break;
    case 3: vgg_wgrad_kernel<float, 128, 128><<<grid, 256, 0, st>>>(a); break;
    case 4: vgg_wgrad_kernel<bf16, 64, 64><<<grid, 256, 0, st>>>(a); break;
    case 6: vgg_wgrad_kernel<bf16, 128, 64><<<grid, 256, 0, st>>>(a); break;
    case 7: vgg_wgrad_kernel<bf16, 128, 128><<<grid, 256, 0, st>>>(a); break;
    default: return EA_ERR_BAD_ARG;  // 128 -> 64 is no layer of VGG2L
  }
  EA_LAUNCH_CHECK();
  return 0;
}

int ea_vgg_pool_dbias(const int* geo, const long* strides, const float* dp, const unsigned char* dec, float* part, int nparts,
                      void* stream) {
  EA_ENTRY();
  const VggGeo gg = make_geo(geo, strides);
  const VggGeo* g = &gg;
  EA_CHECK_ARG(geo_ok(gg) && strides && dp && dec && part && nparts > 0 && nparts <= 65535);
  const int H2 = (g->H + 1) / 2, W2 = (g->W + 1) / 2;
  const long Q = (long)g->B * H2 * W2;
  vgg_pool_dbias_kernel<<<nparts, 256, 0, (hipStream_t)stream>>>(g->cout, Q, W2, H2, pooled_src(gg, dp, dec), part,
                                                                (Q + nparts - 1) / nparts);
  EA_LAUNCH_CHECK();
  return 0;
}

int ea_vgg_conv1_fwd(int B, int H, int W, const float* x, const float* w, const float* bias, void* y, int dtype,
                     void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(B > 0 && H > 0 && W > 0 && x && w && bias && y);
  EA_CHECK_ARG(dtype == EA_F32 || dtype == EA_BF16);
  const long P = (long)B * H * W;
  const int grid = ea_grid_cap((P * 16 + 255) / 256, 8192);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EA_F32) vgg_conv1_fwd_kernel<float><<<grid, 256, 0, st>>>(B, H, W, x, w, bias, (float*)y);
  else vgg_conv1_fwd_kernel<bf16><<<grid, 256, 0, st>>>(B, H, W, x, w, bias, (bf16*)y);
  EA_LAUNCH_CHECK();
  return 0;
}

int ea_vgg_conv1_wgrad(int B, int H, int W, const float* x, const void* dy, int dtype, float* part, int nparts,
                       void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(B > 0 && H > 0 && W > 0 && x && dy && part && nparts > 0);
  EA_CHECK_ARG(dtype == EA_F32 || dtype == EA_BF16);
  const long P = (long)B * H * W;
  const long ppb = (P + nparts - 1) / nparts;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EA_F32) vgg_conv1_wgrad_kernel<float><<<nparts, 256, 0, st>>>(B, H, W, x, (const float*)dy, part, ppb);
  else vgg_conv1_wgrad_kernel<bf16><<<nparts, 256, 0, st>>>(B, H, W, x, (const bf16*)dy, part, ppb);
  EA_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
