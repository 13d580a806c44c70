// E-Branchformer block kernels (espnet2/asr/layers/cgmlp.py, e_branchformer_encoder.py:148-164):
// the convolutional spatial gating unit of the cgMLP and the depthwise merge convolution.
//
// Both are depthwise Conv1d(C, C, K, pad (K-1)/2, groups=C) passes over channel-last rows in
// the compute dtype (f32, or bf16 under AMP) and share one tiling, that of the Conformer's
// register-window depthwise kernels: a block is 64 channels x 64 frames, the frames plus their
// K-1 halo staged once in LDS as f32, each thread owning one channel and 16 consecutive frames
// with its taps in registers.  What differs is the tile loader and the store:
//   CSGU  : loader  LN(gelu(h[:, C + c]))   (exact erf GELU, LayerNorm over the C gate channels
//                   from the row statistics of ea_csgu_stats), store gelu(h[:, c]) * conv, dropout
//   merge : loader  xc                      store xc + conv
// The activated copy of h and the normalised gate are never stored: the backward recomputes them.
#include <math.h>

#include "common.h"

namespace {

constexpr int EB_CT = 64;  // channels per block
constexpr int EB_R = 16;   // frames per thread (64-frame tiles)

EA_DEV float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
// d gelu / dx = Phi(x) + x phi(x)
EA_DEV float gelu_grad(float x) {
  return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.39894228040143268f * __expf(-0.5f * x * x);
}

// dropout keep-scale of element idx under an already salted and folded stream key (the law of
// drop_scale in common.h, with the key hoisted out of the element loops)
EA_DEV float keep_scale(uint32_t key, uint32_t thr, float sc, uint64_t idx) {
  const uint32_t h = ea_pair_hash(key, idx >> 1);
  return ((idx & 1) ? h >> 16 : h & 0xffffu) >= thr ? sc : 0.f;
}

// ---------------------------------------------------------------- CSGU row statistics
// mean / rstd over the C = U/2 gate channels of gelu(h[row, C:]); one wave per row, two passes
// (the row is re-read from cache), f32 accumulation
template <typename T>
__global__ __launch_bounds__(256) void csgu_stats_kernel(int rows, int C, const T* __restrict__ h, long ldh, float eps,
                                                         float* __restrict__ mean, float* __restrict__ rstd) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const T* g = h + (long)row * ldh + C;
  float s = 0.f;
  for (int c = lane * 4; c < C; c += 256) {
    float v[4];
    vld4(g + c, v);
    s += (gelu_f(v[0]) + gelu_f(v[1])) + (gelu_f(v[2]) + gelu_f(v[3]));
  }
  const float mu = wave_sum(s) / (float)C;
  float q = 0.f;
  for (int c = lane * 4; c < C; c += 256) {
    float v[4];
    vld4(g + c, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = gelu_f(v[k]) - mu;
      q += d * d;
    }
  }
  const float var = wave_sum(q) / (float)C;
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = 1.f / sqrtf(var + eps);
  }
}

// ---------------------------------------------------------------- tiled depthwise passes
struct ConvArgs {
  int B, T, C;         // C: conv channels (CSGU: U/2, merge: 2d)
  const void* x;       // conv input rows, channel c at x[row * ldx + c] (CSGU: h + C, ldx = U)
  long ldx;
  const void* xr;      // CSGU: h (x_r = gelu(h[row * ldx + c]))
  const float *mean, *rstd, *gamma, *beta;  // CSGU: gate LayerNorm
  const float *w, *bias;                    // (C, K) taps, (C) bias
  float p;                                  // dropout (CSGU output; merge backward: the branch outputs')
  uint64_t seed, seed2;
  const unsigned long long* salt;
  // forward
  void* out;           // (rows, C) compute dtype
  // backward
  const void* dout;    // CSGU: (rows, C) grad of out; merge: dm (rows, C)
  void* dx;            // CSGU: dh (rows, 2C): the x_r half written here; merge: dxc (rows, C)
  float* dln;          // CSGU: (rows, C) f32 gradient of the normalised gate, for csgu_ln_bwd_kernel
  float* part;         // [block][NP * C] parameter-gradient partials
};

// one 4-channel group of the conv input at (row, c): f32 values the taps run over
template <typename T, bool CSGU>
EA_DEV void load_in4(const ConvArgs& a, long row, int c, const float (&gm)[4], const float (&bt)[4], float (&v)[4]) {
  vld4((const T*)a.x + row * a.ldx + c, v);
  if constexpr (CSGU) {
    const float mu = a.mean[row], rs = a.rstd[row];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (gelu_f(v[k]) - mu) * rs * gm[k] + bt[k];
  }
}

template <int K, typename T, bool CSGU>
__global__ __launch_bounds__(256) void gate_conv_fwd_kernel(ConvArgs a) {
  constexpr int R = EB_R, P = (K - 1) / 2, TT = 4 * R, RL = TT + K - 1, WIN = R + K - 1;
  __shared__ float tile[RL * EB_CT];
  __shared__ float wsm[K * EB_CT];  // [k][c]
  const int T_ = a.T, C = a.C;
  const int ntt = ea_cdiv(T_, TT);
  const int b = blockIdx.x / ntt, t0 = (blockIdx.x % ntt) * TT;
  const int c0 = blockIdx.y * EB_CT;
  const int cc = threadIdx.x % EB_CT, tq = threadIdx.x / EB_CT;
  const int c = c0 + cc;
  for (int i = threadIdx.x; i < EB_CT * K; i += 256) {  // w rows c0.. are one contiguous run
    const int ci = i / K, k = i - ci * K;
    wsm[k * EB_CT + ci] = c0 + ci < C ? a.w[(long)c0 * K + i] : 0.f;
  }
  {
    // 4-channel vector loads (C % 4 == 0): 16 lanes cover one 64-channel row
    const int c4 = (threadIdx.x % (EB_CT / 4)) * 4;
    const bool okc = c0 + c4 < C;
    float gm[4] = {0.f, 0.f, 0.f, 0.f}, bt[4] = {0.f, 0.f, 0.f, 0.f};
    if (CSGU && okc) {
      vld4(a.gamma + c0 + c4, gm);
      vld4(a.beta + c0 + c4, bt);
    }
    constexpr int NL = (RL * (EB_CT / 4) + 255) / 256;
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int i = threadIdx.x + 256 * u;
      const int rr = i / (EB_CT / 4);
      const int t = t0 + rr - P;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (rr < RL && okc && t >= 0 && t < T_) load_in4<T, CSGU>(a, (long)b * T_ + t, c0 + c4, gm, bt, v);
      if (rr < RL) *(float4*)(tile + rr * EB_CT + c4) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
  __syncthreads();
  if (c >= C) return;
  float win[WIN];
#pragma unroll
  for (int i = 0; i < WIN; ++i) win[i] = tile[(tq * R + i) * EB_CT + cc];
  float acc[R];
  const float b0 = a.bias[c];
#pragma unroll
  for (int j = 0; j < R; ++j) acc[j] = b0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float wk = wsm[k * EB_CT + cc];
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] += wk * win[j + k];
  }
  T* out = (T*)a.out;
  if constexpr (CSGU) {
    const bool drop = a.p > 0.f;
    const uint32_t key = drop ? ea_seed_key(ea_salted(a.seed, a.salt)) : 0u, thr = ea_drop_thr(a.p);
    const float sc = drop ? 1.f / (1.f - a.p) : 1.f;
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int t = t0 + tq * R + j;
      if (t < T_) {
        const long row = (long)b * T_ + t;
        float v = gelu_f(to_f(((const T*)a.xr)[row * a.ldx + c])) * acc[j];
        if (drop) v *= keep_scale(key, thr, sc, (uint64_t)row * C + c);
        out[row * C + c] = from_f<T>(v);
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int t = t0 + tq * R + j;
      if (t < T_) out[((long)b * T_ + t) * C + c] = from_f<T>(acc[j] + win[j + P]);
    }
  }
}

// Backward of the pass above.  dconv = grad of the conv output (CSGU: dout * mask * gelu(x_r),
// built in the tile loader; merge: dm).  din[t] = sum_k w[k] dconv[t-k+P] is the gradient of the
// conv input: CSGU writes it (f32) for the LayerNorm backward and also writes the x_r half
// dh[:, c] = dout * mask * conv * gelu'(h) from the recomputed conv output; merge writes
// dxc = dm + din (times the two branch outputs' dropout masks, one stream per half of the
// channels, when p > 0).  Partials per block, NP = K + 1 (+ 2 for CSGU) entries per channel:
// part[blk][k*C + c] = sum_t dconv[t] in[t+k-P], [K*C + c] = sum_t dconv[t] (dbias), CSGU:
// [(K+1)*C + c] = sum_t din[t] n[t] (LayerNorm dgamma, n the normalised gate), [(K+2)*C + c] =
// sum_t din[t] (dbeta).
template <int K, typename T, bool CSGU>
__global__ __launch_bounds__(256) void gate_conv_bwd_kernel(ConvArgs a) {
  constexpr int R = EB_R, P = (K - 1) / 2, TT = 4 * R, RL = TT + K - 1, WIN = R + K - 1;
  constexpr int NP = CSGU ? K + 3 : K + 1;
  constexpr int SM = 2 * RL * EB_CT > 4 * NP * EB_CT ? 2 * RL * EB_CT : 4 * NP * EB_CT;
  __shared__ float sm[SM];
  float* tdy = sm;                // dconv rows t0-P .. t0+TT-1+P
  float* tx = sm + RL * EB_CT;    // conv input rows, the same range
  const int T_ = a.T, C = a.C;
  const int ntt = ea_cdiv(T_, TT);
  const int b = blockIdx.x / ntt, t0 = (blockIdx.x % ntt) * TT;
  const int c0 = blockIdx.y * EB_CT;
  const int cc = threadIdx.x % EB_CT, tq = threadIdx.x / EB_CT;
  const int c = c0 + cc;
  const bool drop = a.p > 0.f;
  const uint32_t thr = ea_drop_thr(a.p);
  const float sc = drop ? 1.f / (1.f - a.p) : 1.f;
  const uint32_t key = drop ? ea_seed_key(ea_salted(a.seed, a.salt)) : 0u;
  float wr[K];
#pragma unroll
  for (int k = 0; k < K; ++k) wr[k] = c < C ? a.w[(long)c * K + k] : 0.f;
  {
    const int c4 = (threadIdx.x % (EB_CT / 4)) * 4;
    const bool okc = c0 + c4 < C;
    float gm[4] = {0.f, 0.f, 0.f, 0.f}, bt[4] = {0.f, 0.f, 0.f, 0.f};
    if (CSGU && okc) {
      vld4(a.gamma + c0 + c4, gm);
      vld4(a.beta + c0 + c4, bt);
    }
    constexpr int NL = (RL * (EB_CT / 4) + 255) / 256;
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int i = threadIdx.x + 256 * u;
      const int rr = i / (EB_CT / 4);
      const int t = t0 + rr - P;
      float vd[4] = {0.f, 0.f, 0.f, 0.f}, vx[4] = {0.f, 0.f, 0.f, 0.f};
      if (rr < RL && okc && t >= 0 && t < T_) {
        const long row = (long)b * T_ + t;
        vld4((const T*)a.dout + row * C + c0 + c4, vd);
        if constexpr (CSGU) {
          float hr[4];
          vld4((const T*)a.xr + row * a.ldx + c0 + c4, hr);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            vd[k] *= gelu_f(hr[k]);
            if (drop) vd[k] *= keep_scale(key, thr, sc, (uint64_t)row * C + c0 + c4 + k);
          }
        }
        load_in4<T, CSGU>(a, row, c0 + c4, gm, bt, vx);
      }
      if (rr < RL) {
        *(float4*)(tdy + rr * EB_CT + c4) = make_float4(vd[0], vd[1], vd[2], vd[3]);
        *(float4*)(tx + rr * EB_CT + c4) = make_float4(vx[0], vx[1], vx[2], vx[3]);
      }
    }
  }
  __syncthreads();
  float aw[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) aw[k] = 0.f;
  {
    float win[WIN], xw[WIN];
#pragma unroll
    for (int i = 0; i < WIN; ++i) {
      win[i] = tdy[(tq * R + i) * EB_CT + cc];
      xw[i] = tx[(tq * R + i) * EB_CT + cc];
    }
    float din[R];
#pragma unroll
    for (int j = 0; j < R; ++j) din[j] = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float wk = wr[k];
#pragma unroll
      for (int j = 0; j < R; ++j) din[j] += wk * win[j - k + K - 1];
    }
    if (c < C) {
      if constexpr (CSGU) {
        const float b0 = a.bias[c];
#pragma unroll
        for (int j = 0; j < R; ++j) {
          const int t = t0 + tq * R + j;
          if (t < T_) {
            const long row = (long)b * T_ + t;
            float conv = b0;
#pragma unroll
            for (int k = 0; k < K; ++k) conv += wr[k] * xw[j + k];
            float e = to_f(((const T*)a.dout)[row * C + c]);
            if (drop) e *= keep_scale(key, thr, sc, (uint64_t)row * C + c);
            const float hr = to_f(((const T*)a.xr)[row * a.ldx + c]);
            ((T*)a.dx)[row * a.ldx + c] = from_f<T>(e * conv * gelu_grad(hr));
            a.dln[row * C + c] = din[j];
            const float hg = to_f(((const T*)a.x)[row * a.ldx + c]);
            const float n = (gelu_f(hg) - a.mean[row]) * a.rstd[row];
            aw[K + 1] += din[j] * n;
            aw[K + 2] += din[j];
          }
        }
      } else {
        const int dh = C >> 1;
        const bool second = c >= dh;
        const uint32_t key2 = drop && second ? ea_seed_key(ea_salted(a.seed2, a.salt)) : key;
#pragma unroll
        for (int j = 0; j < R; ++j) {
          const int t = t0 + tq * R + j;
          if (t < T_) {
            const long row = (long)b * T_ + t;
            float v = win[j + P] + din[j];
            if (drop) v *= keep_scale(key2, thr, sc, (uint64_t)row * dh + (second ? c - dh : c));
            ((T*)a.dx)[row * C + c] = from_f<T>(v);
          }
        }
      }
    }
    // dconv[t0 + tq*R + j] = win[j + P] (rows outside the utterance are zero)
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const float d = win[j + P];
      aw[K] += d;
#pragma unroll
      for (int k = 0; k < K; ++k) aw[k] += d * xw[j + k];
    }
  }
  __syncthreads();  // the tiles become the 4-group reduction buffer
#pragma unroll
  for (int k = 0; k < NP; ++k) sm[(tq * NP + k) * EB_CT + cc] = aw[k];
  __syncthreads();
  const long blk = (long)blockIdx.x;
  for (int i = threadIdx.x; i < NP * EB_CT; i += 256) {
    const int k = i / EB_CT, ci = i % EB_CT;
    const int cg = c0 + ci;
    if (cg >= C) continue;
    const float v = (sm[(0 * NP + k) * EB_CT + ci] + sm[(1 * NP + k) * EB_CT + ci]) +
                    (sm[(2 * NP + k) * EB_CT + ci] + sm[(3 * NP + k) * EB_CT + ci]);
    a.part[blk * (long)C * NP + (long)k * C + cg] = v;
  }
}

// LayerNorm backward over the C gate channels and the GELU backward of the gate half:
// dn = dln * gamma, dg = rstd * (dn - mean_c(dn) - n * mean_c(dn * n)), dh[:, C + c] = dg * gelu'(h).
// One wave per row, two passes over the row (n recomputed from h).
template <typename T>
__global__ __launch_bounds__(256) void csgu_ln_bwd_kernel(int rows, int C, const float* __restrict__ dln,
                                                          const T* __restrict__ h, long ldh,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          const float* __restrict__ gamma, T* __restrict__ dh) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const T* g = h + (long)row * ldh + C;
  const float* dl = dln + (long)row * C;
  const float mu = mean[row], rs = rstd[row];
  float s1 = 0.f, s2 = 0.f;
  for (int c = lane * 4; c < C; c += 256) {
    float v[4], d[4], gm[4];
    vld4(g + c, v);
    vld4(dl + c, d);
    vld4(gamma + c, gm);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float dn = d[k] * gm[k];
      s1 += dn;
      s2 += dn * (gelu_f(v[k]) - mu) * rs;
    }
  }
  s1 = wave_sum(s1) / (float)C;
  s2 = wave_sum(s2) / (float)C;
  T* o = dh + (long)row * ldh + C;
  for (int c = lane * 4; c < C; c += 256) {
    float v[4], d[4], gm[4], r[4];
    vld4(g + c, v);
    vld4(dl + c, d);
    vld4(gamma + c, gm);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float n = (gelu_f(v[k]) - mu) * rs;
      r[k] = rs * (d[k] * gm[k] - s1 - n * s2) * gelu_grad(v[k]);
    }
    vst4(o + c, r);
  }
}

bool ok_k(int K) { return K == 3 || K == 5 || K == 7 || K == 15 || K == 31; }
bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

template <typename T, bool CSGU>
void launch_fwd(int K, dim3 grid, hipStream_t st, const ConvArgs& a) {
  switch (K) {
#define EA_EBF(KK) case KK: hipLaunchKernelGGL((gate_conv_fwd_kernel<KK, T, CSGU>), grid, dim3(256), 0, st, a); break;
    EA_EBF(3) EA_EBF(5) EA_EBF(7) EA_EBF(15) EA_EBF(31)
#undef EA_EBF
  }
}
template <typename T, bool CSGU>
void launch_bwd(int K, dim3 grid, hipStream_t st, const ConvArgs& a) {
  switch (K) {
#define EA_EBB(KK) case KK: hipLaunchKernelGGL((gate_conv_bwd_kernel<KK, T, CSGU>), grid, dim3(256), 0, st, a); break;
    EA_EBB(3) EA_EBB(5) EA_EBB(7) EA_EBB(15) EA_EBB(31)
#undef EA_EBB
  }
}

}  // namespace

extern "C" int ea_csgu_stats(int rows, int U, const void* h, int dtype, float eps, float* mean, float* rstd,
                             void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(rows >= 0 && U > 0 && U % 8 == 0 && h && mean && rstd && al16(h));
  EA_CHECK_ARG(dtype == EA_F32 || dtype == EA_BF16);
  if (rows == 0) return 0;
  const dim3 grid(ea_cdiv(rows, 4));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EA_BF16)
    hipLaunchKernelGGL(csgu_stats_kernel<bf16>, grid, dim3(256), 0, st, rows, U / 2, (const bf16*)h, (long)U, eps, mean, rstd);
  else
    hipLaunchKernelGGL(csgu_stats_kernel<float>, grid, dim3(256), 0, st, rows, U / 2, (const float*)h, (long)U, eps, mean, rstd);
  EA_LAUNCH_CHECK();
  return 0;
}

extern "C" int ea_csgu_fwd(int B, int T, int U, int K, const void* h, int dtype, const float* mean, const float* rstd,
                           const float* gamma, const float* beta, const float* w, const float* bias, float p,
                           unsigned long long seed, void* out, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(B > 0 && T > 0 && U > 0 && U % 8 == 0 && ok_k(K) && (dtype == EA_F32 || dtype == EA_BF16));
  EA_CHECK_ARG(h && mean && rstd && gamma && beta && w && bias && out && al16(h) && al16(gamma) && al16(beta));
  EA_CHECK_ARG(p >= 0.f && p < 1.f);
  const int C = U / 2;
  const size_t es = dtype == EA_BF16 ? 2 : 4;
  ConvArgs a{};
  a.B = B; a.T = T; a.C = C;
  a.x = (const char*)h + (size_t)C * es; a.ldx = U; a.xr = h;
  a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta; a.w = w; a.bias = bias;
  a.p = p; a.seed = seed; a.salt = ea_g_rng_salt; a.out = out;
  const dim3 grid(B * ea_cdiv(T, 4 * EB_R), ea_cdiv(C, EB_CT));
  if (dtype == EA_BF16) launch_fwd<bf16, true>(K, grid, (hipStream_t)stream, a);
  else launch_fwd<float, true>(K, grid, (hipStream_t)stream, a);
  EA_LAUNCH_CHECK();
  return 0;
}

extern "C" int ea_csgu_bwd_ws_elems(int B, int T, int U, int K, long* dln_elems, long* ws_elems) {
  EA_ENTRY();
  EA_CHECK_ARG(B > 0 && T > 0 && U > 0 && U % 8 == 0 && ok_k(K) && dln_elems && ws_elems);
  *dln_elems = (long)B * T * (U / 2);
  *ws_elems = (long)B * ea_cdiv(T, 4 * EB_R) * (U / 2) * (K + 3);
  return 0;
}

extern "C" int ea_csgu_bwd(int B, int T, int U, int K, const void* dout, const void* h, int dtype, const float* mean,
                           const float* rstd, const float* gamma, const float* beta, const float* w,
                           const float* bias, float p, unsigned long long seed, void* dh, float* dgamma, float* dbeta,
                           float* dw, float* dbias, int accumulate_params, float* dln, float* workspace, long ws_elems,
                           void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(B > 0 && T > 0 && U > 0 && U % 8 == 0 && ok_k(K) && (dtype == EA_F32 || dtype == EA_BF16));
  EA_CHECK_ARG(dout && h && mean && rstd && gamma && beta && w && bias && dh && dgamma && dbeta && dw && dbias && dln &&
               workspace);
  EA_CHECK_ARG(al16(dout) && al16(h) && al16(dh) && al16(gamma) && al16(beta) && al16(dln) && p >= 0.f && p < 1.f);
  const int C = U / 2;
  const int nblk = B * ea_cdiv(T, 4 * EB_R);
  const long rowlen = (long)C * (K + 3);
  EA_CHECK_ARG((long)nblk * rowlen <= ws_elems);
  const size_t es = dtype == EA_BF16 ? 2 : 4;
  ConvArgs a{};
  a.B = B; a.T = T; a.C = C;
  a.x = (const char*)h + (size_t)C * es; a.ldx = U; a.xr = h;
  a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta; a.w = w; a.bias = bias;
  a.p = p; a.seed = seed; a.salt = ea_g_rng_salt;
  a.dout = dout; a.dx = dh; a.dln = dln; a.part = workspace;
  const dim3 grid(nblk, ea_cdiv(C, EB_CT));
  hipStream_t st = (hipStream_t)stream;
  const long rows = (long)B * T;
  if (dtype == EA_BF16) {
    launch_bwd<bf16, true>(K, grid, st, a);
    EA_LAUNCH_CHECK();
    hipLaunchKernelGGL(csgu_ln_bwd_kernel<bf16>, dim3(ea_cdiv(rows, 4)), dim3(256), 0, st, (int)rows, C, dln,
                       (const bf16*)h, (long)U, mean, rstd, gamma, (bf16*)dh);
  } else {
    launch_bwd<float, true>(K, grid, st, a);
    EA_LAUNCH_CHECK();
    hipLaunchKernelGGL(csgu_ln_bwd_kernel<float>, dim3(ea_cdiv(rows, 4)), dim3(256), 0, st, (int)rows, C, dln,
                       (const float*)h, (long)U, mean, rstd, gamma, (float*)dh);
  }
  EA_LAUNCH_CHECK();
  // fixed-order reductions of the per-block partials: [k][c] taps written as dw (C, 1, K), then
  // dbias, LayerNorm dgamma, dbeta (adjacent parameter gradients share a launch)
  int rc;
  if (dbias == dw + (long)C * K) {
    rc = ea_reduce_partials_tr(nblk, C * (K + 1), workspace, rowlen, dw, accumulate_params, C, K, stream);
  } else {
    rc = ea_reduce_partials_tr(nblk, C * K, workspace, rowlen, dw, accumulate_params, C, K, stream);
    if (rc) return rc;
    rc = ea_reduce_partials(nblk, C, workspace + (long)C * K, rowlen, dbias, accumulate_params, stream);
  }
  if (rc) return rc;
  if (dbeta == dgamma + C)
    return ea_reduce_partials(nblk, 2 * C, workspace + (long)C * (K + 1), rowlen, dgamma, accumulate_params, stream);
  rc = ea_reduce_partials(nblk, C, workspace + (long)C * (K + 1), rowlen, dgamma, accumulate_params, stream);
  if (rc) return rc;
  return ea_reduce_partials(nblk, C, workspace + (long)C * (K + 2), rowlen, dbeta, accumulate_params, stream);
}

extern "C" int ea_merge_conv_fwd(int B, int T, int C, int K, const void* xc, int dtype, const float* w,
                                 const float* bias, void* m, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(B > 0 && T > 0 && C > 0 && C % 4 == 0 && ok_k(K) && (dtype == EA_F32 || dtype == EA_BF16));
  EA_CHECK_ARG(xc && w && bias && m && al16(xc));
  ConvArgs a{};
  a.B = B; a.T = T; a.C = C;
  a.x = xc; a.ldx = C; a.w = w; a.bias = bias; a.out = m;
  const dim3 grid(B * ea_cdiv(T, 4 * EB_R), ea_cdiv(C, EB_CT));
  if (dtype == EA_BF16) launch_fwd<bf16, false>(K, grid, (hipStream_t)stream, a);
  else launch_fwd<float, false>(K, grid, (hipStream_t)stream, a);
  EA_LAUNCH_CHECK();
  return 0;
}

extern "C" int ea_merge_conv_bwd_ws_elems(int B, int T, int C, int K, long* ws_elems) {
  EA_ENTRY();
  EA_CHECK_ARG(B > 0 && T > 0 && C > 0 && ok_k(K) && ws_elems);
  *ws_elems = (long)B * ea_cdiv(T, 4 * EB_R) * C * (K + 1);
  return 0;
}

extern "C" int ea_merge_conv_bwd(int B, int T, int C, int K, const void* xc, const void* dm, int dtype, const float* w,
                                 float p, unsigned long long seed_a, unsigned long long seed_b, void* dxc, float* dw,
                                 float* dbias, int accumulate_params, float* workspace, long ws_elems, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(B > 0 && T > 0 && C > 0 && C % 4 == 0 && ok_k(K) && (dtype == EA_F32 || dtype == EA_BF16));
  EA_CHECK_ARG(xc && dm && w && dxc && dw && dbias && workspace && al16(xc) && al16(dm) && p >= 0.f && p < 1.f);
  const int nblk = B * ea_cdiv(T, 4 * EB_R);
  const long rowlen = (long)C * (K + 1);
  EA_CHECK_ARG((long)nblk * rowlen <= ws_elems);
  ConvArgs a{};
  a.B = B; a.T = T; a.C = C;
  a.x = xc; a.ldx = C; a.w = w;
  a.p = p; a.seed = seed_a; a.seed2 = seed_b; a.salt = ea_g_rng_salt;
  a.dout = dm; a.dx = dxc; a.part = workspace;
  const dim3 grid(nblk, ea_cdiv(C, EB_CT));
  if (dtype == EA_BF16) launch_bwd<bf16, false>(K, grid, (hipStream_t)stream, a);
  else launch_bwd<float, false>(K, grid, (hipStream_t)stream, a);
  EA_LAUNCH_CHECK();
  if (dbias == dw + (long)C * K)
    return ea_reduce_partials_tr(nblk, C * (K + 1), workspace, rowlen, dw, accumulate_params, C, K, stream);
  int rc = ea_reduce_partials_tr(nblk, C * K, workspace, rowlen, dw, accumulate_params, C, K, stream);
  if (rc) return rc;
  return ea_reduce_partials(nblk, C, workspace + (long)C * K, rowlen, dbias, accumulate_params, stream);
}
