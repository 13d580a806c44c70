// Masked softmax + dropout of multi-head attention (transformer/attention.py:63-93), with
// the relative-position term of RelPositionMultiHeadedAttention (attention.py:262-305):
//   score[i,j] = (AC[i,j] + BD_raw[i, T1-1-i+j]) / sqrt(d_k)
// rel_shift (attention.py:237-260) is the index law above (bit-exact), so
// the shifted (T1,T1) matrix is never materialised: the softmax row kernel gathers the
// band, and the backward scatters dS straight into dBD_raw.
// Legacy variant (LegacyRelPositionMultiHeadedAttention, attention.py:114-206): its rel_shift
// pads one zero column on the left and reshapes, which is the same band column read from the
// query row below in the strict upper triangle, against an extended table Pext of 2*T1-1 rows
// (ea_legacy_pext: p, one zero row, p[0 .. T1-3]):
//   score[i,j] = (AC[i,j] + BD_raw[i + (j > i), T1-1-i+j]) / sqrt(d_k),  BD_raw[r,k] = (q_r+v)·Pext[k]
// Backward: band row r takes columns [T1-1-r, T1-1] from score row r and [T1+1, 2*T1-1-r] from
// score row r-1, disjoint ranges, so the wave of score row i writes columns [0, T1] of band row
// i and columns (T1, 2*T1-1) of band row i+1 (row 0's upper columns are written by row 0's wave).
// Masks: key j valid iff j < klen[b] (and j <= i when causal) — the padding mask of
// make_pad_mask + subsequent_mask; a fully-masked row gives P = 0 like the reference's
// masked_fill(min) -> softmax -> masked_fill(0).
#include "common.h"

namespace {

struct SmP {
  int B, H, T1, T2;
  float scale;
  const float* S; long ldS;        // [z][i][ldS], z = b*H + h
  const float* BD; long ldBD;      // [h][b][i][ldBD] or null
  const long long* klen;           // [B] or null
  int causal;
  float p; uint64_t seed; const unsigned long long* salt;
  float* P; long ldP;              // f32 softmax [z][i][ldP] (may alias S)
  void* Pd; int pd_dtype; long ldPd;  // dropout(P) in compute dtype
};

template <int MAXE, bool LEG>
__global__ __launch_bounds__(256) void softmax_fwd_kernel(SmP a) {
  const int lane = threadIdx.x & 63;
  const long rows = (long)a.B * a.H * a.T1;
  const long nw = (long)gridDim.x * 4;
  for (long r = blockIdx.x * 4L + (threadIdx.x >> 6); r < rows; r += nw) {
    const int i = (int)(r % a.T1);
    const long z = r / a.T1;
    const int b = (int)(z / a.H), h = (int)(z % a.H);
    const int kl = a.klen ? (int)min((long long)a.T2, a.klen[b]) : a.T2;
    const int lim = a.causal ? min(kl, i + 1) : kl;
    const float* srow = a.S + r * a.ldS;
    const float* brow = a.BD ? a.BD + (((long)h * a.B + b) * a.T1 + i) * a.ldBD + (a.T1 - 1 - i) : nullptr;
    float v[MAXE];
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < MAXE; ++e) {
      const int j = e * 64 + lane;
      float s = -INFINITY;
      if (j < lim) {
        s = srow[j];
        if (brow) s += LEG && j > i ? brow[a.ldBD + j] : brow[j];
        s *= a.scale;
      }
      v[e] = s;
      mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < MAXE; ++e) {
      const int j = e * 64 + lane;
      const float t = j < lim ? __expf(v[e] - mx) : 0.f;
      v[e] = t;
      sum += t;
    }
    sum = wave_sum(sum);
    const float inv = lim > 0 ? 1.f / sum : 0.f;
    float* prow = a.P + r * a.ldP;
    const uint64_t base = (uint64_t)r * a.T2;
    const uint64_t seed = ea_salted(a.seed, a.salt);
#pragma unroll
    for (int e = 0; e < MAXE; ++e) {
      const int j = e * 64 + lane;
      if (j < a.T2) {
        const float pj = v[e] * inv;
        prow[j] = pj;
        const float pd = a.p > 0.f ? pj * attn_drop_scale(seed, r, a.T2, j, a.p) : pj;
        store_from_f(a.Pd, r * a.ldPd + j, a.pd_dtype, pd);
      }
    }
  }
}

struct SmBP {
  int B, H, T1, T2;
  float scale;
  const float* dPd; long ldd;      // d(dropout(P)) [z][i][ldd] f32
  const float* P; long ldP;
  float p; uint64_t seed; const unsigned long long* salt;
  void* dS; int ds_dtype; long ldS;    // scale * dS [z][i][ldS]
  void* dBD; long ldBD; int nbd;       // [h][b][i][ldBD], rows of nbd = 2*T1-1 entries, or null
};

template <int MAXE, bool LEG>
__global__ __launch_bounds__(256) void softmax_bwd_kernel(SmBP a) {
  __shared__ float stash[4][64 * MAXE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long rows = (long)a.B * a.H * a.T1;
  const long nw = (long)gridDim.x * 4;
  for (long r = blockIdx.x * 4L + w; r < rows; r += nw) {
    const int i = (int)(r % a.T1);
    const long z = r / a.T1;
    const int b = (int)(z / a.H), h = (int)(z % a.H);
    const float* drow = a.dPd + r * a.ldd;
    const float* prow = a.P + r * a.ldP;
    const uint64_t base = (uint64_t)r * a.T2;
    const uint64_t seed = ea_salted(a.seed, a.salt);
    float pv[MAXE], dv[MAXE];
    float dot = 0.f;
#pragma unroll
    for (int e = 0; e < MAXE; ++e) {
      const int j = e * 64 + lane;
      if (j < a.T2) {
        pv[e] = prow[j];
        float d = drow[j];
        if (a.p > 0.f) d *= attn_drop_scale(seed, r, a.T2, j, a.p);
        dv[e] = d;
        dot += pv[e] * d;
      } else {
        pv[e] = dv[e] = 0.f;
      }
    }
    dot = wave_sum(dot);
#pragma unroll
    for (int e = 0; e < MAXE; ++e) {
      const int j = e * 64 + lane;
      if (j < a.T2) {
        const float g = pv[e] * (dv[e] - dot) * a.scale;
        store_from_f(a.dS, r * a.ldS + j, a.ds_dtype, g);
        stash[w][j] = g;
      }
    }
    if (a.dBD) {
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      const long orow = (((long)h * a.B + b) * a.T1 + i) * a.ldBD;
      const int off = a.T1 - 1 - i;
      if (LEG) {
        // this row's lower triangle (j <= i) and the forced zero of column T1 into band row i
        for (int q = lane; q <= a.T1 && q < a.nbd; q += 64) {
          const int j = q - off;
          const float g = (j >= 0 && q < a.T1) ? stash[w][j] : 0.f;
          store_from_f(a.dBD, orow + q, a.ds_dtype, g);
        }
        // its strict upper triangle beyond the zero (j >= i + 2) into band row i + 1
        if (i + 1 < a.T1) {
          for (int q = a.T1 + 1 + lane; q < a.nbd; q += 64) {
            const int j = q - off;
            const float g = j < a.T2 ? stash[w][j] : 0.f;
            store_from_f(a.dBD, orow + a.ldBD + q, a.ds_dtype, g);
          }
        }
        if (i == 0) {  // band row 0 has no score row above it
          for (int q = a.T1 + 1 + lane; q < a.nbd; q += 64) store_from_f(a.dBD, orow + q, a.ds_dtype, 0.f);
        }
      } else {
        for (int q = lane; q < a.nbd; q += 64) {
          const int j = q - off;
          const float g = (j >= 0 && j < a.T2) ? stash[w][j] : 0.f;
          store_from_f(a.dBD, orow + q, a.ds_dtype, g);
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// Pext of the legacy variant from p = linear_pos(pos_emb) (T rows): rows [0, T) = p, row T = 0,
// rows T+1+m = p[m] for m <= T-3 (2T-1 rows); and its adjoint dp[k] = dPext[k] + dPext[T+1+k].
template <typename T>
__global__ __launch_bounds__(256) void legacy_pext_kernel(int Tn, int d, const T* __restrict__ p, long ldp,
                                                          T* __restrict__ x, long ldx) {
  const long n = (2L * Tn - 1) * d;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += gridDim.x * 256L) {
    const int k = (int)(e / d), c = (int)(e % d);
    const int src = k < Tn ? k : k - Tn - 1;  // -1: the zero row
    x[k * ldx + c] = src >= 0 ? p[src * ldp + c] : (T)0.f;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void legacy_pext_fold_kernel(int Tn, int d, const T* __restrict__ dx, long ldx,
                                                               T* __restrict__ dp, long ldp) {
  const long n = (long)Tn * d;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += gridDim.x * 256L) {
    const int k = (int)(e / d), c = (int)(e % d);
    float g = to_f(dx[k * ldx + c]);
    if (k <= Tn - 3) g += to_f(dx[(Tn + 1 + k) * ldx + c]);
    dp[k * ldp + c] = (T)g;
  }
}

}  // namespace

#define EA_SM_DISPATCH(KER, LEG, T2, ARG)                                                     \
  do {                                                                                        \
    dim3 grid(ea_grid_cap(ea_cdiv((long)B * H * T1, 4), 4096)), blk(256);                     \
    hipStream_t st = (hipStream_t)stream;                                                     \
    if (T2 <= 64) hipLaunchKernelGGL((KER<1, LEG>), grid, blk, 0, st, ARG);                   \
    else if (T2 <= 128) hipLaunchKernelGGL((KER<2, LEG>), grid, blk, 0, st, ARG);             \
    else if (T2 <= 256) hipLaunchKernelGGL((KER<4, LEG>), grid, blk, 0, st, ARG);             \
    else if (T2 <= 512) hipLaunchKernelGGL((KER<8, LEG>), grid, blk, 0, st, ARG);             \
    else if (T2 <= 1024) hipLaunchKernelGGL((KER<16, LEG>), grid, blk, 0, st, ARG);           \
    else if (T2 <= 2048) hipLaunchKernelGGL((KER<32, LEG>), grid, blk, 0, st, ARG);           \
    else return EA_ERR_BAD_ARG;                                                               \
  } while (0)

extern "C" int ea_attn_softmax_fwd_mode(int B, int H, int T1, int T2, float scale, const float* S, long ldS,
                                        const float* BD, long ldBD, const long long* klen, int causal, float p,
                                        unsigned long long seed, float* P, long ldP, void* Pd, int pd_dtype,
                                        long ldPd, int rel_mode, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(rel_mode == EA_REL_LATEST || rel_mode == EA_REL_LEGACY);
  if (rel_mode == EA_REL_LEGACY) EA_CHECK_ARG(BD != nullptr && !causal);
  if ((long)B * H * T1 == 0) return 0;
  if (BD) EA_CHECK_ARG(T1 == T2);
  SmP a{B, H, T1, T2, scale, S, ldS, BD, ldBD, klen, causal, p, (uint64_t)seed, ea_g_rng_salt, P, ldP, Pd, pd_dtype, ldPd};
  if (rel_mode == EA_REL_LEGACY) EA_SM_DISPATCH(softmax_fwd_kernel, true, T2, a);
  else EA_SM_DISPATCH(softmax_fwd_kernel, false, T2, a);
  EA_LAUNCH_CHECK();
  return 0;
}

extern "C" int ea_attn_softmax_fwd(int B, int H, int T1, int T2, float scale, const float* S, long ldS,
                                   const float* BD, long ldBD, const long long* klen, int causal, float p,
                                   unsigned long long seed, float* P, long ldP, void* Pd, int pd_dtype,
                                   long ldPd, void* stream) {
  return ea_attn_softmax_fwd_mode(B, H, T1, T2, scale, S, ldS, BD, ldBD, klen, causal, p, seed, P, ldP, Pd, pd_dtype,
                                  ldPd, EA_REL_LATEST, stream);
}

extern "C" int ea_attn_softmax_bwd_mode(int B, int H, int T1, int T2, float scale, const float* dPd, long ldd,
                                        const float* P, long ldP, float p, unsigned long long seed, void* dS,
                                        int ds_dtype, long ldS, void* dBD, long ldBD, int rel_mode, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(rel_mode == EA_REL_LATEST || rel_mode == EA_REL_LEGACY);
  if (rel_mode == EA_REL_LEGACY) EA_CHECK_ARG(dBD != nullptr);
  if ((long)B * H * T1 == 0) return 0;
  if (dBD) EA_CHECK_ARG(T1 == T2);
  SmBP a{B, H, T1, T2, scale, dPd, ldd, P, ldP, p, (uint64_t)seed, ea_g_rng_salt, dS, ds_dtype, ldS, dBD, ldBD, 2 * T1 - 1};
  if (rel_mode == EA_REL_LEGACY) EA_SM_DISPATCH(softmax_bwd_kernel, true, T2, a);
  else EA_SM_DISPATCH(softmax_bwd_kernel, false, T2, a);
  EA_LAUNCH_CHECK();
  return 0;
}

extern "C" int ea_attn_softmax_bwd(int B, int H, int T1, int T2, float scale, const float* dPd, long ldd,
                                   const float* P, long ldP, float p, unsigned long long seed, void* dS,
                                   int ds_dtype, long ldS, void* dBD, long ldBD, void* stream) {
  return ea_attn_softmax_bwd_mode(B, H, T1, T2, scale, dPd, ldd, P, ldP, p, seed, dS, ds_dtype, ldS, dBD, ldBD,
                                  EA_REL_LATEST, stream);
}

extern "C" int ea_legacy_pext(int T, int d, const void* p, long ldp, void* pext, long ldx, int dtype, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(T >= 0 && d >= 0 && ldp >= d && ldx >= d && (dtype == EA_F32 || dtype == EA_BF16));
  if (T == 0 || d == 0) return 0;
  const dim3 grid(ea_grid_cap(ea_cdiv((2L * T - 1) * d, 256), 4096)), blk(256);
  if (dtype == EA_BF16)
    hipLaunchKernelGGL(legacy_pext_kernel<bf16>, grid, blk, 0, (hipStream_t)stream, T, d, (const bf16*)p, ldp,
                       (bf16*)pext, ldx);
  else
    hipLaunchKernelGGL(legacy_pext_kernel<float>, grid, blk, 0, (hipStream_t)stream, T, d, (const float*)p, ldp,
                       (float*)pext, ldx);
  EA_LAUNCH_CHECK();
  return 0;
}

extern "C" int ea_legacy_pext_fold(int T, int d, const void* dpext, long ldx, void* dp, long ldp, int dtype,
                                   void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(T >= 0 && d >= 0 && ldp >= d && ldx >= d && (dtype == EA_F32 || dtype == EA_BF16));
  if (T == 0 || d == 0) return 0;
  const dim3 grid(ea_grid_cap(ea_cdiv((long)T * d, 256), 4096)), blk(256);
  if (dtype == EA_BF16)
    hipLaunchKernelGGL(legacy_pext_fold_kernel<bf16>, grid, blk, 0, (hipStream_t)stream, T, d, (const bf16*)dpext,
                       ldx, (bf16*)dp, ldp);
  else
    hipLaunchKernelGGL(legacy_pext_fold_kernel<float>, grid, blk, 0, (hipStream_t)stream, T, d,
                       (const float*)dpext, ldx, (float*)dp, ldp);
  EA_LAUNCH_CHECK();
  return 0;
}
