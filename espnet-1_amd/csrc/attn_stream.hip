// Streaming (flash-style) forward attention in f32 on v_mfma_f32_16x16x4_f32, for the inference
// forward the unfused GEMM -> softmax -> GEMM path cannot serve: key rows longer than the 2048
// that ea_attn_softmax_fwd keeps in registers.  Nothing of size T1 x T2 is written.  DESIGN.md §20.
//
// Score law (attention.hip's header): the scale after the optional positional term,
//   s[i,j] = (q_i . k_j + BD[i + (legacy && j > i)][T1-1-i+j]) * scale,
// BD the raw band [h][b][i][ldBD] the band GEMM of the unfused path produces.  Key j is valid iff
// j < klen[b] (and j <= i when causal); a row with no valid key gives O = 0 and lse = -inf.
//
//   attn_stream_kernel<T, DKP>  a workgroup of 4 waves owns 64 query rows of one (b, h), a wave 16 of
//     them.  The wave's Q rows stay in registers as the A operand (DKP/4 values per lane).  Keys are
//     walked in tiles of 64: the K and V tiles are staged once per workgroup in LDS as f32 (bf16
//     operands are widened on the way in; rows past klen and columns past dk are zeros), rows DKP + 4
//     floats apart.  S = Q K^T of the wave's 16 x 64 tile is DKP/4 MFMA steps into four f32x4
//     accumulators: both operands take a float4 along the head dim and feed element e to step e, the
//     same permutation of k on either side.  The C layout leaves row 4*(lane>>4)+e of key column
//     lane&15 in register e, so a row's maximum is a 4-step shuffle over the 16 lanes of its group;
//     the running maximum and each lane's partial sum live in registers, and the DKP/16 f32x4 O
//     accumulators (the same row map) are rescaled when the maximum moves.  P goes through a per-wave
//     16 x 64 LDS patch into A-operand layout; P V reads V with the same k permutation (four scalar
//     reads a step, rows 4 apart per lane group: conflict-free with the DKP + 4 stride).
// No atomics: every output element has one owning lane and every sum a fixed order.
#include "common.h"

namespace {

constexpr int KT = 64;        // keys per tile
constexpr int LDP = KT + 4;   // row stride of a wave's P patch

struct StP {
  int B, H, T1, T2, dk;
  float scale;
  const void* q; long ldq;
  const void* k; long ldk;
  const void* v; long ldv;
  const float* BD; long ldBD;
  const long long* klen;
  int causal, legacy;
  float* O; long ldo;
  float* lse;
};

template <int DKP> constexpr long stream_lds_bytes() { return (2L * KT * (DKP + 4) + 4L * 16 * LDP) * 4; }

EA_DEV float group16_max(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
EA_DEV float group16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// 4 elements at column c (a multiple of 4) of a row, or zeros when `ok` is false
template <typename T>
EA_DEV f32x4 load4_or_zero(const T* row, int c, bool ok) {
  float t[4] = {0.f, 0.f, 0.f, 0.f};
  if (ok) vld4(row + c, t);
  return f32x4{t[0], t[1], t[2], t[3]};
}

template <typename T, int DKP>
__global__ __launch_bounds__(256) void attn_stream_kernel(StP a) {
  constexpr int LD = DKP + 4, NKB = DKP / 16, C4 = DKP / 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Ks = (float*)smem;             // (KT, LD)
  float* Vs = Ks + KT * LD;             // (KT, LD)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, qd = lane >> 4;
  float* Ps = Vs + KT * LD + w * 16 * LDP;  // this wave's (16, LDP) patch
  const int nqt = ea_cdiv(a.T1, 64);
  const int qt = (int)(blockIdx.x % nqt);
  const long z = blockIdx.x / nqt;
  const int b = (int)(z / a.H), h = (int)(z % a.H);
  const int T1 = a.T1, T2 = a.T2, dk = a.dk;
  long long kl64 = a.klen ? a.klen[b] : (long long)T2;
  const int kl = (int)(kl64 < 0 ? 0 : (kl64 > T2 ? T2 : kl64));
  const int kend = a.causal ? min(kl, min(T1, qt * 64 + 64)) : kl;  // keys any row of the block can see
  const int i0 = qt * 64 + w * 16;
  const bool live = i0 < T1;  // wave-uniform: the wave has at least one real query row

  const T* qp = (const T*)a.q + (long)b * T1 * a.ldq + (long)h * dk;
  const T* kp = (const T*)a.k + (long)b * T2 * a.ldk + (long)h * dk;
  const T* vp = (const T*)a.v + (long)b * T2 * a.ldv + (long)h * dk;

  // Q as the A operand: lane (r, qd) holds Q[i0 + r][16 kb + 4 qd + e]
  f32x4 qa[NKB];
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    const int c = 16 * kb + 4 * qd;
    qa[kb] = load4_or_zero(qp + (long)(i0 + r) * a.ldq, c, i0 + r < T1 && c < dk);
  }
  f32x4 o[NKB];
#pragma unroll
  for (int n = 0; n < NKB; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float mrow[4], lrow[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { mrow[e] = -INFINITY; lrow[e] = 0.f; }

  // band row bases of this lane's four query rows (i = i0 + 4 qd + e): BD[i][T1-1-i + j]
  const float* bdrow[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = i0 + 4 * qd + e;
    bdrow[e] = a.BD && i < T1 ? a.BD + (((long)h * a.B + b) * T1 + i) * a.ldBD + (T1 - 1 - i) : nullptr;
  }

  for (int j0 = 0; j0 < kend; j0 += KT) {
    __syncthreads();  // the previous tile has been read
#pragma unroll
    for (int t = 0; t < C4 * KT / 256; ++t) {
      const int idx = tid + t * 256;
      const int row = idx / C4, c = (idx % C4) * 4;
      const bool ok = j0 + row < kl && c < dk;
      *(f32x4*)(Ks + row * LD + c) = load4_or_zero(kp + (long)(j0 + row) * a.ldk, c, ok);
      *(f32x4*)(Vs + row * LD + c) = load4_or_zero(vp + (long)(j0 + row) * a.ldv, c, ok);
    }
    __syncthreads();
    if (!live) continue;

    // S = Q K^T: s[jt][e] = row i0 + 4 qd + e, key j0 + 16 jt + r
    f32x4 s[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) s[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const f32x4 kf = *(const f32x4*)(Ks + (jt * 16 + r) * LD + 16 * kb + 4 * qd);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[kb][e], kf[e], s[jt], 0, 0, 0);
      }

    // positional term, scale, masks; the tile's row maxima
    float tmax[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = i0 + 4 * qd + e;
      const int lim = a.causal ? min(kl, i + 1) : kl;
      float mx = -INFINITY;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const int j = j0 + jt * 16 + r;
        float x = -INFINITY;
        if (j < lim && i < T1) {
          x = s[jt][e];
          if (bdrow[e]) x += a.legacy && j > i ? bdrow[e][a.ldBD + j] : bdrow[e][j];
          x *= a.scale;
        }
        s[jt][e] = x;
        mx = fmaxf(mx, x);
      }
      tmax[e] = group16_max(mx);
    }
    // online softmax: rescale the running sum and O when the maximum moves, P into the patch
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float mnew = fmaxf(mrow[e], tmax[e]);
      const bool any = mnew > -INFINITY;  // some valid key so far
      const float alpha = any ? __expf(mrow[e] - mnew) : 1.f;
      mrow[e] = mnew;
      float ps = 0.f;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const float p = any ? __expf(s[jt][e] - mnew) : 0.f;
        ps += p;
        Ps[(4 * qd + e) * LDP + jt * 16 + r] = p;
      }
      lrow[e] = lrow[e] * alpha + ps;
#pragma unroll
      for (int n = 0; n < NKB; ++n) o[n][e] *= alpha;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // O += P V: A = P[r][16 kb + 4 qd + e], B = V[16 kb + 4 qd + e][16 n + r]
#pragma unroll
    for (int kb = 0; kb < KT / 16; ++kb) {
      const f32x4 pf = *(const f32x4*)(Ps + r * LDP + 16 * kb + 4 * qd);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float* vrow = Vs + (16 * kb + 4 * qd + e) * LD + r;
#pragma unroll
        for (int n = 0; n < NKB; ++n) o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(pf[e], vrow[16 * n], o[n], 0, 0, 0);
      }
    }
    __builtin_amdgcn_wave_barrier();  // the patch is read before the next tile rewrites it
  }

  if (!live) return;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = i0 + 4 * qd + e;
    const float l = group16_sum(lrow[e]);
    if (i >= T1) continue;
    const float inv = l > 0.f ? 1.f / l : 0.f;
    float* orow = a.O + ((long)b * T1 + i) * a.ldo + (long)h * dk;
#pragma unroll
    for (int n = 0; n < NKB; ++n)
      if (16 * n + r < dk) orow[16 * n + r] = o[n][e] * inv;
    if (a.lse && r == 0) a.lse[z * T1 + i] = l > 0.f ? mrow[e] + __logf(l) : -INFINITY;
  }
}

template <typename T, int DKP>
int launch_stream(const StP& a, hipStream_t st) {
  constexpr long bytes = stream_lds_bytes<DKP>();
  if (bytes > 65536) {  // every call: a host-side attribute of the current device's function, no stream work
    const hipError_t e = hipFuncSetAttribute((const void*)attn_stream_kernel<T, DKP>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
  }
  const long blocks = (long)a.B * a.H * ea_cdiv(a.T1, 64);
  if (blocks > 0x7fffffffL) return EA_ERR_BAD_ARG;
  hipLaunchKernelGGL((attn_stream_kernel<T, DKP>), dim3((unsigned)blocks), dim3(256), (size_t)bytes, st, a);
  EA_LAUNCH_CHECK();
  return 0;
}

template <typename T>
int launch_stream_dk(const StP& a, hipStream_t st) {
  if (a.dk <= 16) return launch_stream<T, 16>(a, st);
  if (a.dk <= 32) return launch_stream<T, 32>(a, st);
  if (a.dk <= 64) return launch_stream<T, 64>(a, st);
  return launch_stream<T, 128>(a, st);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int ea_attn_stream_fwd(int B, int H, int T1, int T2, int dk, const void* q, long ldq, const void* k,
                                  long ldk, const void* v, long ldv, int dtype, const float* BD, long ldBD,
                                  const long long* klen, int causal, float scale, float p, float* O, long ldo,
                                  float* lse, int rel_mode, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(p <= 0.f);  // no dropout: a forward for inference
  EA_CHECK_ARG(B >= 0 && H >= 0 && T1 >= 0 && T2 >= 1);
  EA_CHECK_ARG(dk >= 8 && dk <= 128 && dk % 8 == 0);
  EA_CHECK_ARG(dtype == EA_F32 || dtype == EA_BF16);
  EA_CHECK_ARG(rel_mode == EA_REL_LATEST || rel_mode == EA_REL_LEGACY);
  if (rel_mode == EA_REL_LEGACY) EA_CHECK_ARG(BD != nullptr && !causal);
  if (BD) EA_CHECK_ARG(T1 == T2 && ldBD >= 2L * T1 - 1);
  if ((long)B * H * T1 == 0) return 0;
  EA_CHECK_ARG(ldq >= dk && ldk >= dk && ldv >= dk && ldo >= dk && ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0);
  EA_CHECK_ARG(q && k && v && O && aligned16(q) && aligned16(k) && aligned16(v));
  const StP a{B, H, T1, T2, dk, scale, q, ldq, k, ldk, v, ldv, BD, ldBD, klen, causal, rel_mode == EA_REL_LEGACY,
              O, ldo, lse};
  return dtype == EA_BF16 ? launch_stream_dk<bf16>(a, (hipStream_t)stream)
                          : launch_stream_dk<float>(a, (hipStream_t)stream);
}
