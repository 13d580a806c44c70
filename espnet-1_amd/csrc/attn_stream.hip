// Streaming (flash-style) forward attention in f32 on v_mfma_f32_16x16x4_f32, for the inference
// forward the unfused GEMM -> softmax -> GEMM path cannot serve: key rows longer than the 2048
// that ea_attn_softmax_fwd keeps in registers.  Nothing of size T1 x T2 is written.  DESIGN.md §20.
// With dropout (DROP) it is the training forward, and its backward follows below.
//
// Score law (attention.hip's header): the scale after the optional positional term,
//   s[i,j] = (q_i . k_j + BD[i + (legacy && j > i)][T1-1-i+j]) * scale,
// BD the raw band [h][b][i][ldBD] the band GEMM of the unfused path produces.  Key j is valid iff
// j < klen[b] (and j <= i when causal); a row with no valid key gives O = 0 and lse = -inf.
//
//   attn_stream_kernel<T, DKP, DROP>  a workgroup of 4 waves owns 64 query rows of one (b, h), a wave 16 of
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
  float p; uint64_t seed; const unsigned long long* salt;  // DROP instantiations only
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

// DROP: the training forward.  The keep decision of common.h's attn_keep (row z*T1 + i, the law of the
// unfused softmax and the fused kernels) scales the probabilities that enter P V by 1/(1-p) or 0; the
// row sum, and so lse, stays that of the undropped scores.
template <typename T, int DKP, bool DROP>
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

  const uint32_t key = DROP ? ea_seed_key(ea_salted(a.seed, a.salt)) : 0u, thr = DROP ? ea_drop_thr(a.p) : 0u;
  const float keep = DROP ? 1.f / (1.f - a.p) : 1.f;

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
        if (DROP)
          Ps[(4 * qd + e) * LDP + jt * 16 + r] =
              attn_keep(key, thr, (uint64_t)z * T1 + (i0 + 4 * qd + e), T2, j0 + jt * 16 + r) ? p * keep : 0.f;
        else
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

template <typename T, int DKP, bool DROP>
int launch_stream(const StP& a, hipStream_t st) {
  constexpr long bytes = stream_lds_bytes<DKP>();
  if (bytes > 65536) {  // every call: a host-side attribute of the current device's function, no stream work
    const hipError_t e = hipFuncSetAttribute((const void*)attn_stream_kernel<T, DKP, DROP>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
  }
  const long blocks = (long)a.B * a.H * ea_cdiv(a.T1, 64);
  if (blocks > 0x7fffffffL) return EA_ERR_BAD_ARG;
  hipLaunchKernelGGL((attn_stream_kernel<T, DKP, DROP>), dim3((unsigned)blocks), dim3(256), (size_t)bytes, st, a);
  EA_LAUNCH_CHECK();
  return 0;
}

template <typename T, bool DROP>
int launch_stream_dk(const StP& a, hipStream_t st) {
  if (a.dk <= 16) return launch_stream<T, 16, DROP>(a, st);
  if (a.dk <= 32) return launch_stream<T, 32, DROP>(a, st);
  if (a.dk <= 64) return launch_stream<T, 64, DROP>(a, st);
  return launch_stream<T, 128, DROP>(a, st);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int stream_fwd(int B, int H, int T1, int T2, int dk, const void* q, long ldq, const void* k, long ldk, const void* v,
               long ldv, int dtype, const float* BD, long ldBD, const long long* klen, int causal, float scale,
               float p, unsigned long long seed, float* O, long ldo, float* lse, int rel_mode, void* stream) {
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
              O, ldo, lse, p, (uint64_t)seed, ea_g_rng_salt};
  hipStream_t st = (hipStream_t)stream;
  if (p > 0.f) return dtype == EA_BF16 ? launch_stream_dk<bf16, true>(a, st) : launch_stream_dk<float, true>(a, st);
  return dtype == EA_BF16 ? launch_stream_dk<bf16, false>(a, st) : launch_stream_dk<float, false>(a, st);
}

// ------------------------------------------------------------------------------------------ backward
// Three sweeps of one kernel template, each recomputing the scores from q, k and the forward's lse.
// A workgroup of 4 waves owns 64 rows of one (b, h) on the OWNER
// axis, a wave 16 of them, and walks the other axis in tiles of 64 staged in LDS as f32:
//   MODE 2, the row-sum sweep, runs first: the query-owner tiles below without the dQ product, summing
//     D_i = sum_j (m/(1-p) P_ij) dP_ij over the key tiles in registers (= dO_i . O_i; taken from the same
//     MFMA values the passes recompute, so P (dP - D) of a row with one valid key is an exact zero as it is
//     on the unfused path, and D does not see O's rounding to bf16).  The same sweep sums C_i = sum_j
//     exp(s_ij - lse_i), 1 but for the rounding of lse to f32 and of exp, and stores it beside the sum
//     (D unnormalised): the passes take P = exp(s - lse) / C, normalised by the sum of its own terms as
//     the unfused softmax is, and dS = scale / C (exp(s - lse) m dP - P D).
//   MODE 0, the query-owner pass: owner rows are queries (Q and dO rows in registers as A operands),
//     walked tiles are K and V.  S = Q K^T and dP = dO V^T come out in the C layout [query][key]; dS goes
//     through the wave's 16 x 64 patch into A-operand layout and dQ += dS K reads the staged K tile as
//     the forward reads V.  The dS registers are also the band gradient: lane (r, qd) stores element
//     (i, j) at dbd[i + (legacy && j > i)][T1-1-i+j], 16 consecutive columns per lane group, and after
//     the loop the wave zero-fills the band positions of its rows no (i, j) of the loop landed on.
//   MODE 1 (KO), the key-owner pass: owner rows are keys (K and V rows in registers as A operands), walked
//     tiles are Q and dO (with the lse and D of those 64 queries beside them).  The transposed tiles
//     S^T = K Q^T and dP^T = V dO^T are computed directly, the operand roles swapped, so they come out in
//     the C layout [key][query] and P^T / dS^T need no transpose of their own: each goes through the same
//     per-wave patch (one after the other) into A-operand layout, and dV += P^T dO, dK += dS^T Q read the
//     staged dO and Q tiles as B operands, row = the reduction index (the query), as P V reads V.
// Every output element has one owning lane (dbd: one source (i, j) per band position, attention.hip's
// header), every sum a fixed order; keys past klen, rows with lse = -inf and band positions without a
// source are exact zeros, and no operand element outside the valid rows / first dk columns is read.
// LDS per workgroup = two (64, DKP + 4) f32 tiles + four (16, 68) patches (+ 1 KiB of lse / D / C / 1/C):
// DKP 16: 28,672 B; 32: 36,864 B; 64: 53,248 B; 128: 86,016 B of the CU's 160 KiB (5 / 4 / 3 / 1 workgroups).
// Splitting the backward into passes is what keeps DKP = 128 at 64-row tiles on both axes: one
// pass never holds more than two tiles.
struct StB {
  int B, H, T1, T2, dk;
  float scale;
  const void* q; long ldq;
  const void* k; long ldk;
  const void* v; long ldv;
  const float* BD; long ldBD;
  const long long* klen;
  int causal, legacy;
  float p; uint64_t seed; const unsigned long long* salt;
  const float* lse;
  const void* dO; long lddo;
  float* D;  // the row-sum sweep's output: sum_j e m dP [z][i], then C = sum_j e [z][i]
  void* dq; long lddq;
  void* dk_; long lddk;
  void* dv; long lddv;
  void* dbd; long lddbd;
};

template <int DKP> constexpr long stream_bwd_lds_bytes() { return stream_lds_bytes<DKP>() + 4L * KT * 4; }

// acc[n] += patch (16 x 64, A-operand layout) . Ys (64 x DKP tile): the forward's P V step
template <int NKB, int LD>
EA_DEV void patch_mma(const float* Ps, const float* Ys, int r, int qd, f32x4 (&acc)[NKB]) {
#pragma unroll
  for (int kb = 0; kb < KT / 16; ++kb) {
    const f32x4 pf = *(const f32x4*)(Ps + r * LDP + 16 * kb + 4 * qd);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float* yrow = Ys + (16 * kb + 4 * qd + e) * LD + r;
#pragma unroll
      for (int n = 0; n < NKB; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(pf[e], yrow[16 * n], acc[n], 0, 0, 0);
    }
  }
}

// a * b rounded on its own, never contracted into an FMA with a neighbouring add or subtract
EA_DEV float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

EA_DEV void patch_store(float* Ps, int r, int qd, const f32x4 (&x)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) Ps[(4 * qd + e) * LDP + jt * 16 + r] = x[jt][e];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <typename T, int DKP, int MODE>
__global__ __launch_bounds__(256) void attn_stream_bwd_kernel(StB a) {
  constexpr bool KO = MODE == 1, DSUM = MODE == 2;
  constexpr int LD = DKP + 4, NKB = DKP / 16, C4 = DKP / 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Y1s = (float*)smem;   // (KT, LD) walked tile of the score product: K, or Q when KO
  float* Y2s = Y1s + KT * LD;  // (KT, LD) walked tile of the dP product: V, or dO when KO
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, qd = lane >> 4;
  float* Ps = Y2s + KT * LD + w * 16 * LDP;   // this wave's (16, LDP) patch
  float* Ls = Y2s + KT * LD + 4 * 16 * LDP;   // KO: lse of the walked queries
  float* Dw = Ls + KT;                        // KO: D of the walked queries
  float* Cw = Dw + KT;                        // KO: their normalisers C
  float* Iw = Cw + KT;                        // KO: 1 / C
  const int T1 = a.T1, T2 = a.T2, dk = a.dk;
  const int TA = KO ? T2 : T1;  // length of the owner axis
  const int nat = ea_cdiv(TA, 64);
  const int at = (int)(blockIdx.x % nat);
  const long z = blockIdx.x / nat;
  const int b = (int)(z / a.H), h = (int)(z % a.H);
  long long kl64 = a.klen ? a.klen[b] : (long long)T2;
  const int kl = (int)(kl64 < 0 ? 0 : (kl64 > T2 ? T2 : kl64));
  const int a0 = at * 64 + w * 16;
  const int alim = KO ? kl : T1, clim = KO ? T1 : kl;  // real rows of the owner / walked axis
  const bool live = a0 < alim;                         // wave-uniform
  // walked range: the queries at or below the block's first key when causal / the keys any row can see
  const int cbeg = KO && a.causal ? at * 64 : 0;
  const int cend = KO ? (at * 64 < kl ? T1 : 0) : (a.causal ? min(kl, min(T1, at * 64 + 64)) : kl);

  const T* qp = (const T*)a.q + (long)b * T1 * a.ldq + (long)h * dk;
  const T* kp = (const T*)a.k + (long)b * T2 * a.ldk + (long)h * dk;
  const T* vp = (const T*)a.v + (long)b * T2 * a.ldv + (long)h * dk;
  const T* gp = (const T*)a.dO + (long)b * T1 * a.lddo + (long)h * dk;
  const T* x1 = KO ? kp : qp; const long ldx1 = KO ? a.ldk : a.ldq;
  const T* x2 = KO ? vp : gp; const long ldx2 = KO ? a.ldv : a.lddo;
  const T* y1 = KO ? qp : kp; const long ldy1 = KO ? a.ldq : a.ldk;
  const T* y2 = KO ? gp : vp; const long ldy2 = KO ? a.lddo : a.ldv;

  // owner rows as A operands: lane (r, qd) holds X[a0 + r][16 kb + 4 qd + e]
  f32x4 xa1[NKB], xa2[NKB], acc1[NKB], acc2[KO ? NKB : 1];
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    const int c = 16 * kb + 4 * qd;
    const bool ok = a0 + r < alim && c < dk;
    xa1[kb] = load4_or_zero(x1 + (long)(a0 + r) * ldx1, c, ok);
    xa2[kb] = load4_or_zero(x2 + (long)(a0 + r) * ldx2, c, ok);
    acc1[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (KO) acc2[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // query-owner: lse, D and the normaliser correction of this lane's four rows (DSUM: the partial sums)
  const long nrows = (long)a.B * a.H * T1;
  float lrow[4], drow[4], crow[4], irow[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = a0 + 4 * qd + e;
    const bool ok = !KO && i < T1;
    lrow[e] = ok ? a.lse[z * T1 + i] : -INFINITY;
    drow[e] = ok && !DSUM ? a.D[z * T1 + i] : 0.f;
    crow[e] = DSUM ? 0.f : ok ? a.D[nrows + z * T1 + i] : 1.f;
    irow[e] = DSUM || crow[e] <= 0.f ? 0.f : 1.f / crow[e];
  }
  const bool drop = a.p > 0.f;
  const uint32_t key = drop ? ea_seed_key(ea_salted(a.seed, a.salt)) : 0u, thr = drop ? ea_drop_thr(a.p) : 0u;
  const float keep = drop ? 1.f / (1.f - a.p) : 1.f;
  const long bz = ((long)h * a.B + b) * T1;  // first band row of (h, b)
  T* dbd = MODE == 0 ? (T*)a.dbd : nullptr;

  for (int c0 = cbeg; c0 < cend; c0 += KT) {
    __syncthreads();  // the previous tile has been read
#pragma unroll
    for (int t = 0; t < C4 * KT / 256; ++t) {
      const int idx = tid + t * 256;
      const int row = idx / C4, c = (idx % C4) * 4;
      const bool ok = c0 + row < clim && c < dk;
      *(f32x4*)(Y1s + row * LD + c) = load4_or_zero(y1 + (long)(c0 + row) * ldy1, c, ok);
      *(f32x4*)(Y2s + row * LD + c) = load4_or_zero(y2 + (long)(c0 + row) * ldy2, c, ok);
    }
    if (KO && tid < KT) {
      const bool ok = c0 + tid < T1;
      Ls[tid] = ok ? a.lse[z * T1 + c0 + tid] : -INFINITY;
      Dw[tid] = ok ? a.D[z * T1 + c0 + tid] : 0.f;
      Cw[tid] = ok ? a.D[nrows + z * T1 + c0 + tid] : 1.f;
      Iw[tid] = Cw[tid] > 0.f ? 1.f / Cw[tid] : 0.f;
    }
    __syncthreads();
    if (!live) continue;

    // s[jt][e], dp[jt][e]: owner row a0 + 4 qd + e against walked row c0 + 16 jt + r
    f32x4 s[4], dp[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) s[jt] = dp[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const f32x4 f1 = *(const f32x4*)(Y1s + (jt * 16 + r) * LD + 16 * kb + 4 * qd);
        const f32x4 f2 = *(const f32x4*)(Y2s + (jt * 16 + r) * LD + 16 * kb + 4 * qd);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa1[kb][e], f1[e], s[jt], 0, 0, 0);
          dp[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa2[kb][e], f2[e], dp[jt], 0, 0, 0);
        }
      }
    // P = exp(s - lse), then s <- dS = scale P (m/(1-p) dP - D) and dp <- m/(1-p) P
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const int aa = a0 + 4 * qd + e, cc = c0 + jt * 16 + r;
        const int i = KO ? cc : aa, j = KO ? aa : cc;
        const float L = KO ? Ls[jt * 16 + r] : lrow[e], Dv = KO ? Dw[jt * 16 + r] : drow[e];
        const float Cv = DSUM ? 1.f : KO ? Cw[jt * 16 + r] : crow[e], Iv = KO ? Iw[jt * 16 + r] : irow[e];
        float g = 0.f, pd = 0.f;
        if (i < T1 && j < kl && (!a.causal || j <= i) && L > -INFINITY) {
          float x = s[jt][e];
          if (a.BD) x += a.BD[(bz + i + (a.legacy && j > i)) * a.ldBD + (T1 - 1 - i + j)];
          // e = exp(s - lse) to an ulp.  The largest P of a row sit at s - lse = -log(sum), not at 0 as under
          // a row maximum, where the rounding of the difference and of __expf's argument would cost them
          // several 1e-7: the difference is taken exactly (TwoSum) and the product s * scale with its
          // residual, the low parts applied as 1 + lo, and exp is the full one.
          const float xs = mul_rn(x, a.scale), hi = xs - L, bb = hi - xs;
          const float lo = ((xs - (hi - bb)) + (-L - bb)) + fmaf(x, a.scale, -xs);
          const float ex = expf(hi) * (1.f + lo);
          const float m = !drop || attn_keep(key, thr, (uint64_t)z * T1 + i, T2, j) ? keep : 0.f;
          // t = e m dP, rounded once here and in the row sum D = sum t.  P = e / C by a true division and
          // dS = scale / C (t - P D): for a row with one valid key C = e, P is exactly 1 and t - D exactly 0.
          const float t = mul_rn(ex, mul_rn(m, dp[jt][e]));
          if constexpr (DSUM) {
            drow[e] += t;
            crow[e] += ex;
          } else {
            const float pr = ex / Cv;
            pd = pr * m;
            g = a.scale * Iv * (t - pr * Dv);
          }
        }
        s[jt][e] = g;
        dp[jt][e] = pd;
        if (dbd && i < T1 && j < T1)
          dbd[(bz + i + (a.legacy && j > i)) * a.lddbd + (T1 - 1 - i + j)] = from_f<T>(g);
      }
    if constexpr (DSUM) continue;
    if constexpr (KO) {
      patch_store(Ps, r, qd, dp);
      patch_mma<NKB, LD>(Ps, Y2s, r, qd, acc2);  // dV += (m/(1-p) P)^T dO
      __builtin_amdgcn_wave_barrier();          // the patch is read before dS^T overwrites it
    }
    patch_store(Ps, r, qd, s);
    patch_mma<NKB, LD>(Ps, Y1s, r, qd, acc1);  // dQ += dS K, or dK += dS^T Q
    __builtin_amdgcn_wave_barrier();
  }

  // band positions of this wave's rows the loop did not reach: keys past the last tile walked, the
  // columns left of a row's band and right of it (legacy: the upper part lives on the row below)
  if (dbd && live) {
    const int n2 = 2 * T1 - 1, jcov = min(T1, ea_cdiv(cend, KT) * KT);
    const T zero = from_f<T>(0.f);
    for (int rr = 0; rr < 16 && a0 + rr < T1; ++rr) {
      const int i = a0 + rr;
      T* row = dbd + (bz + i) * a.lddbd;
      for (int j = jcov + lane; j < T1; j += 64) row[(a.legacy && j > i ? a.lddbd : 0) + T1 - 1 - i + j] = zero;
      for (int c = lane; c < T1 - 1 - i; c += 64) row[c] = zero;
      if (!a.legacy || i + 1 < T1)
        for (int c = n2 - i + lane; c < n2; c += 64) row[(a.legacy ? a.lddbd : 0) + c] = zero;
      if (a.legacy && i == 0)  // band row 0 has no query above it
        for (int c = T1 + lane; c < n2; c += 64) row[c] = zero;
    }
  }

  if constexpr (DSUM) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float dsum = group16_sum(drow[e]), csum = group16_sum(crow[e]);
      if (r == 0 && a0 + 4 * qd + e < T1) {
        a.D[z * T1 + a0 + 4 * qd + e] = dsum;
        a.D[nrows + z * T1 + a0 + 4 * qd + e] = csum;
      }
    }
    return;
  }
  T* o1 = (T*)(KO ? a.dk_ : a.dq); const long ldo1 = KO ? a.lddk : a.lddq;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int aa = a0 + 4 * qd + e;
    if (aa >= TA) continue;
    T* r1 = o1 + ((long)b * TA + aa) * ldo1 + (long)h * dk;
    T* r2 = KO ? (T*)a.dv + ((long)b * TA + aa) * a.lddv + (long)h * dk : nullptr;
#pragma unroll
    for (int n = 0; n < NKB; ++n)
      if (16 * n + r < dk) {
        r1[16 * n + r] = from_f<T>(acc1[n][e]);
        if constexpr (KO) r2[16 * n + r] = from_f<T>(acc2[n][e]);
      }
  }
}

template <typename T, int DKP, int MODE>
int launch_stream_bwd_pass(const StB& a, hipStream_t st) {
  constexpr long bytes = stream_bwd_lds_bytes<DKP>();
  if (bytes > 65536) {
    const hipError_t e = hipFuncSetAttribute((const void*)attn_stream_bwd_kernel<T, DKP, MODE>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
  }
  const long blocks = (long)a.B * a.H * ea_cdiv(MODE == 1 ? a.T2 : a.T1, 64);
  if (blocks > 0x7fffffffL) return EA_ERR_BAD_ARG;
  if (blocks == 0) return 0;
  hipLaunchKernelGGL((attn_stream_bwd_kernel<T, DKP, MODE>), dim3((unsigned)blocks), dim3(256), (size_t)bytes, st, a);
  EA_LAUNCH_CHECK();
  return 0;
}

template <typename T, int DKP>
int launch_stream_bwd(const StB& a, hipStream_t st) {
  int rc = launch_stream_bwd_pass<T, DKP, 2>(a, st);
  if (rc == 0) rc = launch_stream_bwd_pass<T, DKP, 1>(a, st);
  return rc ? rc : launch_stream_bwd_pass<T, DKP, 0>(a, st);
}

template <typename T>
int launch_stream_bwd_dk(const StB& a, hipStream_t st) {
  if (a.dk <= 16) return launch_stream_bwd<T, 16>(a, st);
  if (a.dk <= 32) return launch_stream_bwd<T, 32>(a, st);
  if (a.dk <= 64) return launch_stream_bwd<T, 64>(a, st);
  return launch_stream_bwd<T, 128>(a, st);
}

}  // namespace

extern "C" int ea_attn_stream_fwd(int B, int H, int T1, int T2, int dk, const void* q, long ldq, const void* k,
                                  long ldk, const void* v, long ldv, int dtype, const float* BD, long ldBD,
                                  const long long* klen, int causal, float scale, float p, float* O, long ldo,
                                  float* lse, int rel_mode, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(p <= 0.f);  // no dropout: a forward for inference
  return stream_fwd(B, H, T1, T2, dk, q, ldq, k, ldk, v, ldv, dtype, BD, ldBD, klen, causal, scale, 0.f, 0, O, ldo,
                    lse, rel_mode, stream);
}

extern "C" int ea_attn_stream_fwd_train(int B, int H, int T1, int T2, int dk, const void* q, long ldq, const void* k,
                                        long ldk, const void* v, long ldv, int dtype, const float* BD, long ldBD,
                                        const long long* klen, int causal, float scale, float p,
                                        unsigned long long seed, float* O, long ldo, float* lse, int rel_mode,
                                        void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(p >= 0.f && p < 1.f && lse != nullptr);
  return stream_fwd(B, H, T1, T2, dk, q, ldq, k, ldk, v, ldv, dtype, BD, ldBD, klen, causal, scale, p, seed, O, ldo,
                    lse, rel_mode, stream);
}

extern "C" int ea_attn_stream_bwd(int B, int H, int T1, int T2, int dk, const void* q, long ldq, const void* k,
                                  long ldk, const void* v, long ldv, int dtype, const float* BD, long ldBD,
                                  const long long* klen, int causal, float scale, float p, unsigned long long seed,
                                  const float* lse, const void* dO, long lddo, void* dq, long lddq, void* dkout,
                                  long lddk, void* dvout, long lddv, void* dbd, long lddbd,
                                  float* ws, long ws_bytes, int rel_mode, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(p >= 0.f && p < 1.f);
  EA_CHECK_ARG(B >= 0 && H >= 0 && T1 >= 0 && T2 >= 1);
  EA_CHECK_ARG(dk >= 8 && dk <= 128 && dk % 8 == 0);
  EA_CHECK_ARG(dtype == EA_F32 || dtype == EA_BF16);
  EA_CHECK_ARG(rel_mode == EA_REL_LATEST || rel_mode == EA_REL_LEGACY);
  if (rel_mode == EA_REL_LEGACY) EA_CHECK_ARG(BD != nullptr && !causal);
  if (BD) EA_CHECK_ARG(T1 == T2 && ldBD >= 2L * T1 - 1 && dbd != nullptr && lddbd >= 2L * T1 - 1);
  if ((long)B * H == 0) return 0;
  EA_CHECK_ARG(ldk >= dk && ldv >= dk && lddk >= dk && lddv >= dk && ldk % 4 == 0 && ldv % 4 == 0);
  EA_CHECK_ARG(k && v && dkout && dvout && aligned16(k) && aligned16(v));
  if (T1 > 0) {
    EA_CHECK_ARG(ldq >= dk && lddo >= dk && lddq >= dk && ldq % 4 == 0 && lddo % 4 == 0);
    EA_CHECK_ARG(q && lse && dO && dq && aligned16(q) && aligned16(dO));
    EA_CHECK_ARG(ws && ws_bytes >= (long)B * H * T1 * 8);
  }
  const StB a{B, H, T1, T2, dk, scale, q, ldq, k, ldk, v, ldv, BD, ldBD, klen, causal, rel_mode == EA_REL_LEGACY,
              p, (uint64_t)seed, ea_g_rng_salt, lse, dO, lddo, ws, dq, lddq, dkout, lddk, dvout, lddv,
              BD ? dbd : nullptr, lddbd};
  return dtype == EA_BF16 ? launch_stream_bwd_dk<bf16>(a, (hipStream_t)stream)
                          : launch_stream_bwd_dk<float>(a, (hipStream_t)stream);
}
