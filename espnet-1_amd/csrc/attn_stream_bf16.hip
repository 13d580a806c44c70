// Streaming attention on the bf16 matrix cores (v_mfma_f32_16x16x32_bf16, f32 accumulation): the forward,
// training forward and three-sweep backward of attn_stream.hip for bf16 operands.  Same score law, masks,
// rel-pos band indexing and dropout keep law as there (its header); nothing of size T1 x T2 exists and
// there are no atomics.  DESIGN.md §22.
//
// One orientation everywhere: the score tile is computed TRANSPOSED to the walked axis, C[walked][owner], the
// walked tile (64 rows staged in LDS as bf16) as the A operand and the workgroup's own rows (registers, 8 bf16
// of the head dim per lane) as the B operand.  The C layout of the 16x16 MFMA then leaves owner row `r =
// lane & 15` in lane (r, g = lane >> 4) with walked rows 16 jt + 4 g + e (jt, e < 4) in its 16 accumulator
// registers: one owner row per lane.
//   - softmax statistics are per-lane scalars: a row's maximum / sum is an in-register reduction and two
//     shuffles (xor 16, 32) instead of four 4-step shuffles;
//   - rounded to bf16, the 16 values of a lane ARE the B operand of the second product (contraction over the
//     walked axis, 8 values per 16x16x32 step: walked rows {32 h + 4 g + e, 32 h + 16 + 4 g + e}): no LDS
//     patch, no wave barrier.  The second product is computed transposed too, out^T[d][owner] = Y^T P^T,
//     its A operand Y^T read from a transposed copy of the walked tile ((DKP, 64 + 4) bf16: two 8-byte
//     reads per step), so the accumulator again has one owner row per lane and the online-softmax rescale
//     is a per-lane scalar.
// LDS strides: row-major tiles DKP + 8 bf16 (20 / 36 / 68 dwords: 16-byte operand reads of 16 rows land
// 4 r (mod 32) dwords apart, every bank equally often); transposed tiles 64 + 4 bf16 (34 dwords: 8-byte reads
// of 16 rows at 2 r + 2 g (mod 32), every bank equally often).  Head dims below DKP are zero columns in LDS
// and registers.  The forward double-buffers its K / V^T tiles: the next tile's global loads are issued
// before this tile's MFMA and stored after it, one barrier a tile.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

constexpr int KT = 64;       // walked rows per tile
constexpr int LDT = KT + 4;  // row stride of a transposed tile

struct StP {
  int B, H, T1, T2, dk;
  float scale;
  const bf16* q; long ldq;
  const bf16* k; long ldk;
  const bf16* v; long ldv;
  const float* BD; long ldBD;
  const long long* klen;
  int causal, legacy;
  bf16* O; long ldo;
  float* lse;
  float p; uint64_t seed; const unsigned long long* salt;  // DROP instantiations only
};

EA_DEV float quad_max(float v) {  // over the four lanes (r, 0..3) of an owner row
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
EA_DEV float quad_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// a * b rounded on its own, never contracted into an FMA with a neighbouring add or subtract
EA_DEV float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

EA_DEV bf16x8 zero8() {
  const f32x4 z{0.f, 0.f, 0.f, 0.f};
  return __builtin_bit_cast(bf16x8, z);
}
EA_DEV bf16x8 load8_or_zero(const bf16* row, int c, bool ok) { return ok ? *(const bf16x8*)(row + c) : zero8(); }

// A (64, DKP) tile as DKP/32 chunks of 8 bf16 per thread: chunk idx -> row idx / C8, columns 8 (idx % C8)
template <int DKP>
EA_DEV void tile_fetch(bf16x8 (&reg)[DKP / 32], const bf16* base, long ld, int row0, int rlim, int dk, int tid) {
  constexpr int C8 = DKP / 8;
#pragma unroll
  for (int t = 0; t < DKP / 32; ++t) {
    const int idx = tid + t * 256, row = idx / C8, c = (idx % C8) * 8;
    reg[t] = load8_or_zero(base + (long)(row0 + row) * ld, c, row0 + row < rlim && c < dk);
  }
}
template <int DKP>
EA_DEV void tile_put(bf16* S, const bf16x8 (&reg)[DKP / 32], int tid) {  // row-major (KT, DKP + 8)
  constexpr int C8 = DKP / 8;
#pragma unroll
  for (int t = 0; t < DKP / 32; ++t) {
    const int idx = tid + t * 256;
    *(bf16x8*)(S + (idx / C8) * (DKP + 8) + (idx % C8) * 8) = reg[t];
  }
}
template <int DKP>
EA_DEV void tile_put_tr(bf16* St, const bf16x8 (&reg)[DKP / 32], int tid) {  // transposed (DKP, LDT)
  constexpr int C8 = DKP / 8;
#pragma unroll
  for (int t = 0; t < DKP / 32; ++t) {
    const int idx = tid + t * 256, row = idx / C8, c = (idx % C8) * 8;
#pragma unroll
    for (int u = 0; u < 8; ++u) St[(c + u) * LDT + row] = reg[t][u];
  }
}

// s[jt] += Y[16 jt + r][:] . x (the owner row's registers): C[walked 16 jt + 4 g + e][owner r]
template <int DKP>
EA_DEV void score_mma(const bf16* Y, const bf16x8 (&x)[DKP / 32], int r, int g, f32x4 (&s)[4]) {
#pragma unroll
  for (int kb = 0; kb < DKP / 32; ++kb)
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      const bf16x8 y = *(const bf16x8*)(Y + (jt * 16 + r) * (DKP + 8) + 32 * kb + 8 * g);
      s[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(y, x[kb], s[jt], 0, 0, 0);
    }
}
// acc[n] += Y^T[16 n + r][walked] . pb: out^T[d 16 n + 4 g + e][owner r]
template <int DKP>
EA_DEV void walk_mma(const bf16* Yt, const bf16x8 (&pb)[2], int r, int g, f32x4 (&acc)[DKP / 16]) {
#pragma unroll
  for (int n = 0; n < DKP / 16; ++n)
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2) {
      const bf16* yr = Yt + (16 * n + r) * LDT + 32 * h2 + 4 * g;
      const bf16x8 y = __builtin_shufflevector(*(const bf16x4*)yr, *(const bf16x4*)(yr + 16), 0, 1, 2, 3, 4, 5, 6, 7);
      acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(y, pb[h2], acc[n], 0, 0, 0);
    }
}
// the 16 values of a lane as the B operand of walk_mma
EA_DEV void pack_b(const f32x4 (&x)[4], bf16x8 (&pb)[2]) {
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int e = 0; e < 4; ++e) pb[jt >> 1][(jt & 1) * 4 + e] = (bf16)x[jt][e];
}
// out^T accumulators to (rows, ld) bf16: 4 consecutive head-dim columns per lane and 16-column block
template <int DKP>
EA_DEV void store_rows(bf16* row, int dk, int g, const f32x4 (&acc)[DKP / 16], float mul) {
#pragma unroll
  for (int n = 0; n < DKP / 16; ++n)
    if (16 * n + 4 * g < dk) {
      const float t[4] = {acc[n][0] * mul, acc[n][1] * mul, acc[n][2] * mul, acc[n][3] * mul};
      vst4(row + 16 * n + 4 * g, t);
    }
}

template <int DKP> constexpr long fwd_lds_bytes() { return 2L * (KT * (DKP + 8) + DKP * LDT) * 2; }

template <int DKP, bool DROP>
__global__ __launch_bounds__(256) void attn_stream_bf16_kernel(StP a) {
  constexpr int KB = KT * (DKP + 8), VB = DKP * LDT, NKB = DKP / 32, ND = DKP / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16* Ks = (bf16*)smem;  // 2 x (KT, DKP + 8)
  bf16* Vt = Ks + 2 * KB;  // 2 x (DKP, LDT)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
  const int nqt = ea_cdiv(a.T1, 64);
  const int qt = (int)(blockIdx.x % nqt);
  const long z = blockIdx.x / nqt;
  const int b = (int)(z / a.H), h = (int)(z % a.H);
  const int T1 = a.T1, T2 = a.T2, dk = a.dk;
  long long kl64 = a.klen ? a.klen[b] : (long long)T2;
  const int kl = (int)(kl64 < 0 ? 0 : (kl64 > T2 ? T2 : kl64));
  const int kend = a.causal ? min(kl, min(T1, qt * 64 + 64)) : kl;  // keys any row of the block can see
  const int i0 = qt * 64 + w * 16, i = i0 + r;
  const bool live = i0 < T1, rowok = i < T1;  // live: wave-uniform

  const bf16* qp = a.q + (long)b * T1 * a.ldq + (long)h * dk;
  const bf16* kp = a.k + (long)b * T2 * a.ldk + (long)h * dk;
  const bf16* vp = a.v + (long)b * T2 * a.ldv + (long)h * dk;

  bf16x8 qb[NKB];  // lane (r, g): Q[i][32 kb + 8 g ..]
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) qb[kb] = load8_or_zero(qp + (long)i * a.ldq, 32 * kb + 8 * g, rowok && 32 * kb + 8 * g < dk);
  f32x4 o[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;  // the row's running maximum, this lane's part of its running sum
  const float* bdrow = a.BD && rowok ? a.BD + (((long)h * a.B + b) * T1 + i) * a.ldBD + (T1 - 1 - i) : nullptr;
  const int lim = rowok ? (a.causal ? min(kl, i + 1) : kl) : 0;
  const uint32_t key = DROP ? ea_seed_key(ea_salted(a.seed, a.salt)) : 0u, thr = DROP ? ea_drop_thr(a.p) : 0u;
  const float keep = DROP ? 1.f / (1.f - a.p) : 1.f;

  const int ntiles = ea_cdiv(kend, KT);
  bf16x8 kr[NKB], vr[NKB];
  if (ntiles > 0) {
    tile_fetch<DKP>(kr, kp, a.ldk, 0, kl, dk, tid);
    tile_fetch<DKP>(vr, vp, a.ldv, 0, kl, dk, tid);
    tile_put<DKP>(Ks, kr, tid);
    tile_put_tr<DKP>(Vt, vr, tid);
  }
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    const int j0 = t * KT;
    const bool more = t + 1 < ntiles;
    if (more) {  // in flight across this tile's MFMA
      tile_fetch<DKP>(kr, kp, a.ldk, j0 + KT, kl, dk, tid);
      tile_fetch<DKP>(vr, vp, a.ldv, j0 + KT, kl, dk, tid);
    }
    if (live) {
      const bf16* Kb = Ks + (t & 1) * KB;
      const bf16* Vb = Vt + (t & 1) * VB;
      f32x4 s[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) s[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
      score_mma<DKP>(Kb, qb, r, g, s);  // s[jt][e]: key j0 + 16 jt + 4 g + e, query i
      float mx = -INFINITY;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int j = j0 + 16 * jt + 4 * g + e;
          float x = -INFINITY;
          if (j < lim) {
            x = s[jt][e];
            if (bdrow) x += a.legacy && j > i ? bdrow[a.ldBD + j] : bdrow[j];
            x = mul_rn(x, a.scale);
          }
          s[jt][e] = x;
          mx = fmaxf(mx, x);
        }
      const float mnew = fmaxf(m, quad_max(mx));
      const bool any = mnew > -INFINITY;  // some valid key so far
      const float alpha = any ? __expf(m - mnew) : 1.f;
      m = mnew;
      float ps = 0.f;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float p = any ? __expf(s[jt][e] - mnew) : 0.f;
          ps += p;  // the row sum, and so lse, is that of the undropped scores
          if (DROP) p = attn_keep(key, thr, (uint64_t)z * T1 + i, T2, j0 + 16 * jt + 4 * g + e) ? p * keep : 0.f;
          s[jt][e] = p;
        }
      l = l * alpha + ps;
#pragma unroll
      for (int n = 0; n < ND; ++n) o[n] *= alpha;
      bf16x8 pb[2];
      pack_b(s, pb);
      walk_mma<DKP>(Vb, pb, r, g, o);  // O^T += V^T P^T
    }
    if (more) {  // the other buffer: last read before the barrier that ended tile t - 1
      tile_put<DKP>(Ks + ((t + 1) & 1) * KB, kr, tid);
      tile_put_tr<DKP>(Vt + ((t + 1) & 1) * VB, vr, tid);
    }
    __syncthreads();
  }

  if (!live) return;
  l = quad_sum(l);
  if (!rowok) return;
  store_rows<DKP>(a.O + ((long)b * T1 + i) * a.ldo + (long)h * dk, dk, g, o, l > 0.f ? 1.f / l : 0.f);
  if (a.lse && g == 0) a.lse[z * T1 + i] = l > 0.f ? m + __logf(l) : -INFINITY;
}

template <int DKP, bool DROP>
int launch_fwd(const StP& a, hipStream_t st) {
  constexpr long bytes = fwd_lds_bytes<DKP>();
  if (bytes > 65536) {  // a host-side attribute of the current device's function, no stream work
    const hipError_t e = hipFuncSetAttribute((const void*)attn_stream_bf16_kernel<DKP, DROP>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
  }
  const long blocks = (long)a.B * a.H * ea_cdiv(a.T1, 64);
  if (blocks > 0x7fffffffL) return EA_ERR_BAD_ARG;
  hipLaunchKernelGGL((attn_stream_bf16_kernel<DKP, DROP>), dim3((unsigned)blocks), dim3(256), (size_t)bytes, st, a);
  EA_LAUNCH_CHECK();
  return 0;
}

template <bool DROP>
int launch_fwd_dk(const StP& a, hipStream_t st) {
  if (a.dk <= 32) return launch_fwd<32, DROP>(a, st);
  if (a.dk <= 64) return launch_fwd<64, DROP>(a, st);
  return launch_fwd<128, DROP>(a, st);
}

bool aligned_to(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

int stream_fwd(int B, int H, int T1, int T2, int dk, const void* q, long ldq, const void* k, long ldk, const void* v,
               long ldv, const float* BD, long ldBD, const long long* klen, int causal, float scale, float p,
               unsigned long long seed, void* O, long ldo, float* lse, int rel_mode, void* stream) {
  EA_CHECK_ARG(B >= 0 && H >= 0 && T1 >= 0 && T2 >= 1);
  EA_CHECK_ARG(dk >= 8 && dk <= 128 && dk % 8 == 0);
  EA_CHECK_ARG(rel_mode == EA_REL_LATEST || rel_mode == EA_REL_LEGACY);
  if (rel_mode == EA_REL_LEGACY) EA_CHECK_ARG(BD != nullptr && !causal);
  if (BD) EA_CHECK_ARG(T1 == T2 && ldBD >= 2L * T1 - 1);
  if ((long)B * H * T1 == 0) return 0;
  EA_CHECK_ARG(ldq >= dk && ldk >= dk && ldv >= dk && ldo >= dk);
  EA_CHECK_ARG(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 4 == 0);
  EA_CHECK_ARG(q && k && v && O && aligned_to(q, 16) && aligned_to(k, 16) && aligned_to(v, 16) && aligned_to(O, 8));
  const StP a{B, H, T1, T2, dk, scale, (const bf16*)q, ldq, (const bf16*)k, ldk, (const bf16*)v, ldv, BD, ldBD, klen,
              causal, rel_mode == EA_REL_LEGACY, (bf16*)O, ldo, lse, p, (uint64_t)seed, ea_g_rng_salt};
  return p > 0.f ? launch_fwd_dk<true>(a, (hipStream_t)stream) : launch_fwd_dk<false>(a, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------ backward
// The three sweeps of attn_stream.hip, each recomputing the scores from q, k and lse, in the orientation of
// the header: a workgroup owns 64 rows of one (b, h) on the OWNER axis, a lane one of them.
//   MODE 2, row sums: owner = queries; D_i = sum_j (m/(1-p) P_ij) dP_ij (= dO_i . O_i, from the MFMA values the
//     passes recompute), a per-lane scalar reduced over the row's four lanes at the end.
//   MODE 0, query owner: walked K and V row-major (S^T = K Q^T, dP^T = V dO^T) and K transposed;
//     dQ^T += K^T dS^T with the lane's 16 dS values as the B operand.  The dS registers are also the band
//     gradient; afterwards the wave zero-fills the band positions of its rows no (i, j) landed on.
//   MODE 1, key owner: walked Q and dO row-major (S = Q K^T, dP = dO V^T) and both transposed;
//     dV^T += dO^T (m/(1-p) P), dK^T += Q^T dS.
// P = exp(s - lse) in f32; only the MFMA operands (m/(1-p) P and dS) are rounded to bf16.  A row with one
// valid key has lse = s, P = 1 and D = its one term, so its dS is an exact zero.
struct StB {
  int B, H, T1, T2, dk;
  float scale;
  const bf16* q; long ldq;
  const bf16* k; long ldk;
  const bf16* v; long ldv;
  const float* BD; long ldBD;
  const long long* klen;
  int causal, legacy;
  float p; uint64_t seed; const unsigned long long* salt;
  const float* lse;
  const bf16* dO; long lddo;
  float* D;  // the row-sum sweep's output [z][i]
  bf16* dq; long lddq;
  bf16* dk_; long lddk;
  bf16* dv; long lddv;
  bf16* dbd; long lddbd;
};

template <int DKP, int MODE> constexpr long bwd_lds_bytes() {
  return (2L * KT * (DKP + 8) + (MODE == 2 ? 0 : MODE == 1 ? 2 : 1) * DKP * LDT) * 2 + (MODE == 1 ? 2 * KT * 4 : 0);
}

template <int DKP, int MODE>
__global__ __launch_bounds__(256) void attn_stream_bf16_bwd_kernel(StB a) {
  constexpr bool KO = MODE == 1, DSUM = MODE == 2;
  constexpr int RB = KT * (DKP + 8), TB = DKP * LDT, NKB = DKP / 32, ND = DKP / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16* Y1s = (bf16*)smem;                  // (KT, DKP + 8) walked tile of the score product: K, or Q when KO
  bf16* Y2s = Y1s + RB;                     // (KT, DKP + 8) walked tile of the dP product: V, or dO when KO
  bf16* Y1t = Y2s + RB;                     // (DKP, LDT) Y1 transposed (not DSUM)
  bf16* Y2t = Y1t + TB;                     // (DKP, LDT) Y2 transposed (KO)
  float* Ls = (float*)(Y2t + TB);           // KO: lse of the walked queries
  float* Dw = Ls + KT;                      // KO: their D
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
  const int T1 = a.T1, T2 = a.T2, dk = a.dk;
  const int TA = KO ? T2 : T1;  // length of the owner axis
  const int nat = ea_cdiv(TA, 64);
  const int at = (int)(blockIdx.x % nat);
  const long z = blockIdx.x / nat;
  const int b = (int)(z / a.H), h = (int)(z % a.H);
  long long kl64 = a.klen ? a.klen[b] : (long long)T2;
  const int kl = (int)(kl64 < 0 ? 0 : (kl64 > T2 ? T2 : kl64));
  const int a0 = at * 64 + w * 16, aa = a0 + r;
  const int alim = KO ? kl : T1, clim = KO ? T1 : kl;  // real rows of the owner / walked axis
  const bool live = a0 < alim;                         // wave-uniform
  // walked range: the queries at or below the block's first key when causal / the keys any row can see
  const int cbeg = KO && a.causal ? at * 64 : 0;
  const int cend = KO ? (at * 64 < kl ? T1 : 0) : (a.causal ? min(kl, min(T1, at * 64 + 64)) : kl);

  const bf16* qp = a.q + (long)b * T1 * a.ldq + (long)h * dk;
  const bf16* kp = a.k + (long)b * T2 * a.ldk + (long)h * dk;
  const bf16* vp = a.v + (long)b * T2 * a.ldv + (long)h * dk;
  const bf16* gp = a.dO + (long)b * T1 * a.lddo + (long)h * dk;
  const bf16* x1 = KO ? kp : qp; const long ldx1 = KO ? a.ldk : a.ldq;
  const bf16* x2 = KO ? vp : gp; const long ldx2 = KO ? a.ldv : a.lddo;
  const bf16* y1 = KO ? qp : kp; const long ldy1 = KO ? a.ldq : a.ldk;
  const bf16* y2 = KO ? gp : vp; const long ldy2 = KO ? a.lddo : a.ldv;

  // the owner row as B operands: lane (r, g) holds X[aa][32 kb + 8 g ..]
  bf16x8 xb1[NKB], xb2[NKB];
  f32x4 acc1[ND], acc2[KO ? ND : 1];
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    const int c = 32 * kb + 8 * g;
    xb1[kb] = load8_or_zero(x1 + (long)aa * ldx1, c, aa < alim && c < dk);
    xb2[kb] = load8_or_zero(x2 + (long)aa * ldx2, c, aa < alim && c < dk);
  }
#pragma unroll
  for (int n = 0; n < ND; ++n) {
    acc1[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (KO) acc2[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // query owner: lse and D of the lane's row (DSUM: its partial sum)
  const float lown = !KO && aa < T1 ? a.lse[z * T1 + aa] : -INFINITY;
  const float down = MODE == 0 && aa < T1 ? a.D[z * T1 + aa] : 0.f;
  float dsum = 0.f;
  const bool drop = a.p > 0.f;
  const uint32_t key = drop ? ea_seed_key(ea_salted(a.seed, a.salt)) : 0u, thr = drop ? ea_drop_thr(a.p) : 0u;
  const float keep = drop ? 1.f / (1.f - a.p) : 1.f;
  const long bz = ((long)h * a.B + b) * T1;  // first band row of (h, b)
  bf16* dbd = MODE == 0 ? a.dbd : nullptr;

  for (int c0 = cbeg; c0 < cend; c0 += KT) {
    __syncthreads();  // the previous tile has been read
    {
      bf16x8 reg[NKB];
      tile_fetch<DKP>(reg, y1, ldy1, c0, clim, dk, tid);
      tile_put<DKP>(Y1s, reg, tid);
      if constexpr (!DSUM) tile_put_tr<DKP>(Y1t, reg, tid);
      tile_fetch<DKP>(reg, y2, ldy2, c0, clim, dk, tid);
      tile_put<DKP>(Y2s, reg, tid);
      if constexpr (KO) tile_put_tr<DKP>(Y2t, reg, tid);
    }
    if (KO && tid < KT) {
      const bool ok = c0 + tid < T1;
      Ls[tid] = ok ? a.lse[z * T1 + c0 + tid] : -INFINITY;
      Dw[tid] = ok ? a.D[z * T1 + c0 + tid] : 0.f;
    }
    __syncthreads();
    if (!live) continue;

    // s[jt][e], dp[jt][e]: walked row c0 + 16 jt + 4 g + e against owner row aa
    f32x4 s[4], dp[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) s[jt] = dp[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
    score_mma<DKP>(Y1s, xb1, r, g, s);
    score_mma<DKP>(Y2s, xb2, r, g, dp);
    // P = exp(s - lse), then s <- dS = scale P (m/(1-p) dP - D) and dp <- m/(1-p) P
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int cl = 16 * jt + 4 * g + e, cc = c0 + cl;
        const int i = KO ? cc : aa, j = KO ? aa : cc;
        const float L = KO ? Ls[cl] : lown, Dv = KO ? Dw[cl] : down;
        float gs = 0.f, pd = 0.f;
        if (i < T1 && j < kl && (!a.causal || j <= i) && L > -INFINITY) {
          float x = s[jt][e];
          if (a.BD) x += a.BD[(bz + i + (a.legacy && j > i)) * a.ldBD + (T1 - 1 - i + j)];
          const float ex = __expf(mul_rn(x, a.scale) - L);  // the forward's rounding of the scaled score
          const float mk = !drop || attn_keep(key, thr, (uint64_t)z * T1 + i, T2, j) ? keep : 0.f;
          const float t = ex * (mk * dp[jt][e]);
          if constexpr (DSUM) {
            dsum += t;
          } else {
            pd = ex * mk;
            gs = a.scale * (t - ex * Dv);
          }
        }
        s[jt][e] = gs;
        dp[jt][e] = pd;
        if (dbd && i < T1 && j < T1) dbd[(bz + i + (a.legacy && j > i)) * a.lddbd + (T1 - 1 - i + j)] = (bf16)gs;
      }
    if constexpr (DSUM) continue;
    bf16x8 pb[2];
    if constexpr (KO) {
      pack_b(dp, pb);
      walk_mma<DKP>(Y2t, pb, r, g, acc2);  // dV^T += dO^T (m/(1-p) P)
    }
    pack_b(s, pb);
    walk_mma<DKP>(Y1t, pb, r, g, acc1);  // dQ^T += K^T dS^T, or dK^T += Q^T dS
  }

  // band positions of this wave's rows the loop did not reach: keys past the last tile walked, the
  // columns left of a row's band and right of it (legacy: the upper part lives on the row below)
  if (dbd && live) {
    const int n2 = 2 * T1 - 1, jcov = min(T1, ea_cdiv(cend, KT) * KT);
    const bf16 zero = (bf16)0.f;
    for (int rr = 0; rr < 16 && a0 + rr < T1; ++rr) {
      const int i = a0 + rr;
      bf16* row = dbd + (bz + i) * a.lddbd;
      for (int j = jcov + lane; j < T1; j += 64) row[(a.legacy && j > i ? a.lddbd : 0) + T1 - 1 - i + j] = zero;
      for (int c = lane; c < T1 - 1 - i; c += 64) row[c] = zero;
      if (!a.legacy || i + 1 < T1)
        for (int c = n2 - i + lane; c < n2; c += 64) row[(a.legacy ? a.lddbd : 0) + c] = zero;
      if (a.legacy && i == 0)  // band row 0 has no query above it
        for (int c = T1 + lane; c < n2; c += 64) row[c] = zero;
    }
  }

  if constexpr (DSUM) {
    dsum = quad_sum(dsum);
    if (g == 0 && aa < T1) a.D[z * T1 + aa] = dsum;
    return;
  }
  if (aa >= TA) return;
  store_rows<DKP>((KO ? a.dk_ : a.dq) + ((long)b * TA + aa) * (KO ? a.lddk : a.lddq) + (long)h * dk, dk, g, acc1, 1.f);
  if constexpr (KO) store_rows<DKP>(a.dv + ((long)b * TA + aa) * a.lddv + (long)h * dk, dk, g, acc2, 1.f);
}

template <int DKP, int MODE>
int launch_bwd_pass(const StB& a, hipStream_t st) {
  constexpr long bytes = bwd_lds_bytes<DKP, MODE>();
  if (bytes > 65536) {
    const hipError_t e = hipFuncSetAttribute((const void*)attn_stream_bf16_bwd_kernel<DKP, MODE>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
  }
  const long blocks = (long)a.B * a.H * ea_cdiv(MODE == 1 ? a.T2 : a.T1, 64);
  if (blocks > 0x7fffffffL) return EA_ERR_BAD_ARG;
  if (blocks == 0) return 0;
  hipLaunchKernelGGL((attn_stream_bf16_bwd_kernel<DKP, MODE>), dim3((unsigned)blocks), dim3(256), (size_t)bytes, st, a);
  EA_LAUNCH_CHECK();
  return 0;
}

template <int DKP>
int launch_bwd(const StB& a, hipStream_t st) {
  int rc = launch_bwd_pass<DKP, 2>(a, st);
  if (rc == 0) rc = launch_bwd_pass<DKP, 1>(a, st);
  return rc ? rc : launch_bwd_pass<DKP, 0>(a, st);
}

}  // namespace

extern "C" int ea_attn_stream_bf16_fwd(int B, int H, int T1, int T2, int dk, const void* q, long ldq, const void* k,
                                       long ldk, const void* v, long ldv, const float* BD, long ldBD,
                                       const long long* klen, int causal, float scale, float p, void* O, long ldo,
                                       float* lse, int rel_mode, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(p <= 0.f);  // no dropout: a forward for inference
  return stream_fwd(B, H, T1, T2, dk, q, ldq, k, ldk, v, ldv, BD, ldBD, klen, causal, scale, 0.f, 0, O, ldo, lse,
                    rel_mode, stream);
}

extern "C" int ea_attn_stream_bf16_fwd_train(int B, int H, int T1, int T2, int dk, const void* q, long ldq,
                                             const void* k, long ldk, const void* v, long ldv, const float* BD,
                                             long ldBD, const long long* klen, int causal, float scale, float p,
                                             unsigned long long seed, void* O, long ldo, float* lse, int rel_mode,
                                             void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(p >= 0.f && p < 1.f && lse != nullptr);
  return stream_fwd(B, H, T1, T2, dk, q, ldq, k, ldk, v, ldv, BD, ldBD, klen, causal, scale, p, seed, O, ldo, lse,
                    rel_mode, stream);
}

extern "C" int ea_attn_stream_bf16_bwd(int B, int H, int T1, int T2, int dk, const void* q, long ldq, const void* k,
                                       long ldk, const void* v, long ldv, const float* BD, long ldBD,
                                       const long long* klen, int causal, float scale, float p,
                                       unsigned long long seed, const float* lse, const void* dO, long lddo, void* dq,
                                       long lddq, void* dkout, long lddk, void* dvout, long lddv, void* dbd,
                                       long lddbd, float* ws, long ws_bytes, int rel_mode, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(p >= 0.f && p < 1.f);
  EA_CHECK_ARG(B >= 0 && H >= 0 && T1 >= 0 && T2 >= 1);
  EA_CHECK_ARG(dk >= 8 && dk <= 128 && dk % 8 == 0);
  EA_CHECK_ARG(rel_mode == EA_REL_LATEST || rel_mode == EA_REL_LEGACY);
  if (rel_mode == EA_REL_LEGACY) EA_CHECK_ARG(BD != nullptr && !causal);
  if (BD) EA_CHECK_ARG(T1 == T2 && ldBD >= 2L * T1 - 1 && dbd != nullptr && lddbd >= 2L * T1 - 1);
  if ((long)B * H == 0) return 0;
  EA_CHECK_ARG(ldk >= dk && ldv >= dk && lddk >= dk && lddv >= dk);
  EA_CHECK_ARG(ldk % 8 == 0 && ldv % 8 == 0 && lddk % 4 == 0 && lddv % 4 == 0);
  EA_CHECK_ARG(k && v && dkout && dvout && aligned_to(k, 16) && aligned_to(v, 16) && aligned_to(dkout, 8) &&
               aligned_to(dvout, 8));
  if (T1 > 0) {
    EA_CHECK_ARG(ldq >= dk && lddo >= dk && lddq >= dk && ldq % 8 == 0 && lddo % 8 == 0 && lddq % 4 == 0);
    EA_CHECK_ARG(q && lse && dO && dq && aligned_to(q, 16) && aligned_to(dO, 16) && aligned_to(dq, 8));
    EA_CHECK_ARG(ws && ws_bytes >= (long)B * H * T1 * 4);
  }
  const StB a{B, H, T1, T2, dk, scale, (const bf16*)q, ldq, (const bf16*)k, ldk, (const bf16*)v, ldv, BD, ldBD, klen,
              causal, rel_mode == EA_REL_LEGACY, p, (uint64_t)seed, ea_g_rng_salt, lse, (const bf16*)dO, lddo, ws,
              (bf16*)dq, lddq, (bf16*)dkout, lddk, (bf16*)dvout, lddv, BD ? (bf16*)dbd : nullptr, lddbd};
  hipStream_t st = (hipStream_t)stream;
  if (dk <= 32) return launch_bwd<32>(a, st);
  if (dk <= 64) return launch_bwd<64>(a, st);
  return launch_bwd<128>(a, st);
}
