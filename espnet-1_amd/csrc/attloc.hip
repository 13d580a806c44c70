// Location-aware attention (AttLoc, espnet/nets/pytorch_backend/rnn/attentions.py:249-379) of the
// attention-RNN decoder: one decoding step of B utterances, forward (ea_attloc_fwd) and backward
// (ea_attloc_bwd).  The products around it (mlp_enc over all frames, mlp_dec of the query, the
// LSTM input projection of the context) are the caller's GEMMs.
//
//   conv[t,c] = sum_k K[c,k] aprev[t+k-F]                     (aprev = 0 outside [0, n))
//   e[t]      = g0 + sum_a g[a] tanh(pre_enc[b,t,a] + dec[b,a] + sum_c M[a,c] conv[t,c])
//   w[t]      = softmax_t(2 e[t]) over t < n = hlens[b], 0 for t >= n;   c[b,:] = sum_t w[t] hs[b,t,:]
//
// Launches (plain, stream ordered; no block waits for another, no atomics, every output element
// has one owner, so every sum runs in a fixed order):
//   forward   score    grid (ceil(T/16), B): the block's 16 frames: conv (one wave per (frame,
//                      channel), lanes over the taps), then one wave per 4 frames, lanes over the
//                      attention units
//             context  grid (ceil(E/64), B): the softmax over the utterance's n scores inside the
//                      block, then 64 columns of hs x 4 frame groups
//   backward  frames   grid (ceil(T/16), B): dw[t] = hs[b,t,:] . dc + dw_next, dhs += w[t] dc, conv
//             units    grid (ceil(A/64), B): 64 attention units x all frames of the utterance:
//                      u = tanh(..) recomputed, dpre, dPre +=, ddec, and through a 32-frame LDS
//                      tile the dM partial and this unit chunk's part of dconv (its rows of M
//                      and the tile's rows of conv staged in LDS while (64 + 32) C floats fit 32 KB)
//             dconv    sums the unit chunks' parts of dconv in chunk order
//             loc      each channel's part of daprev, and the dK partial
//             daprev   sums the channels' parts in channel order (the next launch's dw_next)
// Frames t >= n are never read.  T, A, C, F, E are any positive integers (loops, no caps).
// All sums, tanhf, expf and the softmax are f32; hs and pre_enc are f32 or bf16 memory.
#include "common.h"

namespace {

constexpr int TF = 16;  // frames per block of the frame-major kernels (4 waves x FW frames)
constexpr int FW = TF / 4;
constexpr int AC = 64;  // attention units per block of the unit-major kernel
constexpr int TT = 32;  // frames per LDS tile there
constexpr float SCALING = 2.0f;  // AttLoc.forward(scaling=2.0)

EA_DEV int valid_frames(const long long* hlens, int b, int T) {
  const long long n = hlens[b];
  return n < 0 ? 0 : (n > T ? T : (int)n);
}

// conv[t, c] of one utterance for frames [t0, t1), t1 <= n, by the whole block (every thread must
// call it): one wave per (frame, channel), its lanes over the taps in strides of 64 and a fixed
// shuffle tree over the lanes' sums.  ap: the utterance's aprev row, or NULL = 1 / n.
EA_DEV void conv_frames(const float* __restrict__ K, int C, int F, const float* __restrict__ ap, int n, int t0,
                        int t1, float* __restrict__ conv) {
  const int KW = 2 * F + 1;
  const float inv_n = 1.f / (float)n;
  const int cnt = (t1 - t0) * C, lane = threadIdx.x & 63;
  for (int i = threadIdx.x >> 6; i < cnt; i += blockDim.x >> 6) {
    const int t = t0 + i / C, c = i % C;
    const int j0 = t - F > 0 ? t - F : 0, j1 = t + F < n - 1 ? t + F : n - 1;
    const float* kr = K + (long)c * KW;
    float s = 0.f;
    for (int j = j0 + lane; j <= j1; j += 64) s += kr[j - t + F] * (ap ? ap[j] : inv_n);
    s = wave_sum(s);
    if (lane == 0) conv[(long)t * C + c] = s;
  }
}

struct FwdP {
  int B, T, E, A, C, F;
  const void* hs; long ldhs, shs;
  const void* pre; long ldpre, spre;
  const long long* hlens;
  const float* dec; long lddec;
  const float* aprev; long ldap;
  const float *K, *M, *g, *g0;
  float* w; long ldw;
  float* c; long ldc;
  float* e;     // (B, T) scores
  float* conv;  // (B, T, C)
};

template <typename MT>
__global__ __launch_bounds__(256) void attloc_score_kernel(FwdP p) {
  const int b = blockIdx.y, n = valid_frames(p.hlens, b, p.T);
  const int t0 = blockIdx.x * TF;
  if (t0 >= n) return;
  const int t1 = t0 + TF < n ? t0 + TF : n;
  float* conv = p.conv + (long)b * p.T * p.C;
  conv_frames(p.K, p.C, p.F, p.aprev ? p.aprev + (long)b * p.ldap : nullptr, n, t0, t1, conv);
  __syncthreads();  // the block reads back its own conv rows
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int f0 = t0 + wave * FW;
  if (f0 >= t1) return;
  int tf[FW];  // frames past the block's last valid one repeat it and are not stored
#pragma unroll
  for (int f = 0; f < FW; ++f) tf[f] = f0 + f < t1 ? f0 + f : t1 - 1;
  const MT* pre = (const MT*)p.pre + (long)b * p.spre;
  const float* dec = p.dec + (long)b * p.lddec;
  float acc[FW] = {};
  for (int a = lane; a < p.A; a += 64) {
    float s[FW] = {};
    const float* m = p.M + (long)a * p.C;
    for (int c = 0; c < p.C; ++c) {
      const float mv = m[c];
#pragma unroll
      for (int f = 0; f < FW; ++f) s[f] += mv * conv[(long)tf[f] * p.C + c];
    }
    const float d = dec[a], gv = p.g[a];
#pragma unroll
    for (int f = 0; f < FW; ++f) acc[f] += gv * tanhf(to_f(pre[(long)tf[f] * p.ldpre + a]) + d + s[f]);
  }
#pragma unroll
  for (int f = 0; f < FW; ++f) {
    const float v = wave_sum(acc[f]);
    if (lane == 0 && f0 + f < t1) p.e[(long)b * p.T + f0 + f] = v + p.g0[0];
  }
}

template <typename MT>
__global__ __launch_bounds__(256) void attloc_context_kernel(FwdP p) {
  __shared__ float red[16];
  __shared__ float part[4][64];
  const int b = blockIdx.y, n = valid_frames(p.hlens, b, p.T);
  const int tid = threadIdx.x, el = tid & 63, tg = tid >> 6;
  const float* e = p.e + (long)b * p.T;
  float mx = -INFINITY;
  for (int t = tid; t < n; t += 256) mx = fmaxf(mx, e[t]);
  mx = block_max(mx, red);
  float sm = 0.f;
  for (int t = tid; t < n; t += 256) sm += expf(SCALING * (e[t] - mx));
  sm = block_sum(sm, red);
  if (blockIdx.x == 0)
    for (int t = tid; t < p.T; t += 256) p.w[(long)b * p.ldw + t] = t < n ? expf(SCALING * (e[t] - mx)) / sm : 0.f;
  const int col = blockIdx.x * 64 + el;
  float acc = 0.f;
  if (col < p.E) {
    const MT* hs = (const MT*)p.hs + (long)b * p.shs + col;
    for (int t = tg; t < n; t += 4) acc += expf(SCALING * (e[t] - mx)) / sm * to_f(hs[(long)t * p.ldhs]);
  }
  part[tg][el] = acc;
  __syncthreads();
  if (tg == 0 && col < p.E) p.c[(long)b * p.ldc + col] = (part[0][el] + part[1][el]) + (part[2][el] + part[3][el]);
}

struct BwdP {
  int B, T, E, A, C, F, nchunk;
  const void* hs; long ldhs, shs;
  const void* pre; long ldpre, spre;
  const long long* hlens;
  const float* dec; long lddec;
  const float* aprev; long ldap;
  const float* w; long ldw;
  const float *K, *M, *g;
  const float* dc; long lddc;
  const float* dwn; long lddwn;
  float* dpre; long lddpre, sdpre;
  float* dhs; long lddhs, sdhs;
  float* ddec; long ldddec;
  float* daprev; long ldda;
  float* part; long ldpart;  // row b: [dM (A*C) | dK (C*(2F+1)) | dg (A) | dg0]
  float* dwbuf;   // (B, T)
  float* conv;    // (B, T, C)
  float* dconv;   // (B, T, C)
  float* dconvp;  // (B, nchunk, T, C)
  float* dap;     // (B, T, C): the channels' parts of daprev
  int lds;        // the units kernel stages M and conv in LDS
};

template <typename MT>
__global__ __launch_bounds__(256) void attloc_bwd_frames_kernel(BwdP p) {
  const int b = blockIdx.y, n = valid_frames(p.hlens, b, p.T);
  const int t0 = blockIdx.x * TF;
  if (t0 >= n) return;
  const int t1 = t0 + TF < n ? t0 + TF : n;
  conv_frames(p.K, p.C, p.F, p.aprev ? p.aprev + (long)b * p.ldap : nullptr, n, t0, t1,
              p.conv + (long)b * p.T * p.C);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* dc = p.dc + (long)b * p.lddc;
  for (int f = 0; f < FW; ++f) {
    const int t = t0 + wave * FW + f;
    if (t >= t1) break;
    const MT* h = (const MT*)p.hs + (long)b * p.shs + (long)t * p.ldhs;
    float* dh = p.dhs + (long)b * p.sdhs + (long)t * p.lddhs;
    const float wt = p.w[(long)b * p.ldw + t];
    float s = 0.f;
    for (int e = lane; e < p.E; e += 64) {
      const float d = dc[e];
      s += to_f(h[e]) * d;
      dh[e] += wt * d;
    }
    s = wave_sum(s);
    if (lane == 0) p.dwbuf[(long)b * p.T + t] = s + (p.dwn ? p.dwn[(long)b * p.lddwn + t] : 0.f);
  }
}

template <typename MT>
__global__ __launch_bounds__(256) void attloc_bwd_units_kernel(BwdP p) {
  __shared__ float red[16];
  __shared__ float tile[TT][AC + 1];
  __shared__ float fin[2][4][AC];
  extern __shared__ float staged[];  // p.lds: the block's AC rows of M, then the tile's TT rows of conv
  const int b = blockIdx.y, n = valid_frames(p.hlens, b, p.T);
  const int tid = threadIdx.x, al = tid & 63, tg = tid >> 6;
  const int a0 = blockIdx.x * AC, a = a0 + al;
  const bool av = a < p.A;
  const int C = p.C;
  const float* w = p.w + (long)b * p.ldw;
  const float* dw = p.dwbuf + (long)b * p.T;
  float* part = p.part + (long)b * p.ldpart;
  const long offK = (long)p.A * C, offg = offK + (long)C * (2 * p.F + 1);
  float d = 0.f;
  for (int t = tid; t < n; t += 256) d += w[t] * dw[t];
  const float dot = block_sum(d, red);  // the same threads in the same order in every block
  if (blockIdx.x == 0) {
    float s = 0.f;
    for (int t = tid; t < n; t += 256) s += SCALING * w[t] * (dw[t] - dot);
    s = block_sum(s, red);
    if (tid == 0) part[offg + p.A] += s;
  }
  const int na = p.A - a0 < AC ? p.A - a0 : AC;
  // the block's rows of M and each tile's rows of conv are read many times: from LDS when they
  // fit (p.lds, the launcher's choice from C), else where they are
  const float* Mc = p.M + (long)a0 * C;
  if (p.lds) {
    for (int i = tid; i < na * C; i += 256) staged[i] = Mc[i];
    Mc = staged;
  }
  const float decv = av ? p.dec[(long)b * p.lddec + a] : 0.f, gv = av ? p.g[a] : 0.f;
  const MT* pre = (const MT*)p.pre + (long)b * p.spre;
  const float* conv = p.conv + (long)b * p.T * C;
  float* dpre = p.dpre + (long)b * p.sdpre;
  float acc_dd = 0.f, acc_dg = 0.f;
  constexpr int FT = TT / 4;  // frames of a tile per thread
  for (int tt0 = 0; tt0 < n; tt0 += TT) {
    const int nt = n - tt0 < TT ? n - tt0 : TT;
    const float* cvt = conv + (long)tt0 * C;
    if (p.lds) {
      float* cv = staged + AC * C;
      for (int i = tid; i < nt * C; i += 256) cv[i] = cvt[i];
      cvt = cv;
    }
    __syncthreads();
    float s[FT] = {};
    if (av) {
      for (int c = 0; c < C; ++c) {
        const float mv = Mc[al * C + c];
#pragma unroll
        for (int f = 0; f < FT; ++f) {
          const int tl = tg + 4 * f < nt ? tg + 4 * f : nt - 1;
          s[f] += mv * cvt[tl * C + c];
        }
      }
    }
#pragma unroll
    for (int f = 0; f < FT; ++f) {
      const int tl = tg + 4 * f, t = tt0 + tl;
      float dp = 0.f;
      if (t < n && av) {
        const float u = tanhf(to_f(pre[(long)t * p.ldpre + a]) + decv + s[f]);
        const float det = SCALING * w[t] * (dw[t] - dot);
        dp = det * gv * (1.f - u * u);
        dpre[(long)t * p.lddpre + a] += dp;
        acc_dd += dp;
        acc_dg += det * u;
      }
      tile[tl][al] = dp;
    }
    __syncthreads();
    // dM[a, c] += sum over the tile's frames (c is uniform over a wave)
    for (int i = tid; i < AC * C; i += 256) {
      const int aa = i & (AC - 1), c = i / AC;
      if (aa < na) {
        float v = 0.f;
#pragma unroll 8
        for (int tl = 0; tl < nt; ++tl) v += tile[tl][aa] * cvt[tl * C + c];
        part[(long)(a0 + aa) * C + c] += v;
      }
    }
    // this unit chunk's part of dconv[t, c]
    for (int i = tid; i < nt * C; i += 256) {
      const int tl = i / C, c = i % C;
      float v = 0.f;
#pragma unroll 8
      for (int aa = 0; aa < na; ++aa) v += tile[tl][aa] * Mc[aa * C + c];
      p.dconvp[(((long)b * p.nchunk + blockIdx.x) * p.T + tt0 + tl) * C + c] = v;
    }
    __syncthreads();
  }
  fin[0][tg][al] = acc_dd;
  fin[1][tg][al] = acc_dg;
  __syncthreads();
  if (tg == 0 && av) {
    p.ddec[(long)b * p.ldddec + a] = (fin[0][0][al] + fin[0][1][al]) + (fin[0][2][al] + fin[0][3][al]);
    part[offg + a] += (fin[1][0][al] + fin[1][1][al]) + (fin[1][2][al] + fin[1][3][al]);
  }
}

__global__ __launch_bounds__(256) void attloc_bwd_dconv_kernel(BwdP p) {
  const int b = blockIdx.y, n = valid_frames(p.hlens, b, p.T);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)n * p.C) return;
  float s = 0.f;
  for (int k = 0; k < p.nchunk; ++k) s += p.dconvp[((long)b * p.nchunk + k) * p.T * p.C + i];
  p.dconv[(long)b * p.T * p.C + i] = s;
}

// one thread per (s, c): channel c's part of daprev[s]; and one per (c, k): the dK partial
__global__ __launch_bounds__(256) void attloc_bwd_loc_kernel(BwdP p) {
  const int b = blockIdx.y, n = valid_frames(p.hlens, b, p.T);
  const int KW = 2 * p.F + 1;
  const long o = (long)blockIdx.x * 256 + threadIdx.x, TC = (long)p.T * p.C;
  const float* dconv = p.dconv + (long)b * TC;
  if (o < TC) {
    const int s = (int)(o / p.C), c = (int)(o % p.C);
    if (!p.daprev || s >= n) return;
    const int j0 = s - p.F > 0 ? s - p.F : 0, j1 = s + p.F < n - 1 ? s + p.F : n - 1;
    const float* kr = p.K + (long)c * KW;
    float v = 0.f;
#pragma unroll 8
    for (int t = j0; t <= j1; ++t) v += dconv[(long)t * p.C + c] * kr[s + p.F - t];
    p.dap[(long)b * TC + o] = v;
    return;
  }
  const long q = o - TC;
  if (q >= (long)p.C * KW || n == 0) return;
  const int c = (int)(q / KW), k = (int)(q % KW);
  // dK[c, k] = sum_t dconv[t, c] aprev[t + k - F], 0 <= t + k - F < n
  const int j0 = p.F - k > 0 ? p.F - k : 0, j1 = n - 1 + p.F - k < n - 1 ? n - 1 + p.F - k : n - 1;
  const float* ap = p.aprev ? p.aprev + (long)b * p.ldap : nullptr;
  const float inv_n = 1.f / (float)n;
  float v = 0.f;
#pragma unroll 8
  for (int t = j0; t <= j1; ++t) v += dconv[(long)t * p.C + c] * (ap ? ap[t + k - p.F] : inv_n);
  p.part[(long)b * p.ldpart + (long)p.A * p.C + q] += v;
}

// daprev[s] = the channels' parts in channel order; 0 for s >= n
__global__ __launch_bounds__(256) void attloc_bwd_daprev_kernel(BwdP p) {
  const int b = blockIdx.y, n = valid_frames(p.hlens, b, p.T);
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= p.T) return;
  float v = 0.f;
  if (s < n) {
    const float* d = p.dap + ((long)b * p.T + s) * p.C;
    for (int c = 0; c < p.C; ++c) v += d[c];
  }
  p.daprev[(long)b * p.ldda + s] = v;
}

bool dims_ok(int mdtype, int B, int T, int E, int A, int C, int F) {
  return (mdtype == EA_F32 || mdtype == EA_BF16) && B >= 0 && B <= 65535 && T >= 1 && E >= 1 && A >= 1 && C >= 1 &&
         F >= 0 && (long)C * (2L * F + 1) < (1L << 30) && (long)T * C < (1L << 30) && (long)A * C < (1L << 30);
}

}  // namespace

extern "C" int ea_attloc_fwd(int mdtype, int B, int T, int E, int A, int C, int F, const void* hs, long ldhs,
                             long shs, const void* pre_enc, long ldpre, long spre, const long long* hlens,
                             const float* dec, long lddec, const float* aprev, long ldap, const float* conv_w,
                             const float* att_w, const float* gvec_w, const float* gvec_b, float* w, long ldw,
                             float* c, long ldc, float* ws, long ws_floats, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(dims_ok(mdtype, B, T, E, A, C, F));
  EA_CHECK_ARG(hs && pre_enc && hlens && dec && conv_w && att_w && gvec_w && gvec_b && w && c && ws);
  // shs = spre = 0: one memory shared by every row (the hypotheses of a beam)
  EA_CHECK_ARG(ldhs >= E && (shs >= (long)T * ldhs || shs == 0) && ldpre >= A &&
               (spre >= (long)T * ldpre || spre == 0) && lddec >= A && ldw >= T && ldc >= E &&
               (!aprev || ldap >= T) && aprev != w);
  EA_CHECK_ARG(ws_floats >= (long)B * T * (1 + C));
  if (B == 0) return 0;
  FwdP p;
  p.B = B; p.T = T; p.E = E; p.A = A; p.C = C; p.F = F;
  p.hs = hs; p.ldhs = ldhs; p.shs = shs; p.pre = pre_enc; p.ldpre = ldpre; p.spre = spre; p.hlens = hlens;
  p.dec = dec; p.lddec = lddec; p.aprev = aprev; p.ldap = ldap;
  p.K = conv_w; p.M = att_w; p.g = gvec_w; p.g0 = gvec_b;
  p.w = w; p.ldw = ldw; p.c = c; p.ldc = ldc;
  p.e = ws; p.conv = ws + (long)B * T;
  hipStream_t st = (hipStream_t)stream;
  const bool bf = mdtype == EA_BF16;
  const dim3 g1(ea_cdiv(T, TF), B), g2(ea_cdiv(E, 64), B);
  if (bf) {
    attloc_score_kernel<bf16><<<g1, 256, 0, st>>>(p);
    attloc_context_kernel<bf16><<<g2, 256, 0, st>>>(p);
  } else {
    attloc_score_kernel<float><<<g1, 256, 0, st>>>(p);
    attloc_context_kernel<float><<<g2, 256, 0, st>>>(p);
  }
  EA_LAUNCH_CHECK();
  return 0;
}

extern "C" int ea_attloc_bwd(int mdtype, int B, int T, int E, int A, int C, int F, const void* hs, long ldhs,
                             long shs, const void* pre_enc, long ldpre, long spre, const long long* hlens,
                             const float* dec, long lddec, const float* aprev, long ldap, const float* w, long ldw,
                             const float* conv_w, const float* att_w, const float* gvec_w, const float* dc,
                             long lddc, const float* dw_next, long lddwn, float* dpre, long lddpre, long sdpre,
                             float* dhs, long lddhs, long sdhs, float* ddec, long ldddec, float* daprev, long ldda,
                             float* part, long ldpart, float* ws, long ws_floats, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(dims_ok(mdtype, B, T, E, A, C, F));
  EA_CHECK_ARG(hs && pre_enc && hlens && dec && w && conv_w && att_w && gvec_w && dc && dpre && dhs && ddec &&
               part && ws);
  EA_CHECK_ARG(ldhs >= E && shs >= (long)T * ldhs && ldpre >= A && spre >= (long)T * ldpre && lddec >= A &&
               ldw >= T && (!aprev || ldap >= T) && lddc >= E && (!dw_next || lddwn >= T));
  EA_CHECK_ARG(lddpre >= A && sdpre >= (long)T * lddpre && lddhs >= E && sdhs >= (long)T * lddhs && ldddec >= A &&
               (!daprev || ldda >= T) && ldpart >= (long)A * C + (long)C * (2L * F + 1) + A + 1);
  EA_CHECK_ARG(daprev != dw_next || !daprev);
  EA_CHECK_ARG((const void*)dhs != hs && (const void*)dpre != pre_enc && (!daprev || (daprev != w && daprev != aprev)));
  const int nchunk = ea_cdiv(A, AC);
  EA_CHECK_ARG(ws_floats >= (long)B * T * (1 + (3L + nchunk) * C));
  if (B == 0) return 0;
  BwdP p;
  p.B = B; p.T = T; p.E = E; p.A = A; p.C = C; p.F = F; p.nchunk = nchunk;
  p.hs = hs; p.ldhs = ldhs; p.shs = shs; p.pre = pre_enc; p.ldpre = ldpre; p.spre = spre; p.hlens = hlens;
  p.dec = dec; p.lddec = lddec; p.aprev = aprev; p.ldap = ldap; p.w = w; p.ldw = ldw;
  p.K = conv_w; p.M = att_w; p.g = gvec_w; p.dc = dc; p.lddc = lddc; p.dwn = dw_next; p.lddwn = lddwn;
  p.dpre = dpre; p.lddpre = lddpre; p.sdpre = sdpre; p.dhs = dhs; p.lddhs = lddhs; p.sdhs = sdhs;
  p.ddec = ddec; p.ldddec = ldddec; p.daprev = daprev; p.ldda = ldda; p.part = part; p.ldpart = ldpart;
  const long BT = (long)B * T;
  p.dwbuf = ws; p.conv = ws + BT; p.dconv = p.conv + BT * C; p.dap = p.dconv + BT * C; p.dconvp = p.dap + BT * C;
  // the units kernel's staged rows: (AC + TT) * C floats beside its 11 KB of static LDS
  const size_t stage = (size_t)(AC + TT) * C * sizeof(float);
  p.lds = stage <= 32768;
  const size_t dyn = p.lds ? stage : 0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 g1(ea_cdiv(T, TF), B), g2(nchunk, B), g3(ea_cdiv((long)T * C, 256), B),
      g4(ea_cdiv((long)T * C + (long)C * (2L * F + 1), 256), B), g5(ea_cdiv(T, 256), B);
  if (mdtype == EA_BF16) {
    attloc_bwd_frames_kernel<bf16><<<g1, 256, 0, st>>>(p);
    attloc_bwd_units_kernel<bf16><<<g2, 256, dyn, st>>>(p);
  } else {
    attloc_bwd_frames_kernel<float><<<g1, 256, 0, st>>>(p);
    attloc_bwd_units_kernel<float><<<g2, 256, dyn, st>>>(p);
  }
  attloc_bwd_dconv_kernel<<<g3, 256, 0, st>>>(p);
  attloc_bwd_loc_kernel<<<g4, 256, 0, st>>>(p);
  if (daprev) attloc_bwd_daprev_kernel<<<g5, 256, 0, st>>>(p);
  EA_LAUNCH_CHECK();
  return 0;
}
