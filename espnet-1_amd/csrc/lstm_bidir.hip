// The recurrence of the BLSTM(P) encoder (torch.nn.LSTM on a pack_padded_sequence inside
// espnet/nets/pytorch_backend/rnn/encoders.py, unrolled over time by the host):
// ea_lstm_bicell_fwd and ea_lstm_bicell_bwd, ONE launch per time step for both directions.
//
// A block is a block of lstm_train.hip's kernels: the same block product on the same tiles, the
// same cell epilogue (lstm_core.h).  Two things are added.
//   grid.z   the direction.  Each direction has its own operand block (pack, xproj, states, gates
//            and its own time index t); the block of direction z offsets every pointer by t
//            steps and then knows nothing of the other direction: they share no written memory
//            and no block waits for another.  Two directions double the blocks of a launch
//            (80 -> 160 at H = 320, 128 -> 256 at H = 1024, on 256 CUs) and halve the launches.
//   lens     row r is active iff t < lens[r], read from device memory in the epilogue.  An
//            inactive row stores zeros where an active one stores its update.  That alone is the
//            packed-sequence recurrence (include/espnet_amd.h, ea_lstm_bicell_fwd): the host
//            never needs the lengths, so a captured step replays for any lengths.
// Inactive rows still ride through the block product (their operands are valid memory: zeros the
// mask wrote, or the initial slot); skipping them would save no weight traffic.
//
// ea_tanh_fwd / ea_tanh_bwd: the activation after the encoder's projections.
#include "lstm_core.h"

namespace {

using namespace lstm_core;

// one direction's operand block (include/espnet_amd.h: EA_BIF_* / EA_BIB_*)
struct DirFwd {
  const void* wpack;
  const float* xproj;
  const void* h_prev;
  const float* c_prev;
  float* h_out;
  float* c_out;
  void* hb_out;
  float* gates;
  long ldx, sx, lds, ss, ldg, sg;
  int t;
};
struct DirBwd {
  const void* wpack_t;
  const void* dgates_next;
  const float* dh_out;
  const float* gates;
  const float* c;
  const float* c_prev;
  const float* dc_in;
  float* dc_out;
  float* dgates;
  void* dgates_b;
  long ldd, sd, lddh, sdh, ldg, sg, ldc, sc, lddc, sdc;
  int t, first;
};

struct LenMask {
  const long long* lens;
  int t;
  EA_DEV bool operator()(int row) const { return (long long)t < lens[row]; }
};

// ------------------------------------------------------------------ forward
struct BiFwdP {
  int n, H, Hp;
  const long long* lens;
  DirFwd d[2];
  int hvec[2];
};

template <bool BF, int MT, int NJ, int U>
__global__ __launch_bounds__(64 * NW) void lstm_bicell_fwd_kernel(BiFwdP p) {
  typedef typename Frag<BF>::W WT;
  __shared__ __attribute__((aligned(16))) float red[NW / 2][16 * MT][16 * NJ + 4];
  const int r0 = blockIdx.y * 16 * MT, t0 = blockIdx.x * NJ;
  const DirFwd& d = p.d[blockIdx.z];
  const long t = d.t, ld = d.lds;
  const WT* hp = (const WT*)d.h_prev + t * d.ss;
  const float* cp = d.c_prev + t * d.ss;
  const float* xproj = d.xproj + t * d.sx;
  const int H = p.H;

  RowsA<BF, MT, WT> a;
  a.lim = H; a.vec = p.hvec[blockIdx.z];
#pragma unroll
  for (int i = 0; i < MT; ++i) a.row[i] = hp + (long)lane_row(r0, i, p.n) * ld;
  block_product<BF, MT, NJ, U>(a, d.wpack, p.Hp / (BF ? 32 : 16), t0, (H + 3) / 4, red);

  const long ldx = d.ldx;
  cell_fwd_epilogue<MT, NJ>(
      red, r0, t0, p.n, H,
      [&](int row, int unit) {
        const float* xp = xproj + (long)row * ldx + unit;  // torch gate order: column gate * H + unit
        return make_float4(xp[0], xp[H], xp[2 * (long)H], xp[3 * (long)H]);
      },
      [&](int row, int unit) { return cp[(long)row * ld + unit]; }, d.h_out + t * d.ss, d.c_out + t * d.ss,
      d.hb_out ? (bf16*)d.hb_out + t * d.ss : nullptr, ld, d.gates + t * d.sg, d.ldg, LenMask{p.lens, d.t});
}

// ------------------------------------------------------------------ backward
struct BiBwdP {
  int n, H;
  const long long* lens;
  DirBwd d[2];
  int avec[2];
};

// one direction's step in the field names of lstm_core.h's cell_bwd_epilogue
struct BwdStep {
  int n, H, G;
  const float* dho;
  long lddh;
  const float* gates;
  long ldg;
  const float* c;
  const float* cprev;
  long ldc;
  const float* dci;
  float* dco;
  long lddc;
  float* dg;
  bf16* dgb;
  long ldd;
  float* dht;
  long ldt;
};

template <bool BF, int MT, int U>
__global__ __launch_bounds__(64 * NW) void lstm_bicell_bwd_kernel(BiBwdP p) {
  typedef typename Frag<BF>::W WT;
  __shared__ __attribute__((aligned(16))) float red[NW / 2][16 * MT][16 + 4];
  const int r0 = blockIdx.y * 16 * MT, t0 = blockIdx.x;
  const DirBwd& d = p.d[blockIdx.z];
  const long t = d.t;
  const bool rec = !d.first;  // uniform over the direction's blocks

  BwdStep s;
  s.n = p.n; s.H = p.H; s.G = 4 * p.H;
  s.dho = d.dh_out ? d.dh_out + t * d.sdh : nullptr; s.lddh = d.lddh;
  s.gates = d.gates + t * d.sg; s.ldg = d.ldg;
  s.c = d.c + t * d.sc; s.cprev = d.c_prev + t * d.sc; s.ldc = d.ldc;
  s.dci = rec ? d.dc_in + t * d.sdc : nullptr;
  s.dco = d.dc_out + t * d.sdc; s.lddc = d.lddc;
  s.dg = d.dgates + t * d.sd;
  s.dgb = d.dgates_b ? (bf16*)d.dgates_b + t * d.sd : nullptr;
  s.ldd = d.ldd;
  s.dht = nullptr; s.ldt = 0;

  if (rec) {
    RowsA<BF, MT, WT> a;
    a.lim = s.G; a.vec = p.avec[blockIdx.z];
    const WT* dgn = (const WT*)d.dgates_next + t * d.sd;
#pragma unroll
    for (int i = 0; i < MT; ++i) a.row[i] = dgn + (long)lane_row(r0, i, p.n) * d.ldd;
    const int Gp = (s.G + EA_LSTM_KG - 1) / EA_LSTM_KG * EA_LSTM_KG;
    block_product<BF, MT, 1, U>(a, d.wpack_t, Gp / (BF ? 32 : 16), t0, (p.H + 15) / 16, red);
  }
  cell_bwd_epilogue<MT>(red, rec, r0, t0, s, LenMask{p.lens, d.t});
}

// ------------------------------------------------------------------ tanh
__global__ void tanh_fwd_kernel(long n, const float* __restrict__ x, float* __restrict__ y) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    y[i] = tanhf(x[i]);
}
__global__ void tanh_bwd_kernel(long n, const float* __restrict__ y, const float* dy, float* dx) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = y[i];
    dx[i] = dy[i] * (1.f - v * v);
  }
}

}  // namespace

extern "C" int ea_lstm_bicell_fwd(int wdtype, int ndir, int n, int H, const long long* lens,
                                  const void* const* ptrs, const long* strides, const int* t, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG((wdtype == EA_F32 || wdtype == EA_BF16) && (ndir == 1 || ndir == 2) && n >= 0 && H >= 1);
  EA_CHECK_ARG(lens && ptrs && strides && t);
  DirFwd dirs[2];
  for (int z = 0; z < ndir; ++z) {
    const void* const* q = ptrs + z * EA_BIF_NPTR;
    const long* s = strides + z * EA_BIF_NSTR;
    DirFwd& d = dirs[z];
    d.wpack = q[EA_BIF_WPACK]; d.xproj = (const float*)q[EA_BIF_XPROJ]; d.h_prev = q[EA_BIF_H_PREV];
    d.c_prev = (const float*)q[EA_BIF_C_PREV]; d.h_out = (float*)q[EA_BIF_H_OUT]; d.c_out = (float*)q[EA_BIF_C_OUT];
    d.hb_out = (void*)q[EA_BIF_HB_OUT]; d.gates = (float*)q[EA_BIF_GATES];
    d.ldx = s[EA_BIF_LDX]; d.sx = s[EA_BIF_SX]; d.lds = s[EA_BIF_LDS]; d.ss = s[EA_BIF_SS];
    d.ldg = s[EA_BIF_LDG]; d.sg = s[EA_BIF_SG]; d.t = t[z];
  }
  const bool bf = wdtype == EA_BF16;
  BiFwdP p;
  p.n = n; p.H = H; p.lens = lens;
  p.Hp = ea_cdiv(H, EA_LSTM_KG) * EA_LSTM_KG;
  for (int z = 0; z < 2; ++z) {
    const DirFwd& d = dirs[z < ndir ? z : 0];
    EA_CHECK_ARG(d.wpack && d.xproj && d.h_prev && d.c_prev && d.h_out && d.c_out && d.gates && aligned16(d.wpack));
    EA_CHECK_ARG(d.t >= 0 && d.ldx >= 4L * H && d.lds >= H && d.ldg >= 4L * H && d.ldg % 4 == 0 && d.sg % 4 == 0 &&
                 aligned16(d.gates));
    EA_CHECK_ARG(!bf || d.hb_out);  // the bf16 path's next h_prev
    EA_CHECK_ARG((const void*)d.h_out != d.h_prev && d.c_out != d.c_prev);
    p.d[z] = d;
    const int q = bf ? 8 : 4;
    p.hvec[z] = aligned16(d.h_prev) && d.lds % q == 0 && d.ss % q == 0;
  }
  if (ndir == 2) {  // the directions never touch each other's memory
    const DirFwd &a = dirs[0], &b = dirs[1];
    EA_CHECK_ARG(a.h_out != b.h_out && a.c_out != b.c_out && a.gates != b.gates && (!a.hb_out || a.hb_out != b.hb_out));
  }
  if (n == 0) return 0;
  const int ntiles = (H + 3) / 4;
  return launch_tiles(
      n, ntiles, ntiles >= 256, p, (hipStream_t)stream,
      [bf](auto mt, auto nj, auto u) {
        return bf ? lstm_bicell_fwd_kernel<true, mt(), nj(), u()> : lstm_bicell_fwd_kernel<false, mt(), nj(), u()>;
      },
      ndir);
}

extern "C" int ea_lstm_bicell_bwd(int wdtype, int ndir, int n, int H, const long long* lens,
                                  const void* const* ptrs, const long* strides, const int* t, const int* first,
                                  void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG((wdtype == EA_F32 || wdtype == EA_BF16) && (ndir == 1 || ndir == 2) && n >= 0 && H >= 1);
  EA_CHECK_ARG(lens && ptrs && strides && t && first);
  DirBwd dirs[2];
  for (int z = 0; z < ndir; ++z) {
    const void* const* q = ptrs + z * EA_BIB_NPTR;
    const long* s = strides + z * EA_BIB_NSTR;
    DirBwd& d = dirs[z];
    d.wpack_t = q[EA_BIB_WPACK_T]; d.dgates_next = q[EA_BIB_DGATES_NEXT]; d.dh_out = (const float*)q[EA_BIB_DH_OUT];
    d.gates = (const float*)q[EA_BIB_GATES]; d.c = (const float*)q[EA_BIB_C]; d.c_prev = (const float*)q[EA_BIB_C_PREV];
    d.dc_in = (const float*)q[EA_BIB_DC_IN]; d.dc_out = (float*)q[EA_BIB_DC_OUT]; d.dgates = (float*)q[EA_BIB_DGATES];
    d.dgates_b = (void*)q[EA_BIB_DGATES_B];
    d.ldd = s[EA_BIB_LDD]; d.sd = s[EA_BIB_SD]; d.lddh = s[EA_BIB_LDDH]; d.sdh = s[EA_BIB_SDH];
    d.ldg = s[EA_BIB_LDG]; d.sg = s[EA_BIB_SG]; d.ldc = s[EA_BIB_LDC]; d.sc = s[EA_BIB_SC];
    d.lddc = s[EA_BIB_LDDC]; d.sdc = s[EA_BIB_SDC]; d.t = t[z]; d.first = first[z];
  }
  const bool bf = wdtype == EA_BF16;
  BiBwdP p;
  p.n = n; p.H = H; p.lens = lens;
  for (int z = 0; z < 2; ++z) {
    const DirBwd& d = dirs[z < ndir ? z : 0];
    EA_CHECK_ARG(d.wpack_t && d.gates && d.c && d.c_prev && d.dc_out && d.dgates && aligned16(d.wpack_t) &&
                 aligned16(d.gates));
    EA_CHECK_ARG(d.t >= 0 && d.ldg >= 4L * H && d.ldg % 4 == 0 && d.sg % 4 == 0 && d.ldc >= H && d.lddc >= H &&
                 d.ldd >= 4L * H && (!d.dh_out || d.lddh >= H));
    EA_CHECK_ARG(d.first || (d.dgates_next && d.dc_in));
    EA_CHECK_ARG(!bf || d.dgates_b);  // the bf16 path's next dgates_next
    EA_CHECK_ARG(d.dc_in != d.dc_out && d.dgates_next != (const void*)d.dgates &&
                 (!d.dgates_b || d.dgates_next != d.dgates_b));
    p.d[z] = d;
    const int q = bf ? 8 : 4;
    p.avec[z] = d.dgates_next && aligned16(d.dgates_next) && d.ldd % q == 0 && d.sd % q == 0;
  }
  if (ndir == 2) {
    const DirBwd &a = dirs[0], &b = dirs[1];
    EA_CHECK_ARG(a.dgates != b.dgates && a.dc_out != b.dc_out && (!a.dgates_b || a.dgates_b != b.dgates_b));
  }
  if (n == 0) return 0;
  return launch_tiles(
      n, ea_cdiv(H, 16), false, p, (hipStream_t)stream,
      [bf](auto mt, auto, auto u) {
        return bf ? lstm_bicell_bwd_kernel<true, mt(), u()> : lstm_bicell_bwd_kernel<false, mt(), u()>;
      },
      ndir);
}

extern "C" int ea_tanh_fwd(long n, const float* x, float* y, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(n >= 0 && (n == 0 || (x && y)));
  if (n == 0) return 0;
  hipLaunchKernelGGL(tanh_fwd_kernel, dim3(ea_grid_cap(ea_cdiv(n, 256))), dim3(256), 0, (hipStream_t)stream, n, x, y);
  EA_LAUNCH_CHECK();
  return 0;
}

extern "C" int ea_tanh_bwd(long n, const float* y, const float* dy, float* dx, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG(n >= 0 && (n == 0 || (y && dy && dx)));
  if (n == 0) return 0;
  hipLaunchKernelGGL(tanh_bwd_kernel, dim3(ea_grid_cap(ea_cdiv(n, 256))), dim3(256), 0, (hipStream_t)stream, n, y, dy,
                     dx);
  EA_LAUNCH_CHECK();
  return 0;
}
