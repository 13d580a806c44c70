// LSTM training steps of SequentialRNNLM (torch.nn.LSTM inside espnet2/lm/seq_rnn_lm.py:92-104,
// unrolled over time by the host): ea_lstm_cell_fwd and ea_lstm_cell_bwd, one plain launch per
// time step per layer.  The input projection of all time steps (X . W_ih^T + b_ih + b_hh) and
// every product of the backward that is not recurrent (dW_hh, dW_ih, dX, the bias sums) are
// ordinary GEMMs / column sums over all T * B rows; only the recurrence is here.
//
//   forward   gates = xproj[t] + h_{t-1} . W_hh^T                    K = Hp, N = 4H
//             c_t = sigmoid(f) c_{t-1} + sigmoid(i) tanh(g);  h_t = sigmoid(o) tanh(c_t)
//             writes h_t, c_t, the four ACTIVATED gates (the backward never recomputes them)
//             and, for the bf16 path, a bf16 h_t (the next step's and the dW_hh GEMM's operand)
//   backward  dh = dh_out[t] + dgates[t+1] . W_hh                    K = 4H (padded), N = H
//             then the cell's gradient on the block's own hidden units (see ea_lstm_cell_bwd in
//             include/espnet_amd.h); the first launch (t = T - 1) has no dgates[t+1] and skips
//             the product.
//
// Both run on lstm_core.h's block product with B a training batch.  The forward's column tile
// is 4 hidden units x 4 gates (so the cell update is local to the tile and is the decoding
// step's), the backward's is 16 hidden units with the cell-gradient epilogue (both epilogues are
// lstm_core.h's, shared with lstm_bidir.hip).  The time loop is the host's.
#include "lstm_core.h"

namespace {

using namespace lstm_core;

// ------------------------------------------------------------------ forward
struct CellFwdP {
  int n, H, Hp;
  const void* w;
  const float* xproj;
  long ldx;
  const void* hp;  // f32, or bf16 with the bf16 pack
  const float* cp;
  long ldp;
  float* ho;
  float* co;
  long ldo;
  bf16* hb;
  float* gates;
  long ldg;
  int hvec;
};

template <bool BF, int MT, int NJ, int U>
__global__ __launch_bounds__(64 * NW) void lstm_cell_fwd_kernel(CellFwdP p) {
  typedef typename Frag<BF>::W WT;
  __shared__ __attribute__((aligned(16))) float red[NW / 2][16 * MT][16 * NJ + 4];
  const int r0 = blockIdx.y * 16 * MT, t0 = blockIdx.x * NJ;

  RowsA<BF, MT, WT> a;
  a.lim = p.H; a.vec = p.hvec;
#pragma unroll
  for (int i = 0; i < MT; ++i) a.row[i] = (const WT*)p.hp + (long)lane_row(r0, i, p.n) * p.ldp;
  block_product<BF, MT, NJ, U>(a, p.w, p.Hp / (BF ? 32 : 16), t0, (p.H + 3) / 4, red);

  cell_fwd_epilogue<MT, NJ>(
      red, r0, t0, p.n, p.H,
      [&](int row, int unit) {
        const float* xp = p.xproj + (long)row * p.ldx + unit;  // torch gate order: column gate * H + unit
        return make_float4(xp[0], xp[p.H], xp[2 * (long)p.H], xp[3 * (long)p.H]);
      },
      [&](int row, int unit) { return p.cp[(long)row * p.ldp + unit]; }, p.ho, p.co, p.hb, p.ldo, p.gates, p.ldg);
}

// ------------------------------------------------------------------ backward
struct CellBwdP {
  int n, H, G;  // G = 4H
  const void* wt;
  const void* dgn;  // dgates[t+1]: f32, or bf16 with the bf16 pack; NULL on the first launch
  long lddn;
  int avec;
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
__global__ __launch_bounds__(64 * NW) void lstm_cell_bwd_kernel(CellBwdP p) {
  typedef typename Frag<BF>::W WT;
  __shared__ __attribute__((aligned(16))) float red[NW / 2][16 * MT][16 + 4];
  const int r0 = blockIdx.y * 16 * MT, t0 = blockIdx.x;
  const bool rec = p.dgn != nullptr;  // uniform over the launch

  if (rec) {
    RowsA<BF, MT, WT> a;
    a.lim = p.G; a.vec = p.avec;
#pragma unroll
    for (int i = 0; i < MT; ++i) a.row[i] = (const WT*)p.dgn + (long)lane_row(r0, i, p.n) * p.lddn;
    const int Gp = (p.G + EA_LSTM_KG - 1) / EA_LSTM_KG * EA_LSTM_KG;
    block_product<BF, MT, 1, U>(a, p.wt, Gp / (BF ? 32 : 16), t0, (p.H + 15) / 16, red);
  }

  cell_bwd_epilogue<MT>(red, rec, r0, t0, p, AllRows{});
}

}  // namespace

extern "C" int ea_lstm_cell_fwd(int wdtype, int n, int H, const void* wpack, const float* xproj, long ldx,
                                const void* h_prev, const float* c_prev, long ldp, float* h_out, float* c_out,
                                long ldo, void* hb_out, float* gates, long ldg, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG((wdtype == EA_F32 || wdtype == EA_BF16) && n >= 0 && H >= 1);
  EA_CHECK_ARG(wpack && xproj && h_prev && c_prev && h_out && c_out && gates && aligned16(wpack));
  EA_CHECK_ARG(ldx >= 4L * H && ldp >= H && ldo >= H && ldg >= 4L * H && ldg % 4 == 0 && aligned16(gates));
  EA_CHECK_ARG(wdtype == EA_F32 || hb_out);  // the bf16 path's next h_prev
  EA_CHECK_ARG((const void*)h_out != h_prev && c_out != c_prev && (const void*)h_out != (const void*)c_prev &&
               (const void*)c_out != h_prev && (!hb_out || (hb_out != h_prev && hb_out != (const void*)c_prev)));
  if (n == 0) return 0;
  CellFwdP p;
  p.n = n; p.H = H;
  p.Hp = ea_cdiv(H, EA_LSTM_KG) * EA_LSTM_KG;
  p.w = wpack; p.xproj = xproj; p.ldx = ldx; p.hp = h_prev; p.cp = c_prev; p.ldp = ldp;
  p.ho = h_out; p.co = c_out; p.ldo = ldo; p.hb = (bf16*)hb_out; p.gates = gates; p.ldg = ldg;
  p.hvec = aligned16(h_prev) && ldp % (wdtype == EA_BF16 ? 8 : 4) == 0;
  // a training batch fills 64-row blocks; the narrow row tiles serve B < 64 (the last batch of
  // an epoch, validation).  Two column tiles per block from H = 1024 up, as ea_lstm_step does.
  const int ntiles = (H + 3) / 4;
  const bool bf = wdtype == EA_BF16;
  return launch_tiles(n, ntiles, ntiles >= 256, p, (hipStream_t)stream, [bf](auto mt, auto nj, auto u) {
    return bf ? lstm_cell_fwd_kernel<true, mt(), nj(), u()> : lstm_cell_fwd_kernel<false, mt(), nj(), u()>;
  });
}

extern "C" int ea_lstm_cell_bwd(int wdtype, int n, int H, const void* wpack_t, const void* dgates_next, long lddn,
                                const float* dh_out, long lddh, const float* gates, long ldg, const float* c,
                                const float* c_prev, long ldc, const float* dc_in, float* dc_out, long lddc,
                                float* dgates, void* dgates_b, long ldd, float* dh_tot, long ldt, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG((wdtype == EA_F32 || wdtype == EA_BF16) && n >= 0 && H >= 1);
  EA_CHECK_ARG(wpack_t && gates && c && c_prev && dc_out && dgates && aligned16(wpack_t) && aligned16(gates));
  EA_CHECK_ARG(ldg >= 4L * H && ldg % 4 == 0 && ldc >= H && lddc >= H && ldd >= 4L * H);
  EA_CHECK_ARG((!dgates_next || lddn >= 4L * H) && (!dh_out || lddh >= H) && (!dh_tot || ldt >= H));
  EA_CHECK_ARG(wdtype == EA_F32 || dgates_b);  // the bf16 path's next dgates_next
  EA_CHECK_ARG(dc_in != dc_out && dgates_next != (const void*)dgates && (!dgates_b || dgates_next != dgates_b));
  EA_CHECK_ARG(dh_tot != dh_out || !dh_tot);
  if (n == 0) return 0;
  CellBwdP p;
  p.n = n; p.H = H; p.G = 4 * H;
  p.wt = wpack_t; p.dgn = dgates_next; p.lddn = lddn;
  p.avec = dgates_next && aligned16(dgates_next) && lddn % (wdtype == EA_BF16 ? 8 : 4) == 0;
  p.dho = dh_out; p.lddh = lddh; p.gates = gates; p.ldg = ldg; p.c = c; p.cprev = c_prev; p.ldc = ldc;
  p.dci = dc_in; p.dco = dc_out; p.lddc = lddc; p.dg = dgates; p.dgb = (bf16*)dgates_b; p.ldd = ldd;
  p.dht = dh_tot; p.ldt = ldt;
  const bool bf = wdtype == EA_BF16;
  return launch_tiles(n, ea_cdiv(H, 16), false, p, (hipStream_t)stream, [bf](auto mt, auto, auto u) {
    return bf ? lstm_cell_bwd_kernel<true, mt(), u()> : lstm_cell_bwd_kernel<false, mt(), u()>;
  });
}
