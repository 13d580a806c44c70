// Fused LSTM step (ea_lstm_step): one launch per layer per decoding step of SequentialRNNLM
// (espnet2/lm/seq_rnn_lm.py: torch.nn.LSTM over one token of every running hypothesis).
//
//   gates = x . W_ih^T + h_prev[src] . W_hh^T + (b_ih + b_hh)        (n, 4H), never leaves the block
//   c'    = sigmoid(f) * c_prev[src] + sigmoid(i) * tanh(g)
//   h'    = sigmoid(o) * tanh(c')
//
// n is the number of running hypotheses (a few dozen at most), so the launch is a weight
// stream: 4H x (I + H) elements read once.  The product and the cell update are lstm_core.h's;
// this file adds the step's operands: K = [x | h_prev] (x a row of the embedding table by token
// id for layer 0), the parent gather of h_prev / c_prev by `src`, the bias.
#include "lstm_core.h"

namespace {

using namespace lstm_core;

struct LstmP {
  int n, I, H, Ip, Hp, n_prev, V;
  const void* w;
  const float* bias;
  const float* x;
  long ldx;
  const long long* tok;
  long ldtok;
  const float* hp;
  const float* cp;
  long ldp;
  const int* src;
  float* ho;
  float* co;
  long ldo;
  bf16* hb;
  int xvec, hvec;
};

// the parent row of hypothesis `row` (indices outside [0, n_prev) are clamped)
EA_DEV int parent_row(const LstmP& p, int row) {
  if (!p.src) return row;
  const int sr = p.src[row];
  return sr < 0 ? 0 : (sr >= p.n_prev ? p.n_prev - 1 : sr);
}

// MT 16-row tiles of hypotheses x NJ 16-row weight tiles per block; U slices per wave in flight
// (BF = bf16 pack; a bool so that profilers print the instantiation's name legibly)
template <bool BF, int MT, int NJ, int U>
__global__ __launch_bounds__(64 * NW) void lstm_step_kernel(LstmP p) {
  constexpr int SL = BF ? 32 : 16;
  __shared__ __attribute__((aligned(16))) float red[NW / 2][16 * MT][16 * NJ + 4];
  const int r0 = blockIdx.y * 16 * MT, t0 = blockIdx.x * NJ;

  RowsXH<BF, MT> a;
  a.nkx = p.Ip / SL; a.I = p.I; a.H = p.H; a.xvec = p.xvec; a.hvec = p.hvec;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int rr = lane_row(r0, i, p.n);
    long xi = rr;
    if (p.tok) {
      const long long t = p.tok[rr * p.ldtok];
      xi = t < 0 ? 0 : (t >= p.V ? p.V - 1 : t);
    }
    a.x[i] = p.x + xi * p.ldx;
    a.h[i] = p.hp + (long)parent_row(p, rr) * p.ldp;
  }
  block_product<BF, MT, NJ, U>(a, p.w, (p.Ip + p.Hp) / SL, t0, (p.H + 3) / 4, red);

  cell_fwd_epilogue<MT, NJ>(
      red, r0, t0, p.n, p.H, [&](int, int unit) { return *(const float4*)(p.bias + 4 * (long)unit); },
      [&](int row, int unit) { return p.cp[(long)parent_row(p, row) * p.ldp + unit]; }, p.ho, p.co, p.hb, p.ldo,
      nullptr, 0);
}

}  // namespace

extern "C" int ea_lstm_step(int wdtype, int n, int I, int H, const void* wpack, const float* bias, const float* x,
                            long ldx, const long long* tok, long ldtok, int V, const float* h_prev, const float* c_prev,
                            long ldp, int n_prev, const int* src, float* h_out, float* c_out, long ldo,
                            void* hb_out, void* stream) {
  EA_ENTRY();
  EA_CHECK_ARG((wdtype == EA_F32 || wdtype == EA_BF16) && n >= 0 && I >= 1 && H >= 1);
  EA_CHECK_ARG(wpack && bias && x && h_prev && c_prev && h_out && c_out && aligned16(wpack) && aligned16(bias));
  EA_CHECK_ARG(ldx >= I && ldp >= H && ldo >= H && n_prev >= 1 && (src || n_prev >= n) && (!tok || V >= 1));
  EA_CHECK_ARG(h_out != h_prev && c_out != c_prev && h_out != c_prev && c_out != h_prev);
  if (n == 0) return 0;
  LstmP p;
  p.n = n; p.I = I; p.H = H; p.n_prev = n_prev; p.V = V;
  p.Ip = ea_cdiv(I, EA_LSTM_KG) * EA_LSTM_KG;
  p.Hp = ea_cdiv(H, EA_LSTM_KG) * EA_LSTM_KG;
  p.w = wpack; p.bias = bias; p.x = x; p.ldx = ldx; p.tok = tok; p.ldtok = ldtok;
  p.hp = h_prev; p.cp = c_prev; p.ldp = ldp; p.src = src;
  p.ho = h_out; p.co = c_out; p.ldo = ldo; p.hb = (bf16*)hb_out;
  p.xvec = aligned16(x) && ldx % 4 == 0;
  p.hvec = aligned16(h_prev) && ldp % 4 == 0;
  // two tiles per block from H = 1024 up (>= 128 blocks): halves the blocks' re-reads of x / h,
  // which bound the wide launches (measured against one tile per block)
  const int ntiles = (H + 3) / 4;
  const bool bf = wdtype == EA_BF16;
  return launch_tiles(n, ntiles, ntiles >= 256, p, (hipStream_t)stream, [bf](auto mt, auto nj, auto u) {
    return bf ? lstm_step_kernel<true, mt(), nj(), u()> : lstm_step_kernel<false, mt(), nj(), u()>;
  });
}
