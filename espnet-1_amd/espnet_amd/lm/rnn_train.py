"""Training path of SequentialRNNLM: the autograd nodes (embedding, dropout, one node per LSTM layer, the output Linear, the loss).

Rows are time-major inside the path (row t * B + b), so the slice of one time step is a
contiguous (B, .) block for ea_lstm_cell_fwd / ea_lstm_cell_bwd and every product that is not
recurrent is ONE GEMM over all T * B rows.  Activations between the nodes are f32; under amp a
node rounds its matrix operands to bf16 (the arena's bf16 shadow for the weights), the states,
the gates, the cell update and every gradient stay f32.  Parameter gradients are accumulated
into the arena's gradient views (Parameter.grad), as every other node of the package does.
"""
from __future__ import annotations

import torch

from .. import hip_ops as ops
from .._lib import BF16, F32, lib
from .lstm_pack import rup

EMBED_BWD_ROWS = 4096  # ea_embed_bwd stages the ids of one call in LDS


def _f32c(t: torch.Tensor) -> torch.Tensor:
    """An f32 gradient with unit inner stride."""
    if t.dtype != torch.float32:
        raise RuntimeError("gradients between the LM's nodes are float32")
    return t if t.stride(-1) == 1 else t.contiguous()


class EmbedFn(torch.autograd.Function):
    """rows of encoder.weight by token id -> (rows, ninp) f32.  The row of padding_idx receives
    no gradient (torch.nn.Embedding(padding_idx=...))."""

    @staticmethod
    def forward(ctx, anchor, tok, lm):
        rows, d = tok.numel(), lm.ninp
        x = torch.empty(rows, d, device=tok.device)
        lib.ea_embed_fwd(rows, d, 1, tok.data_ptr(), lm.encoder.weight.data_ptr(), 1.0, lm._pe0.data_ptr(), 0.0, 0,
                         x.data_ptr(), ops.stream())
        ctx.save = (tok, lm)
        return x

    @staticmethod
    def backward(ctx, dx):
        tok, lm = ctx.save
        ctx.save = None
        dx = _f32c(dx).contiguous()
        rows, d = tok.numel(), lm.ninp
        dE = lm.encoder.weight.grad
        # ea_embed_bwd sums the rows of one token in increasing order inside a call; the calls
        # are stream ordered, so the result does not depend on anything but the batch
        for r0 in range(0, rows, EMBED_BWD_ROWS):
            n = min(EMBED_BWD_ROWS, rows - r0)
            lib.ea_embed_bwd(n, d, tok[r0:].data_ptr(), dx[r0:].data_ptr(), 1.0, 0.0, 0, dE.data_ptr(), ops.stream())
        pad = lm.encoder.padding_idx
        if pad is not None:
            dE[pad].zero_()
        return None, None, None


class DropFn(torch.autograd.Function):
    """y = dropout(x) on ea_scale_dropout's counter-based mask of `seed` (element index
    row * cols + col); the backward draws the same mask."""

    @staticmethod
    def forward(ctx, x, p, seed):
        rows, cols, _ = ops._rows(x)
        y = torch.empty(rows, cols, device=x.device)
        ops.scale_dropout(x, y, p=p, seed=seed)
        ctx.ps = (p, seed)
        return y

    @staticmethod
    def backward(ctx, dy):
        p, seed = ctx.ps
        dy = _f32c(dy)
        dx = torch.empty(dy.shape, device=dy.device)
        ops.scale_dropout(dy, dx, p=p, seed=seed)
        return dx, None, None


class LSTMLayerFn(torch.autograd.Function):
    """One torch.nn.LSTM layer over (T, B): x (T*B, I) f32 -> (h of every step (T*B, H), h_T,
    c_T).  h0 / c0 (B, H) or None are constants (no gradient)."""

    @staticmethod
    def forward(ctx, x, lm, k, T, B, h0, c0):
        bf = lm._cd == torch.bfloat16
        wd = BF16 if bf else F32
        H, dev = lm.nhid, x.device
        Hp, G = rup(H), 4 * H
        st = ops.stream()
        w_ih = lm._w(f"rnn.weight_ih_l{k}")
        bsum = getattr(lm.rnn, f"bias_ih_l{k}").detach() + getattr(lm.rnn, f"bias_hh_l{k}").detach()
        xc = ops.cast(x, lm._cd)
        xproj = torch.empty(T * B, G, device=dev)
        ops.linear(xc, w_ih, xproj, epi=ops.make_epi(bias=bsum))
        hs = torch.empty(T + 1, B, Hp, device=dev)
        cs = torch.empty(T + 1, B, Hp, device=dev)
        hb = torch.empty(T + 1, B, Hp, dtype=torch.bfloat16, device=dev) if bf else None
        gates = torch.empty(T, B, G, device=dev)
        hs[0].zero_()
        cs[0].zero_()
        if h0 is not None:
            hs[0, :, :H].copy_(h0)
            cs[0, :, :H].copy_(c0)
        if bf:
            hb[0].copy_(hs[0])
        pack = lm._hh[k].fwd.data_ptr()
        hin = hb if bf else hs
        for t in range(T):
            lib.ea_lstm_cell_fwd(wd, B, H, pack, xproj[t * B:].data_ptr(), G, hin[t].data_ptr(), cs[t].data_ptr(), Hp,
                                 hs[t + 1].data_ptr(), cs[t + 1].data_ptr(), Hp, hb[t + 1].data_ptr() if bf else None,
                                 gates[t].data_ptr(), G, st)
        ctx.save = (lm, k, T, B, xc, hs, cs, hb, gates)
        hn, cn = hs[T, :, :H].clone(), cs[T, :, :H].clone()
        ctx.mark_non_differentiable(hn, cn)
        return hs[1:].view(T * B, Hp)[:, :H], hn, cn

    @staticmethod
    def backward(ctx, dy, _dhn, _dcn):
        lm, k, T, B, xc, hs, cs, hb, gates = ctx.save
        ctx.save = None
        bf = lm._cd == torch.bfloat16
        wd = BF16 if bf else F32
        H, dev = lm.nhid, dy.device
        Hp, G = rup(H), 4 * H
        ldd = rup(G)
        st = ops.stream()
        dy = _f32c(dy)
        lddy = dy.stride(0)
        dg = torch.empty(T, B, ldd, device=dev)
        dgb = torch.empty(T, B, ldd, dtype=torch.bfloat16, device=dev) if bf else None
        dc = torch.empty(2, B, Hp, device=dev)
        pack_t = lm._hh[k].bwd.data_ptr()
        dgn = dgb if bf else dg
        for t in range(T - 1, -1, -1):
            first = t == T - 1
            lib.ea_lstm_cell_bwd(wd, B, H, pack_t, None if first else dgn[t + 1].data_ptr(), ldd,
                                 dy[t * B:].data_ptr(), lddy, gates[t].data_ptr(), G, cs[t + 1].data_ptr(),
                                 cs[t].data_ptr(), Hp, None if first else dc[(t + 1) & 1].data_ptr(),
                                 dc[t & 1].data_ptr(), Hp, dg[t].data_ptr(), dgb[t].data_ptr() if bf else None, ldd,
                                 None, 0, st)
        dgm = dgn.view(T * B, ldd)[:, :G]
        w_ih = lm._w(f"rnn.weight_ih_l{k}")
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(T * B, w_ih.shape[1], device=dev)
            ops.linear_dx(dgm, w_ih, dx)
        hprev = (hb if bf else hs)[:T].view(T * B, Hp)[:, :H]
        ops.linear_dw(dgm, xc, getattr(lm.rnn, f"weight_ih_l{k}").grad, accumulate=True)
        ops.linear_dw(dgm, hprev, getattr(lm.rnn, f"weight_hh_l{k}").grad, accumulate=True)
        dg32 = dg.view(T * B, ldd)[:, :G]
        ops.colsum(dg32, getattr(lm.rnn, f"bias_ih_l{k}").grad, accumulate=True)
        ops.colsum(dg32, getattr(lm.rnn, f"bias_hh_l{k}").grad, accumulate=True)
        return dx, None, None, None, None, None, None


class OutLinearFn(torch.autograd.Function):
    """decoder: (rows, nhid) f32 -> (rows, vocab) f32 logits."""

    @staticmethod
    def forward(ctx, x, lm):
        xc = ops.cast(x, lm._cd)
        y = torch.empty(xc.shape[0], lm.vocab_size, device=x.device)
        ops.linear(xc, lm._w("decoder.weight"), y, epi=ops.make_epi(bias=lm.decoder.bias.detach()))
        ctx.save = (xc, lm)
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, lm = ctx.save
        ctx.save = None
        dy = _f32c(dy)
        dyc = ops.cast(dy, lm._cd)
        w = lm._w("decoder.weight")
        dx = torch.empty(xc.shape[0], w.shape[1], device=dy.device)
        ops.linear_dx(dyc, w, dx)
        ops.linear_dw(dyc, xc, lm.decoder.weight.grad, accumulate=True)
        ops.colsum(dy, lm.decoder.bias.grad, accumulate=True)
        return dx, None


class CrossEntropyFn(torch.autograd.Function):
    """Token-averaged cross-entropy of (rows, V) f32 logits on ea_lsm_loss_fwd / bwd with
    smoothing 0: rows whose target is -1 are masked.  -> (loss = sum / #unmasked rows,
    per-row nll (f32, 0 on masked rows)); only the loss is differentiable."""

    @staticmethod
    def forward(ctx, x, tgt):
        rows, V = x.shape
        dev = x.device
        lse = torch.empty(rows, device=dev)
        loss_row = torch.empty(rows, dtype=torch.float64, device=dev)
        stat = torch.zeros(2, dtype=torch.int32, device=dev)
        loss = torch.empty((), device=dev)
        acc = torch.empty((), device=dev)
        inv = torch.empty(1, device=dev)
        lib.ea_lsm_loss_fwd(rows, V, x.data_ptr(), x.stride(0), tgt.data_ptr(), 0.0, -1, 1, float(rows),
                            lse.data_ptr(), loss_row.data_ptr(), stat.data_ptr(), loss.data_ptr(), acc.data_ptr(),
                            inv.data_ptr(), ops.stream())
        ctx.save = (x, tgt, lse, inv)
        nll = loss_row.float()
        ctx.mark_non_differentiable(nll)
        return loss, nll

    @staticmethod
    def backward(ctx, gloss, _gnll):
        x, tgt, lse, inv = ctx.save
        ctx.save = None
        rows, V = x.shape
        grad = torch.empty(rows, V, device=x.device)
        g = gloss.contiguous()
        if g.dtype != torch.float32:
            raise RuntimeError("loss gradients must be float32")
        lib.ea_lsm_loss_bwd(rows, V, x.data_ptr(), x.stride(0), tgt.data_ptr(), 0.0, -1, lse.data_ptr(), g.data_ptr(),
                            inv.data_ptr(), 1.0, grad.data_ptr(), 0, V, ops.stream())
        return grad, None
