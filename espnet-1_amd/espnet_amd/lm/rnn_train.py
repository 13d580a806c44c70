"""Training nodes of the recurrent models (SequentialRNNLM, the attention-RNN decoder): the
embedding, dropout, one node per LSTM layer, the output Linear, the loss.

The nodes know no model class.  They take handles the owning module builds once it is bound to
its arena: an LSTMLayer per layer (from (nn.LSTM, k) or an nn.LSTMCell), an EmbedTable, a
LinearHead.  A handle holds the module's own Parameters (their .grad is the arena's gradient
view), the compute-dtype view of its matrix and what the kernels' ABI derives from them.  The
recurrence itself (state buffers, the cell kernels' argument lists, the weight-gradient tail) is
LSTMTape's, shared by LSTMLayerFn and the decoder's attention + layer 0 node.

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
from .lstm_pack import HHPacks, rup

EMBED_BWD_ROWS = 4096  # ea_embed_bwd stages the ids of one call in LDS


def f32c(t: torch.Tensor) -> torch.Tensor:
    """An f32 gradient with unit inner stride."""
    if t.dtype != torch.float32:
        raise RuntimeError("gradients between the LM's nodes are float32")
    return t if t.stride(-1) == 1 else t.contiguous()


def _steps(x: torch.Tensor, rows: int = 1):
    """(address of x[0], bytes from one step's block of `rows` leading indices to the next)."""
    return x.data_ptr(), rows * x.stride(0) * x.element_size()


class EmbedTable:
    """An nn.Embedding for EmbedFn: its weight Parameter, padding_idx and the zero position row
    ea_embed_fwd adds."""

    def __init__(self, emb: torch.nn.Embedding, device):
        self.weight, self.padding_idx = emb.weight, emb.padding_idx
        self.pe0 = torch.zeros(1, emb.embedding_dim, device=device)


class LinearHead:
    """An nn.Linear for OutLinearFn: its Parameters and w, the weight in the compute dtype cd."""

    def __init__(self, lin: torch.nn.Linear, w: torch.Tensor, cd):
        self.weight, self.bias, self.w, self.cd = lin.weight, lin.bias, w, cd


class LSTMLayer:
    """One LSTM layer for the recurrent kernels: the four Parameters of nn.LSTM's layer k or of an
    nn.LSTMCell (k None), w_ih = weight_ih in the compute dtype cd (an arena view), the HHPacks of
    weight_hh, and the sizes and dtype code of the cell kernels' ABI."""

    def __init__(self, module, w_ih: torch.Tensor, cd, k: int = None):
        sfx = "" if k is None else f"_l{k}"
        self.weight_ih, self.weight_hh = getattr(module, "weight_ih" + sfx), getattr(module, "weight_hh" + sfx)
        self.bias_ih, self.bias_hh = getattr(module, "bias_ih" + sfx), getattr(module, "bias_hh" + sfx)
        self.w_ih, self.cd = w_ih, cd
        self.G, self.I = self.weight_ih.shape
        self.H = self.weight_hh.shape[1]
        self.Hp, self.ldd = rup(self.H), rup(self.G)  # row strides of the states / of the gate gradients
        self.bf = cd == torch.bfloat16
        self.wd = BF16 if self.bf else F32
        self.hh = HHPacks(self.weight_hh, cd)

    def refresh(self):
        """After the weights changed: repack weight_hh, on the stream."""
        self.hh.refresh(self.weight_hh)

    def bias_sum(self) -> torch.Tensor:
        return self.bias_ih.detach() + self.bias_hh.detach()

    def input_proj(self, x: torch.Tensor, w: torch.Tensor, bsum: torch.Tensor) -> torch.Tensor:
        """xproj = x . w^T + (bias_ih + bias_hh) over all rows (w: w_ih or its leading columns)."""
        xproj = torch.empty(x.shape[0], self.G, device=x.device)
        ops.linear(x, w, xproj, epi=ops.make_epi(bias=bsum))
        return xproj


class LSTMTape:
    """The recurrence of one layer over T steps of B rows: the states hs / cs (T + 1, B, Hp) f32
    (row 0 the initial state: zero, or h0 / c0), hb = hs in bf16 under amp (hin is what the kernels
    read), the gates (T, B, 4H); for the backward dg / dgb (T, B, ldd), the gate gradients (dgm:
    their (T * B, 4H) view in the compute dtype), and the cell-gradient ping-pong dc.  The loops over
    the steps are launch-latency bound: fwd_steps / bwd_steps resolve every pointer, stride and size
    once and return the step, which addresses step t's rows by offset and makes no tensor view."""

    def __init__(self, layer: LSTMLayer, T: int, B: int, dev, h0=None, c0=None):
        H, Hp, bf = layer.H, layer.Hp, layer.bf
        self.layer, self.T, self.B = layer, T, B
        self.hs = hs = torch.empty(T + 1, B, Hp, device=dev)
        self.cs = cs = torch.empty(T + 1, B, Hp, device=dev)
        self.hb = hb = torch.empty(T + 1, B, Hp, dtype=torch.bfloat16, device=dev) if bf else None
        self.gates = torch.empty(T, B, layer.G, device=dev)
        hs[0].zero_()
        cs[0].zero_()
        if h0 is not None:
            hs[0, :, :H].copy_(h0)
            cs[0, :, :H].copy_(c0)
        if bf:
            hb[0].copy_(hs[0])
        self.hin = hb if bf else hs

    def fwd_steps(self, xproj: torch.Tensor):
        """-> step(t): ea_lstm_cell_fwd of step t on rows t * B.. of xproj (T * B, 4H)."""
        lay, B, hs, cs, hb, hin, gates = self.layer, self.B, self.hs, self.cs, self.hb, self.hin, self.gates
        wd, H, Hp, G, bf = lay.wd, lay.H, lay.Hp, lay.G, lay.bf
        pack, st, T = lay.hh.fwd.data_ptr(), ops.stream(), self.T
        if xproj.shape[0] < T * B or xproj.stride(1) != 1:
            raise ValueError(f"xproj {tuple(xproj.shape)} for {T} steps of {B} rows")
        (xp, sx), (hi, shi), (cp, sc), (hp, sh), (gp, sg) = (
            _steps(xproj, B), _steps(hin), _steps(cs), _steps(hs), _steps(gates))
        hbp, shb = _steps(hb) if bf else (None, 0)

        def step(t, _alive=(xproj, self)):  # the step holds addresses: it keeps their buffers alive
            if not 0 <= t < T:
                raise IndexError(t)
            lib.ea_lstm_cell_fwd(wd, B, H, pack, xp + t * sx, G, hi + t * shi, cp + t * sc, Hp, hp + (t + 1) * sh,
                                 cp + (t + 1) * sc, Hp, hbp + (t + 1) * shb if bf else None, gp + t * sg, G, st)
        return step

    def outputs(self) -> torch.Tensor:
        """h of every step, (T * B, H).  (Not kept here: the node's output must not hang on its own tape.)"""
        return self.hs[1:].view(self.T * self.B, self.layer.Hp)[:, :self.layer.H]

    def bwd_steps(self, dy: torch.Tensor, lddy: int):
        """Allocates the backward buffers -> step(t): ea_lstm_cell_bwd of step t, called for
        t = T - 1 .. 0, on rows t * B.. of dy (row stride lddy); leaves dgates_t in dg[t]
        (dgn[t] in the compute dtype)."""
        lay, T, B, cs, gates = self.layer, self.T, self.B, self.cs, self.gates
        wd, H, Hp, G, ldd, bf = lay.wd, lay.H, lay.Hp, lay.G, lay.ldd, lay.bf
        dev = dy.device
        self.dg = dg = torch.empty(T, B, ldd, device=dev)
        dgb = torch.empty(T, B, ldd, dtype=torch.bfloat16, device=dev) if bf else None
        dc = torch.empty(2, B, Hp, device=dev)
        self.dgn = dgn = dgb if bf else dg
        self.dgm = dgn.view(T * B, ldd)[:, :G]  # all steps' gate gradients in the compute dtype, (T * B, 4H)
        pack_t, st = lay.hh.bwd.data_ptr(), ops.stream()
        if dy.shape[0] < T * B:
            raise ValueError(f"dy {tuple(dy.shape)} for {T} steps of {B} rows")
        yp, sy = dy.data_ptr(), B * lddy * dy.element_size()
        (gp, sg), (cp, sc), (dnp, sdn), (dgp, sdg), (dcp, sdc) = (
            _steps(gates), _steps(cs), _steps(dgn), _steps(dg), _steps(dc))
        dbp, sdb = _steps(dgb) if bf else (None, 0)

        def step(t, _alive=(dy, dc, self)):
            if not 0 <= t < T:
                raise IndexError(t)
            first = t == T - 1
            lib.ea_lstm_cell_bwd(wd, B, H, pack_t, None if first else dnp + (t + 1) * sdn, ldd, yp + t * sy, lddy,
                                 gp + t * sg, G, cp + (t + 1) * sc, cp + t * sc, Hp,
                                 None if first else dcp + ((t + 1) & 1) * sdc, dcp + (t & 1) * sdc, Hp, dgp + t * sdg,
                                 dbp + t * sdb if bf else None, ldd, None, 0, st)
        return step

    def weight_grads(self, x: torch.Tensor) -> torch.Tensor:
        """The layer's four parameter gradients from dgm and the input rows x (T * B, I) in the
        compute dtype -> h_prev of every step (T * B, H), the other operand."""
        lay, TB, dgm = self.layer, self.T * self.B, self.dgm
        hprev = self.hin[:self.T].view(TB, lay.Hp)[:, :lay.H]
        ops.linear_dw(dgm, x, lay.weight_ih.grad, accumulate=True)
        ops.linear_dw(dgm, hprev, lay.weight_hh.grad, accumulate=True)
        dg32 = self.dg.view(TB, lay.ldd)[:, :lay.G]
        ops.colsum(dg32, lay.bias_ih.grad, accumulate=True)
        ops.colsum(dg32, lay.bias_hh.grad, accumulate=True)
        return hprev


class EmbedFn(torch.autograd.Function):
    """rows of an EmbedTable by token id -> (rows, dim) f32.  The row of padding_idx receives no
    gradient (torch.nn.Embedding(padding_idx=...))."""

    @staticmethod
    def forward(ctx, anchor, tok, table):
        rows, d = tok.numel(), table.weight.shape[1]
        x = torch.empty(rows, d, device=tok.device)
        lib.ea_embed_fwd(rows, d, 1, tok.data_ptr(), table.weight.data_ptr(), 1.0, table.pe0.data_ptr(), 0.0, 0,
                         x.data_ptr(), ops.stream())
        ctx.save = (tok, table)
        return x

    @staticmethod
    def backward(ctx, dx):
        tok, table = ctx.save
        ctx.save = None
        dx = f32c(dx).contiguous()
        rows, d = tok.numel(), table.weight.shape[1]
        dE = table.weight.grad
        # ea_embed_bwd sums the rows of one token in increasing order inside a call; the calls
        # are stream ordered, so the result does not depend on anything but the batch
        for r0 in range(0, rows, EMBED_BWD_ROWS):
            n = min(EMBED_BWD_ROWS, rows - r0)
            lib.ea_embed_bwd(n, d, tok[r0:].data_ptr(), dx[r0:].data_ptr(), 1.0, 0.0, 0, dE.data_ptr(), ops.stream())
        pad = table.padding_idx
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
        dy = f32c(dy)
        dx = torch.empty(dy.shape, device=dy.device)
        ops.scale_dropout(dy, dx, p=p, seed=seed)
        return dx, None, None


class LSTMLayerFn(torch.autograd.Function):
    """One LSTMLayer over (T, B): x (T*B, I) f32 -> (h of every step (T*B, H), h_T, c_T).
    h0 / c0 (B, H) or None are constants (no gradient)."""

    @staticmethod
    def forward(ctx, x, layer, T, B, h0, c0):
        H = layer.H
        bsum = layer.bias_sum()
        xc = ops.cast(x, layer.cd)
        xproj = layer.input_proj(xc, layer.w_ih, bsum)
        tape = LSTMTape(layer, T, B, x.device, h0, c0)
        step = tape.fwd_steps(xproj)
        for t in range(T):
            step(t)
        ctx.save = (tape, xc)
        hn, cn = tape.hs[T, :, :H].clone(), tape.cs[T, :, :H].clone()
        ctx.mark_non_differentiable(hn, cn)
        return tape.outputs(), hn, cn

    @staticmethod
    def backward(ctx, dy, _dhn, _dcn):
        tape, xc = ctx.save
        ctx.save = None
        layer = tape.layer
        dy = f32c(dy)
        step = tape.bwd_steps(dy, dy.stride(0))
        for t in range(tape.T - 1, -1, -1):
            step(t)
        dgm, dx = tape.dgm, None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(dgm.shape[0], layer.I, device=dy.device)
            ops.linear_dx(dgm, layer.w_ih, dx)
        tape.weight_grads(xc)
        return dx, None, None, None, None, None


class OutLinearFn(torch.autograd.Function):
    """A LinearHead: (rows, in) f32 -> (rows, out) f32 logits."""

    @staticmethod
    def forward(ctx, x, head):
        xc = ops.cast(x, head.cd)
        y = torch.empty(xc.shape[0], head.weight.shape[0], device=x.device)
        ops.linear(xc, head.w, y, epi=ops.make_epi(bias=head.bias.detach()))
        ctx.save = (xc, head)
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, head = ctx.save
        ctx.save = None
        dy = f32c(dy)
        dyc = ops.cast(dy, head.cd)
        dx = torch.empty(xc.shape[0], head.w.shape[1], device=dy.device)
        ops.linear_dx(dyc, head.w, dx)
        ops.linear_dw(dyc, xc, head.weight.grad, accumulate=True)
        ops.colsum(dy, head.bias.grad, accumulate=True)
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
