"""Training nodes of the recurrent models (SequentialRNNLM, the attention-RNN decoder): the
embedding, dropout, one node per LSTM layer, the output Linear, the loss.

The nodes know no model class.  They take handles the owning module builds once it is bound to
its arena: an LSTMLayer per layer (from (nn.LSTM, k) or an nn.LSTMCell), an EmbedTable, a
LinearHead.  A handle holds the module's own Parameters (their .grad is the arena's gradient
view), the compute-dtype view of its matrix and what the kernels' ABI derives from them.  The
recurrence itself (state buffers, the cell kernels' argument lists, the weight-gradient tail) is
LSTMTape's, shared by LSTMLayerFn and the decoder's attention + layer 0 node.  BiLSTMTape /
BiLSTMLayerFn are the same for the encoder's layers: one or two directions per launch over rows
of unequal lengths (ea_lstm_bicell_fwd / ea_lstm_bicell_bwd).

Rows are time-major inside the path (row t * B + b), so the slice of one time step is a
contiguous (B, .) block for ea_lstm_cell_fwd / ea_lstm_cell_bwd and every product that is not
recurrent is ONE GEMM over all T * B rows.  Activations between the nodes are f32; under amp a
node rounds its matrix operands to bf16 (the arena's bf16 shadow for the weights), the states,
the gates, the cell update and every gradient stay f32.  Parameter gradients are accumulated
into the arena's gradient views (Parameter.grad), as every other node of the package does.
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import torch

from .. import hip_ops as ops
from .._lib import BF16, ENUMS, F32, lib
from .lstm_pack import HHPacks, rup

EMBED_BWD_ROWS = 4096  # ea_embed_bwd stages the ids of one call in LDS
# the operand-block indices of ea_lstm_bicell_fwd / ea_lstm_bicell_bwd (EA_BIF_* / EA_BIB_* of the header)
_BIF = SimpleNamespace(**{k[7:]: v for k, v in ENUMS.items() if k.startswith("EA_BIF_")})
_BIB = SimpleNamespace(**{k[7:]: v for k, v in ENUMS.items() if k.startswith("EA_BIB_")})


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
    weight_hh, and the sizes and dtype code of the cell kernels' ABI.  reverse: the `_reverse`
    parameters of a bidirectional nn.LSTM's layer k."""

    def __init__(self, module, w_ih: torch.Tensor, cd, k: int = None, reverse: bool = False):
        if reverse and k is None:
            raise ValueError("reverse names the second direction of an nn.LSTM layer: give k")
        sfx = ("" if k is None else f"_l{k}") + ("_reverse" if reverse else "")
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


class BiLSTMTape:
    """The recurrence of one layer's ndir = len(layers) directions (1, or 2: forward and reverse)
    over T steps of B rows of unequal lengths `lens` (B int64 on the device), on
    ea_lstm_bicell_fwd / ea_lstm_bicell_bwd: ONE launch per step carries both directions.

    Every direction owns its buffers (the kernels also write the pad columns of a state row, so
    the directions share none): hs / cs (T + 1, B, Hp) f32, hb = hs in bf16 under amp, gates
    (T, B, 4H); for the backward dg / dgb (T, B, ldd) and the carry dc (T, B, Hp).  Direction 0
    keeps its initial state in slot 0 and h_t in slot t + 1; direction 1 keeps its initial state
    in slot T and h_t in slot t.  Both initial slots are zero; every other slot is written by the
    sweep, zeros where t >= lens[b].  The operand blocks hold slot-0 addresses and step strides;
    a step changes only t (and `first`)."""

    def __init__(self, layers, lens: torch.Tensor, T: int, B: int, dev):
        lay = layers[0]
        if len(layers) not in (1, 2) or any((l.H, l.cd) != (lay.H, lay.cd) for l in layers):
            raise ValueError("one or two LSTMLayers of one size and dtype")
        if lens.dtype != torch.long or lens.numel() != B or not lens.is_contiguous():
            raise ValueError(f"lens: {B} int64 lengths on the device")
        self.layers, self.lens, self.T, self.B, self.ndir = layers, lens, T, B, len(layers)
        Hp, bf = lay.Hp, lay.bf
        self.hs, self.cs, self.hb, self.gates = [], [], [], []
        for d in range(self.ndir):
            hs = torch.empty(T + 1, B, Hp, device=dev)
            cs = torch.empty(T + 1, B, Hp, device=dev)
            hb = torch.empty(T + 1, B, Hp, dtype=torch.bfloat16, device=dev) if bf else None
            init = T if d else 0
            hs[init].zero_()
            cs[init].zero_()
            if bf:
                hb[init].zero_()
            self.hs.append(hs)
            self.cs.append(cs)
            self.hb.append(hb)
            self.gates.append(torch.empty(T, B, lay.G, device=dev))
        self.hin = self.hb if bf else self.hs

    def forward(self, xproj):
        """The forward sweep on xproj[d] (T * B, 4H), the input projection of direction d."""
        lay, T, B, ndir = self.layers[0], self.T, self.B, self.ndir
        H, Hp, G, bf = lay.H, lay.Hp, lay.G, lay.bf
        ptrs, strides = (ctypes.c_void_p * (2 * _BIF.NPTR))(), (ctypes.c_long * (2 * _BIF.NSTR))()
        tt = (ctypes.c_int * 2)()
        for d in range(ndir):
            xp = xproj[d]
            if xp.shape != (T * B, G) or xp.stride() != (G, 1):
                raise ValueError(f"xproj {tuple(xp.shape)} for {T} steps of {B} rows")
            hin, hs, cs, hb = self.hin[d], self.hs[d], self.cs[d], self.hb[d]
            prev, out = (1, 0) if d else (0, 1)  # the slot of t's previous / new state, at t = 0
            q, s = d * _BIF.NPTR, d * _BIF.NSTR
            ptrs[q + _BIF.WPACK] = self.layers[d].hh.fwd.data_ptr()
            ptrs[q + _BIF.XPROJ] = xp.data_ptr()
            ptrs[q + _BIF.H_PREV], ptrs[q + _BIF.C_PREV] = hin[prev].data_ptr(), cs[prev].data_ptr()
            ptrs[q + _BIF.H_OUT], ptrs[q + _BIF.C_OUT] = hs[out].data_ptr(), cs[out].data_ptr()
            ptrs[q + _BIF.HB_OUT] = hb[out].data_ptr() if bf else None
            ptrs[q + _BIF.GATES] = self.gates[d].data_ptr()
            for i, v in ((_BIF.LDX, G), (_BIF.SX, B * G), (_BIF.LDS, Hp), (_BIF.SS, B * Hp), (_BIF.LDG, G),
                         (_BIF.SG, B * G)):
                strides[s + i] = v
        wd, lens, st = lay.wd, self.lens.data_ptr(), ops.stream()
        for s in range(T):
            tt[0], tt[1] = s, T - 1 - s
            lib.ea_lstm_bicell_fwd(wd, ndir, B, H, lens, ptrs, strides, tt, st)

    def outputs(self) -> torch.Tensor:
        """h of every step, the directions side by side: a new (T * B, ndir * H) f32 tensor (a
        concat copy: the next GEMM reads one operand)."""
        H, TB = self.layers[0].H, self.T * self.B
        y = torch.empty(TB, self.ndir * H, device=self.hs[0].device)
        for d in range(self.ndir):
            hs = self.hs[d][:self.T] if d else self.hs[d][1:]
            y[:, d * H:(d + 1) * H].copy_(hs.view(TB, -1)[:, :H])
        return y

    def backward(self, dy: torch.Tensor):
        """The backward sweep on dy (T * B, ndir * H) f32 contiguous; leaves every step's gate
        gradients in dg[d] (dgm[d]: their (T * B, 4H) view in the compute dtype)."""
        lay, T, B, ndir = self.layers[0], self.T, self.B, self.ndir
        H, Hp, G, ldd, bf = lay.H, lay.Hp, lay.G, lay.ldd, lay.bf
        dev = dy.device
        if dy.shape != (T * B, ndir * H) or not dy.is_contiguous() or dy.dtype != torch.float32:
            raise ValueError(f"dy {tuple(dy.shape)} for {T} steps of {B} rows, {ndir} directions")
        self.dg, self.dgm, keep = [], [], []
        ptrs, strides = (ctypes.c_void_p * (2 * _BIB.NPTR))(), (ctypes.c_long * (2 * _BIB.NSTR))()
        tt, first = (ctypes.c_int * 2)(), (ctypes.c_int * 2)()
        for d in range(ndir):
            dg = torch.empty(T, B, ldd, device=dev)
            dgb = torch.empty(T, B, ldd, dtype=torch.bfloat16, device=dev) if bf else None
            dc = torch.empty(T, B, Hp, device=dev)
            dgn = dgb if bf else dg
            self.dg.append(dg)
            self.dgm.append(dgn.view(T * B, ldd)[:, :G])
            keep.append(dc)
            cs, q, s = self.cs[d], d * _BIB.NPTR, d * _BIB.NSTR
            nxt = -1 if d else 1  # the step this direction's sweep ran before t, relative to t
            ptrs[q + _BIB.WPACK_T] = self.layers[d].hh.bwd.data_ptr()
            ptrs[q + _BIB.DGATES_NEXT] = dgn.data_ptr() + nxt * B * ldd * dgn.element_size()
            ptrs[q + _BIB.DH_OUT] = dy.data_ptr() + d * H * 4
            ptrs[q + _BIB.GATES] = self.gates[d].data_ptr()
            ptrs[q + _BIB.C], ptrs[q + _BIB.C_PREV] = (cs[0].data_ptr(), cs[1].data_ptr()) if d else (cs[1].data_ptr(),
                                                                                                    cs[0].data_ptr())
            ptrs[q + _BIB.DC_IN] = dc.data_ptr() + nxt * B * Hp * 4
            ptrs[q + _BIB.DC_OUT] = dc.data_ptr()
            ptrs[q + _BIB.DGATES] = dg.data_ptr()
            ptrs[q + _BIB.DGATES_B] = dgb.data_ptr() if bf else None
            for i, v in ((_BIB.LDD, ldd), (_BIB.SD, B * ldd), (_BIB.LDDH, ndir * H), (_BIB.SDH, B * ndir * H),
                         (_BIB.LDG, G), (_BIB.SG, B * G), (_BIB.LDC, Hp), (_BIB.SC, B * Hp), (_BIB.LDDC, Hp),
                         (_BIB.SDC, B * Hp)):
                strides[s + i] = v
        wd, lens, st = lay.wd, self.lens.data_ptr(), ops.stream()
        for s in range(T):
            tt[0], tt[1] = T - 1 - s, s
            first[0] = first[1] = int(s == 0)
            lib.ea_lstm_bicell_bwd(wd, ndir, B, H, lens, ptrs, strides, tt, first, st)
        del keep  # the launches are stream ordered: the allocator reuses dc only after them

    def weight_grads(self, x: torch.Tensor):
        """Every direction's four parameter gradients from dgm and the input rows x (T * B, I)
        in the compute dtype, as LSTMTape.weight_grads."""
        TB = self.T * self.B
        for d, lay in enumerate(self.layers):
            hin = self.hin[d][1:] if d else self.hin[d][:self.T]
            hprev = hin.view(TB, lay.Hp)[:, :lay.H]
            ops.linear_dw(self.dgm[d], x, lay.weight_ih.grad, accumulate=True)
            ops.linear_dw(self.dgm[d], hprev, lay.weight_hh.grad, accumulate=True)
            dg32 = self.dg[d].view(TB, lay.ldd)[:, :lay.G]
            ops.colsum(dg32, lay.bias_ih.grad, accumulate=True)
            ops.colsum(dg32, lay.bias_hh.grad, accumulate=True)


class BiLSTMLayerFn(torch.autograd.Function):
    """One (bi)directional LSTM layer over (T, B) rows of lengths lens, torch.nn.LSTM on a
    pack_padded_sequence: x (T*B, I) f32 -> (T*B, ndir*H) f32, [forward | reverse], rows at
    t >= lens[b] exactly 0.  layers: the LSTMLayer of each direction.  Zero initial states.
    anchor (a tensor that requires grad, or None) keeps the node in the graph when x, the features
    of the first layer, does not require grad."""

    @staticmethod
    def forward(ctx, x, layers, lens, T, B, anchor=None):
        xc = ops.cast(x, layers[0].cd)
        xproj = [lay.input_proj(xc, lay.w_ih, lay.bias_sum()) for lay in layers]
        tape = BiLSTMTape(layers, lens, T, B, x.device)
        tape.forward(xproj)
        ctx.save = (tape, xc)
        return tape.outputs()

    @staticmethod
    def backward(ctx, dy):
        tape, xc = ctx.save
        ctx.save = None
        tape.backward(f32c(dy).contiguous())
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(xc.shape[0], tape.layers[0].I, device=dy.device)
            for d, lay in enumerate(tape.layers):
                ops.linear_dx(tape.dgm[d], lay.w_ih, dx, epi=ops.make_epi(beta=1.0) if d else None)
        tape.weight_grads(xc)
        return dx, None, None, None, None, None


class TanhFn(torch.autograd.Function):
    """tanh on ea_tanh_fwd / ea_tanh_bwd, f32."""

    @staticmethod
    def forward(ctx, x):
        x = f32c(x).contiguous()
        y = torch.empty_like(x)
        lib.ea_tanh_fwd(x.numel(), x.data_ptr(), y.data_ptr(), ops.stream())
        ctx.save = y
        return y

    @staticmethod
    def backward(ctx, dy):
        y = ctx.save
        ctx.save = None
        dy = f32c(dy).contiguous()
        dx = torch.empty_like(y)
        lib.ea_tanh_bwd(y.numel(), y.data_ptr(), dy.data_ptr(), dx.data_ptr(), ops.stream())
        return dx


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
