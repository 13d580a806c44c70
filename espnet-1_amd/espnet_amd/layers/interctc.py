"""Intermediate CTC and self-conditioned CTC taps of the Conformer encoder
(espnet2/asr/encoder/conformer_encoder.py:341-367, espnet2/asr/espnet_model.py:242-286).

A tap after encoder layer l is ONE autograd node on the f32 residual stream x:

    y      = after_norm(x)                       (the encoder's shared final LayerNorm)
    logits = ctc_lo(y)                           one GEMM, kept in f32
    p, lse = softmax(logits), logsumexp(logits)  ea_softmax_lse_rows, one read of the logits
    loss   = CTC(logits, lse)                    the lattice alone (ea_ctc_loss_fwd_lse), on the
                                                 auxiliary stream beside the layers that follow
    x'     = x + conditioning_layer(p)           GEMM with the bias + residual epilogue

The logits serve the loss and the conditioning alike: the reference applies the CTC head's
dropout to the loss branch only, so a head dropout > 0 is refused with taps (ESPnetASRModel).

Backward: the gradient w.r.t. the logits is formed once, by ea_interctc_dlogits, from both
consumers of the softmax (the CTC loss and, through dp = dx' W_c, the conditioning branch), so
the ctc_lo input- and weight-gradient GEMMs run once per tap.  after_norm and ctc_lo get
gradients from every tap and from the final head: all of them accumulate into the gradient
arena, and the three shared prefixes (ctc., encoder.after_norm., encoder.conditioning_layer.)
report grad_ready once per backward, from the lowest tap — the last to run (TapState).
"""
from __future__ import annotations

import torch

from .common import EPI_RESID, F32, empty, lib, ln_bwd, ln_fwd, ops
from .losses import _g


class TapState:
    """Per-encoder bookkeeping of the shared-parameter readiness.  While `deferred` is set, the
    final after_norm / CTC head backward do not report grad_ready (hip_ops.grad_ready: under
    data parallelism that starts the bucket's all-reduce, and the taps still write into it); the
    lowest tap's backward reports for them.  Armed by the encoder at every forward that builds
    a graph through its taps, cleared otherwise."""

    def __init__(self):
        self.deferred = False

    def arm(self, on: bool, *modules):
        self.deferred = on
        for m in modules:
            if m is not None:
                m._ready_deferred = on


class InterCTCTapFn(torch.autograd.Function):
    """(x, hlens, ys, ylens, enc, ctc, Lmax, first) -> (x', loss_ic, y).

    ys None: no loss (inference, or interctc_weight 0): loss_ic is 0 and the lattice does not
    run.  enc.interctc_use_conditioning False: x' is x.  y (B,T,d) f32 is the tap's normalised
    output for the eval-mode CER (not differentiable: its consumers are this node's own).
    `first`: the lowest tap, whose backward is the last writer of the shared gradients."""

    @staticmethod
    def forward(ctx, x, hlens, ys, ylens, enc, ctc, Lmax, first):
        bn, bc = enc.after_norm._b, ctc._b
        cd = bc.cd
        B, T, d = x.shape
        V = ctc.ctc_lo.out_features
        N = B * T
        dev = x.device
        cond = bool(enc.interctc_use_conditioning)
        x2 = x.reshape(N, d)
        y, mu, rs = ln_fwd(x2, bn, "", F32)
        h = ops.cast(y, cd)
        logits = empty(N, V, device=dev)
        ops.linear(h, bc.w("ctc_lo.weight"), logits, epi=ops.make_epi(bias=bc.f("ctc_lo.bias")))
        lse = empty(N, device=dev)
        p = empty(N, V, dtype=cd, device=dev)
        lib.ea_softmax_lse_rows(N, V, logits.data_ptr(), V, lse.data_ptr(), p.data_ptr(), ops.dt(p), V, ops.stream())
        loss = empty((), device=dev)
        lat = None
        if ys is not None:
            S = 2 * Lmax + 1
            alpha = torch.empty(N * S, dtype=torch.float64, device=dev)
            beta = torch.empty(N * S, dtype=torch.float64, device=dev)
            nll = torch.empty(B, dtype=torch.float64, device=dev)
            loss_utt = empty(B, device=dev)
            # T' serial steps on 2 workgroups per utterance: beside the encoder layers that
            # follow (ESPnetASRModel.forward joins the auxiliary stream before it combines losses)
            with ops.aux(logits, lse, hlens, ys, ylens, alpha, beta, nll, loss_utt, loss):
                lib.ea_ctc_loss_fwd_lse(B, T, V, logits.data_ptr(), V, hlens.data_ptr(), ys.data_ptr(), ys.stride(0),
                                        ylens.data_ptr(), Lmax, lse.data_ptr(), alpha.data_ptr(), beta.data_ptr(),
                                        nll.data_ptr(), loss_utt.data_ptr(), loss.data_ptr(), ops.stream())
            lat = (alpha, beta, nll, hlens, ys, ylens)
        else:
            loss.zero_()
        if cond:
            be = enc.conditioning_layer._b
            xo = empty(N, d, device=dev)
            ops.linear(p, be.w("weight"), xo, epi=ops.make_epi(EPI_RESID, bias=be.f("bias"), resid=x2))
        else:
            xo = x2
        if torch.is_grad_enabled() or x.requires_grad:
            ctx.save = (x2, mu, rs, h, logits, lse, p if cond else None, lat)
            ctx.mods = (enc, ctc)
            ctx.meta = (B, T, d, V, Lmax, cond, first)
        yv = y.view(B, T, d)
        ctx.mark_non_differentiable(yv)
        return xo.view(B, T, d), loss, yv

    @staticmethod
    def backward(ctx, gx, gl, gy):
        x2, mu, rs, h, logits, lse, p, lat = ctx.save
        ctx.save = None
        enc, ctc = ctx.mods
        B, T, d, V, Lmax, cond, first = ctx.meta
        bn, bc = enc.after_norm._b, ctc._b
        cd = bc.cd
        N = B * T
        dev = gx.device
        dxo = gx.reshape(N, d)
        if dxo.dtype != F32:
            raise RuntimeError("the residual-stream gradient must be float32")
        dxo = dxo.contiguous()
        dp = None
        if cond:
            be = enc.conditioning_layer._b
            dxc = ops.cast(dxo, cd)
            with ops.wgrad(dxc, p):
                ops.linear_dw(dxc, p, be.g("weight"), accumulate=True,
                              db=be.g("bias"))
            dp = empty(N, V, dtype=cd, device=dev)
            ops.linear_dx(dxc, be.w("weight"), dp)
        if lat is None and dp is None:  # neither a loss nor conditioning: the tap only observed
            if first:
                _report_shared(enc, ctc)
            return gx, None, None, None, None, None, None, None
        dl = empty(N, V, dtype=cd, device=dev)
        if lat is not None:
            alpha, beta, nll, hlens, ys, ylens = lat
            gl = _g(gl)
            lib.ea_interctc_dlogits(B, T, V, logits.data_ptr(), V, hlens.data_ptr(), ys.data_ptr(), ys.stride(0),
                                    ylens.data_ptr(), Lmax, lse.data_ptr(), alpha.data_ptr(), beta.data_ptr(),
                                    nll.data_ptr(), gl.data_ptr(), 1.0 / B, ops.ptr(dp), V, dl.data_ptr(), ops.dt(dl),
                                    V, ops.stream())
        else:
            lib.ea_interctc_dlogits(B, T, V, logits.data_ptr(), V, None, None, 0, None, 0, lse.data_ptr(), None, None,
                                    None, None, 0.0, dp.data_ptr(), V, dl.data_ptr(), ops.dt(dl), V, ops.stream())
        with ops.wgrad(dl, h):
            ops.linear_dw(dl, h, bc.g("ctc_lo.weight"), accumulate=True,
                          db=bc.g("ctc_lo.bias"))
        dy = empty(N, d, device=dev)
        ops.linear_dx(dl, bc.w("ctc_lo.weight"), dy)
        dx = dxo.clone()  # (dx' itself belongs to autograd)
        ln_bwd(dy, x2, bn, "", mu, rs, dx, accumulate=True)  # dx = dx' + LN_bwd(dy)
        if first:
            _report_shared(enc, ctc)
        return dx.view(B, T, d), None, None, None, None, None, None, None


def _report_shared(enc, ctc):
    """The shared parameters' gradients are final: every later tap and the final head wrote
    theirs earlier in this backward."""
    if not enc._taps.deferred:
        return
    ops.grad_ready(ctc._b)
    ops.grad_ready(enc.after_norm._b)
    if enc.conditioning_layer is not None:
        ops.grad_ready(enc.conditioning_layer._b)


class InterCTCMixFn(torch.autograd.Function):
    """loss_ctc' = (1 - w)*loss_ctc + w * mean_k(loss_ic_k)  (espnet_model.py:281-286)."""

    @staticmethod
    def forward(ctx, w, loss_ctc, *loss_ics):
        dev = loss_ctc.device
        st = ops.stream()
        K = len(loss_ics)
        s = loss_ics[0]
        for l in loss_ics[1:]:
            t = empty((), device=dev)
            lib.ea_axpby_scalar(s.data_ptr(), 1.0, l.data_ptr(), 1.0, t.data_ptr(), st)
            s = t
        out = empty((), device=dev)
        lib.ea_axpby_scalar(loss_ctc.data_ptr(), 1.0 - w, s.data_ptr(), w / K, out.data_ptr(), st)
        ctx.wk = (w, K)
        return out

    @staticmethod
    def backward(ctx, g):
        w, K = ctx.wk
        g = _g(g)
        st = ops.stream()
        ga = empty((), device=g.device)
        gb = empty((), device=g.device)
        lib.ea_axpby_scalar(g.data_ptr(), 1.0 - w, 0, 0.0, ga.data_ptr(), st)
        lib.ea_axpby_scalar(g.data_ptr(), w / K, 0, 0.0, gb.data_ptr(), st)
        return (None, ga) + (gb,) * K
