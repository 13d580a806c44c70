"""E-Branchformer encoder block — espnet2/asr/encoder/e_branchformer_encoder.py:49-177 with the
cgMLP of espnet2/asr/layers/cgmlp.py (rel-pos MHSA branch, convolutional gating MLP branch,
depthwise merge convolution, optional FFN / macaron FFN).

Parameter holders keep the reference's attribute names, constructor order and torch default
initialisation (same seed -> same weights, same state_dict keys); the computation is
`EBranchformerBlockFn`: one autograd node per block running the block's HIP kernels forward and
its hand-written backward.

Data layout as the Conformer block's (layers/conformer.py): x (B*T, d) f32 residual stream, GEMM
operands in the compute dtype cd.  The two branch GEMMs (attn.linear_out, cgmlp.channel_proj2)
write, bias and output dropout applied, straight into the halves of x_concat (B*T, 2d) — there
is no concatenation kernel — and their backward GEMMs read the halves of dxc through strided
views.  channel_proj1 stores its PRE-activation h; the exact GELU, the gate LayerNorm and the
depthwise convolution of the CSGU run inside ea_csgu_fwd / ea_csgu_bwd (csrc/ebranchformer.hip).

Dropout sites of a block (site_seed(seed, layer, site)): 1, 2 macaron FFN; 3 attention
probabilities; 4 attention branch output; 5 CSGU output; 6 cgMLP branch output; 7 merge_proj
output; 8, 9 FFN.
"""
from __future__ import annotations

import ctypes

import torch
from torch import nn

from .common import (ACT_SWISH, EPI_RESID, EPI_STORE, F32, REL_LATEST, Bound, drop_arg, dv_buf, empty, lib, ln_bwd,
                     ln_fwd, ops, site_dv, site_seed)
from .conformer import LayerNorm
from .sublayers import ffn_bwd, ffn_fwd, rel_attn_bwd, rel_attn_fwd

CONV_KERNELS = (3, 5, 7, 15, 31)  # the depthwise kernels' compiled widths


# ----------------------------------------------------------------------------- holders
class ConvolutionalSpatialGatingUnit(nn.Module):
    """cgmlp.py:15-48 parameter set."""

    def __init__(self, size, kernel_size, dropout_rate, use_linear_after_conv, gate_activation):
        super().__init__()
        if use_linear_after_conv:
            raise NotImplementedError("use_linear_after_conv=True is not on the HIP hot path")
        if gate_activation != "identity":
            raise NotImplementedError(f"gate_activation={gate_activation} is not on the HIP hot path")
        n_channels = size // 2
        self.norm = LayerNorm(n_channels)
        self.conv = nn.Conv1d(n_channels, n_channels, kernel_size, 1, (kernel_size - 1) // 2, groups=n_channels)
        self.linear = None
        self.kernel_size = kernel_size
        self.dropout_rate = dropout_rate


class ConvolutionalGatingMLP(nn.Module):
    """cgmlp.py:84-108 parameter set (channel_proj1 = Sequential(Linear, GELU): key channel_proj1.0.*)."""

    def __init__(self, size, linear_units, kernel_size, dropout_rate, use_linear_after_conv, gate_activation):
        super().__init__()
        self.channel_proj1 = nn.Sequential(nn.Linear(size, linear_units), nn.GELU())
        self.csgu = ConvolutionalSpatialGatingUnit(linear_units, kernel_size, dropout_rate, use_linear_after_conv,
                                                   gate_activation)
        self.channel_proj2 = nn.Linear(linear_units // 2, size)
        self.linear_units = linear_units


class EBranchformerEncoderLayer(nn.Module):
    """e_branchformer_encoder.py:62-102 parameter set + HIP forward."""

    def __init__(self, size, attn, cgmlp, feed_forward, feed_forward_macaron, dropout_rate, merge_conv_kernel=3):
        super().__init__()
        if feed_forward is None:
            raise NotImplementedError("use_ffn=False is not on the HIP hot path")
        self.size = size
        self.attn = attn
        self.cgmlp = cgmlp
        self.feed_forward = feed_forward
        self.feed_forward_macaron = feed_forward_macaron
        self.ff_scale = 1.0
        if self.feed_forward is not None:
            self.norm_ff = LayerNorm(size)
        if self.feed_forward_macaron is not None:
            self.ff_scale = 0.5
            self.norm_ff_macaron = LayerNorm(size)
        self.norm_mha = LayerNorm(size)
        self.norm_mlp = LayerNorm(size)
        self.norm_final = LayerNorm(size)
        self.dropout_rate = dropout_rate
        self.depthwise_conv_fusion = nn.Conv1d(size + size, size + size, kernel_size=merge_conv_kernel, stride=1,
                                               padding=(merge_conv_kernel - 1) // 2, groups=size + size, bias=True)
        self.merge_proj = nn.Linear(size + size, size)
        self.merge_conv_kernel = merge_conv_kernel
        self.layer_idx = 0
        self._b = None

    def bind(self, arena, prefix, cd):
        self._b = Bound(arena, prefix, cd)

    @staticmethod
    def arena_groups(prefix):
        a = prefix + "attn."
        return [[a + "linear_q.weight", a + "linear_k.weight", a + "linear_v.weight"],
                [a + "linear_q.bias", a + "linear_k.bias", a + "linear_v.bias"]]

    def forward(self, x, pos_emb, olens, seed):
        return EBranchformerBlockFn.apply(x, pos_emb, olens, self, seed, self.training)


def _long(v=0):
    return ctypes.c_long(v)


class EBranchformerBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pos, olens, L: EBranchformerEncoderLayer, seed, training):
        b = L._b
        cd = b.cd
        B, T, d = x.shape
        N = B * T
        dev = x.device
        p = L.dropout_rate if training else 0.0
        pa = L.attn.dropout_rate if training else 0.0
        pg = L.cgmlp.csgu.dropout_rate if training else 0.0  # the CSGU's own dropout (cgmlp.py:80)
        li = L.layer_idx
        sd = lambda s: site_seed(seed, li, s)  # noqa: E731
        macaron = L.feed_forward_macaron is not None
        ff = dict(act=ACT_SWISH, p_in=p, p_out=p, rscale=L.ff_scale)
        x0 = x.reshape(N, d)
        # ---- macaron FFN (e_branchformer_encoder.py:126-129)
        if macaron:
            x1, s_ff1 = ffn_fwd(b, x0, "feed_forward_macaron", "norm_ff_macaron", seed_in=sd(1), seed_out=sd(2), **ff)
        else:
            x1, s_ff1 = x0, None
        xc = empty(N, 2 * d, dtype=cd, device=dev)  # x_concat = [x1 | x2]
        # ---- branch 1: rel-pos MHSA, no residual (:136-146)
        xna, mua, rsa = ln_fwd(x1, b, "norm_mha", cd)
        O, s_core = rel_attn_fwd(b, "attn.", xna, pos, olens, B=B, T=T, H=L.attn.h, rel_mode=REL_LATEST, pa=pa,
                                 seed=sd(3))
        ops.linear(O, b.w("attn.linear_out.weight"), xc[:, :d],
                   epi=ops.make_epi(EPI_STORE, bias=b.f("attn.linear_out.bias"), drop_p=p, seed=sd(4)))
        # ---- branch 2: convolutional gating MLP (:149-157, cgmlp.py:110-118)
        G = "cgmlp."
        U = L.cgmlp.linear_units
        C = U // 2
        Kc = L.cgmlp.csgu.kernel_size
        xnm, mum, rsm = ln_fwd(x1, b, "norm_mlp", cd)
        h = empty(N, U, dtype=cd, device=dev)  # channel_proj1's pre-activation; gelu(h) is never stored
        ops.linear(xnm, b.w(G + "channel_proj1.0.weight"), h, epi=ops.make_epi(bias=b.f(G + "channel_proj1.0.bias")))
        gmu = empty(N, device=dev)
        grs = empty(N, device=dev)
        lib.ea_csgu_stats(N, U, h.data_ptr(), ops.dt(h), 1e-12, gmu.data_ptr(), grs.data_ptr(), ops.stream())
        gout = empty(N, C, dtype=cd, device=dev)
        lib.ea_csgu_fwd(B, T, U, Kc, h.data_ptr(), ops.dt(h), gmu.data_ptr(), grs.data_ptr(),
                        b.f(G + "csgu.norm.weight").data_ptr(), b.f(G + "csgu.norm.bias").data_ptr(),
                        b.f(G + "csgu.conv.weight").data_ptr(), b.f(G + "csgu.conv.bias").data_ptr(),
                        float(pg), sd(5), gout.data_ptr(), ops.stream())
        ops.linear(gout, b.w(G + "channel_proj2.weight"), xc[:, d:],
                   epi=ops.make_epi(EPI_STORE, bias=b.f(G + "channel_proj2.bias"), drop_p=p, seed=sd(6)))
        # ---- merge (:160-164): x = x + dropout(merge_proj(x_concat + dwconv(x_concat)))
        Km = L.merge_conv_kernel
        m = empty(N, 2 * d, dtype=cd, device=dev)
        lib.ea_merge_conv_fwd(B, T, 2 * d, Km, xc.data_ptr(), ops.dt(xc), b.f("depthwise_conv_fusion.weight").data_ptr(),
                              b.f("depthwise_conv_fusion.bias").data_ptr(), m.data_ptr(), ops.stream())
        x2 = empty(N, d, device=dev)
        ops.linear(m, b.w("merge_proj.weight"), x2,
                   epi=ops.make_epi(EPI_RESID, bias=b.f("merge_proj.bias"), resid=x1, drop_p=p, seed=sd(7)))
        # ---- FFN (:166-170) + norm_final (:172)
        x3, s_ff2 = ffn_fwd(b, x2, "feed_forward", "norm_ff", seed_in=sd(8), seed_out=sd(9), **ff)
        out, muf, rsf = ln_fwd(x3, b, "norm_final", F32)
        ctx.L = L
        ctx.meta = (B, T, d, p, pa, pg, seed)
        ctx.save = (x0, x1, x2, x3, s_ff1, (xna, mua, rsa, O, s_core), (xnm, mum, rsm, h, gmu, grs, gout), (xc, m),
                    s_ff2, (muf, rsf), pos, olens)
        return out.view(B, T, d)

    @staticmethod
    def backward(ctx, dout):
        L = ctx.L
        b = L._b
        cd = b.cd
        B, T, d, p, pa, pg, seed = ctx.meta
        (x0, x1, x2, x3, s_ff1, s_att, s_mlp, (xc, m), s_ff2, (muf, rsf), pos, olens) = ctx.save
        ctx.save = None
        li = L.layer_idx
        sd = lambda s: site_seed(seed, li, s)  # noqa: E731
        macaron = L.feed_forward_macaron is not None
        ff = dict(act=ACT_SWISH, p_in=p, p_out=p, rscale=L.ff_scale)
        N = B * T
        dev = dout.device
        dx = empty(N, d, device=dev)
        dv_ff2 = dv_buf(N, d, cd, dev)
        ln_bwd(dout.reshape(N, d).contiguous(), x3, b, "norm_final", muf, rsf, dx, accumulate=False,
               drop=drop_arg(dv_ff2, L.ff_scale, p, sd(9), b.g("feed_forward.w_2.bias")))
        # ---- FFN
        dv_mg = dv_buf(N, d, cd, dev)
        ffn_bwd(b, dx, x2, s_ff2, "feed_forward", "norm_ff", seed_in=sd(8), seed_out=sd(9), dv_in=dv_ff2,
                next_drop=drop_arg(dv_mg, 1.0, p, sd(7), b.g("merge_proj.bias")), **ff)
        # ---- merge: dm = dv . W_merge, dxc = (dm + dwconv^T(dm)) * the two branch dropout masks
        dv = site_dv(dx, dv_mg, b.g("merge_proj.bias"), 1.0, p, sd(7), cd)
        with ops.wgrad(dv, m):
            ops.linear_dw(dv, m, b.g("merge_proj.weight"), accumulate=True)
        dm = empty(N, 2 * d, dtype=cd, device=dev)
        ops.linear_dx(dv, b.w("merge_proj.weight"), dm)
        del m
        Km = L.merge_conv_kernel
        n_ws = _long()
        lib.ea_merge_conv_bwd_ws_elems(B, T, 2 * d, Km, ctypes.addressof(n_ws))
        w, wn = ops.f32_ws(dev, n_ws.value)
        dxc = empty(N, 2 * d, dtype=cd, device=dev)
        lib.ea_merge_conv_bwd(B, T, 2 * d, Km, xc.data_ptr(), dm.data_ptr(), ops.dt(dm),
                              b.f("depthwise_conv_fusion.weight").data_ptr(), float(p), sd(4), sd(6), dxc.data_ptr(),
                              b.g("depthwise_conv_fusion.weight").data_ptr(),
                              b.g("depthwise_conv_fusion.bias").data_ptr(), 1, w, wn, ops.stream())
        del dm, xc
        # ---- branch 2: cgMLP
        G = "cgmlp."
        U = L.cgmlp.linear_units
        C = U // 2
        Kc = L.cgmlp.csgu.kernel_size
        xnm, mum, rsm, h, gmu, grs, gout = s_mlp
        dv2 = dxc[:, d:]
        with ops.wgrad(dxc, gout):
            ops.linear_dw(dv2, gout, b.g(G + "channel_proj2.weight"), accumulate=True,
                          db=b.g(G + "channel_proj2.bias"))
        dgout = empty(N, C, dtype=cd, device=dev)
        ops.linear_dx(dv2, b.w(G + "channel_proj2.weight"), dgout)
        n_dln, n_ws = _long(), _long()
        lib.ea_csgu_bwd_ws_elems(B, T, U, Kc, ctypes.addressof(n_dln), ctypes.addressof(n_ws))
        dln = empty(n_dln.value, device=dev)
        w, wn = ops.f32_ws(dev, n_ws.value)
        dh = empty(N, U, dtype=cd, device=dev)
        lib.ea_csgu_bwd(B, T, U, Kc, dgout.data_ptr(), h.data_ptr(), ops.dt(h), gmu.data_ptr(), grs.data_ptr(),
                        b.f(G + "csgu.norm.weight").data_ptr(), b.f(G + "csgu.norm.bias").data_ptr(),
                        b.f(G + "csgu.conv.weight").data_ptr(), b.f(G + "csgu.conv.bias").data_ptr(),
                        float(pg), sd(5), dh.data_ptr(),
                        b.g(G + "csgu.norm.weight").data_ptr(), b.g(G + "csgu.norm.bias").data_ptr(),
                        b.g(G + "csgu.conv.weight").data_ptr(), b.g(G + "csgu.conv.bias").data_ptr(), 1,
                        dln.data_ptr(), w, wn, ops.stream())
        del dln, dgout
        with ops.wgrad(dh, xnm):
            ops.linear_dw(dh, xnm, b.g(G + "channel_proj1.0.weight"), accumulate=True,
                          db=b.g(G + "channel_proj1.0.bias"))
        dxnm = empty(N, d, dtype=cd, device=dev)
        ops.linear_dx(dh, b.w(G + "channel_proj1.0.weight"), dxnm)
        ln_bwd(dxnm, x1, b, "norm_mlp", mum, rsm, dx, accumulate=True)
        # ---- branch 1: rel-pos MHSA
        xna, mua, rsa, O, s_core = s_att
        dv1 = dxc[:, :d]
        with ops.wgrad(dxc, O):
            ops.linear_dw(dv1, O, b.g("attn.linear_out.weight"), accumulate=True,
                          db=b.g("attn.linear_out.bias"))
        dO = empty(N, d, dtype=cd, device=dev)
        ops.linear_dx(dv1, b.w("attn.linear_out.weight"), dO)
        dxna = rel_attn_bwd(b, "attn.", dO, xna, O, s_core, pos, olens, B=B, T=T, H=L.attn.h, rel_mode=REL_LATEST,
                            pa=pa, seed=sd(3))
        if macaron:
            dv_ff1 = dv_buf(N, d, cd, dev)
            ln_bwd(dxna, x1, b, "norm_mha", mua, rsa, dx, accumulate=True,
                   drop=drop_arg(dv_ff1, L.ff_scale, p, sd(2), b.g("feed_forward_macaron.w_2.bias")))
            ffn_bwd(b, dx, x0, s_ff1, "feed_forward_macaron", "norm_ff_macaron", seed_in=sd(1), seed_out=sd(2),
                    dv_in=dv_ff1, **ff)
        else:
            ln_bwd(dxna, x1, b, "norm_mha", mua, rsa, dx, accumulate=True)
        ops.grad_ready(b)
        return dx.view(B, T, d), None, None, None, None, None
