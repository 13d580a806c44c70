"""VGGRNNEncoder — drop-in for espnet2/asr/encoder/vgg_rnn_encoder.py: the VGG2L front end of
espnet/nets/pytorch_backend/rnn/encoders.py:178-237 before the RNNP / RNN of `encoder: rnn`
(rnn_encoder.py, unchanged).  The encoder of the `encoder: vgg_rnn` recipes.

Same constructor, defaults, module names, state_dict keys and parameter creation order: enc.0 is
VGG2L (conv1_1, conv1_2, conv2_1, conv2_2 as torch.nn.Conv2d), enc.1 the RNNP or RNN over
idim = 128 * ceil(ceil(F / 2) / 2); subsample is all ones.  rnn_type gru, prev_states and
in_channel != 1 raise NotImplementedError.

VGG2L forward, activations channel-last (B, T, F, C) in the compute dtype:

    conv1_1   ea_vgg_conv1_fwd, a vector kernel (Cin = 1), f32 weights in both dtypes, + ReLU
    conv1_2   ea_vgg_conv3x3, implicit GEMM; bias + ReLU + the 2x2 ceil-mode pool in its epilogue,
              which stores the pooled map and one decision byte per pooled element
    conv2_1   ea_vgg_conv3x3 + ReLU
    conv2_2   as conv1_2; its epilogue stores f32 in the reference's feature order c * F' + f and
              time-major rows t * B + b, what the LSTM layers read

Nothing is masked here: the convolutions see whatever the padded frames hold, as the reference's do.
The backward runs each input gradient as the same kernel over the transposed weight with flipped
taps, reads the pooled layers' gradients through the saved decisions in the operand loaders (no
full-resolution gradient of a pooled layer is written), and sums the weight gradients from
pixel-range partials in a fixed order.  No gradient is produced for the features.  The lengths
stay on the device (l -> ceil(ceil(l / 2) / 2)) and the time extent follows from the padded T.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from ..._lib import _DT, ENUMS, VGG_EPI_MASK, VGG_EPI_NONE, VGG_EPI_POOL, VGG_EPI_RELU, VGG_SRC_PLAIN, VGG_SRC_POOLED
from ...layers.common import Bound, empty, lib, ops
from .abs_encoder import AbsEncoder
from .rnn_encoder import RNN, RNNP

_NOT_BUILT = "espnet_amd VGGRNNEncoder: {} is not built"
_GEMM_LAYERS = ("conv1_2", "conv2_1", "conv2_2")


def get_vgg2l_odim(idim: int, in_channel: int = 1, out_channel: int = 128) -> int:
    """The feature size after VGG2L: two ceil-mode halvings of idim / in_channel, times 128."""
    f = idim // in_channel
    return -(-(-(-f // 2)) // 2) * out_channel


def _half(n):
    return (n + 1) // 2


def _nhwc_strides(H, W, C):
    return H * W * C, W * C, C, 1  # b, h, w, c


class _Geo:
    """The geo / strides arrays of the ea_vgg_* entry points (EA_VGG_* of the header)."""

    def __init__(self, B, H, W, cin, cout, *, src=VGG_SRC_PLAIN, epi=VGG_EPI_NONE, flip=0, out_dtype=torch.float32,
                 ps=(0, 0, 0, 0), po=(0, 0, 0, 0)):
        self.cin, self.cout = cin, cout
        geo = {"B": B, "H": H, "W": W, "CIN": cin, "COUT": cout, "SRC": src, "EPI": epi, "FLIP": flip,
               "OUT_DTYPE": _DT[out_dtype]}
        self.geo = (ctypes.c_int * ENUMS["EA_VGG_NGEO"])()
        for k, v in geo.items():
            self.geo[ENUMS["EA_VGG_" + k]] = v
        self.strides = (ctypes.c_long * ENUMS["EA_VGG_NSTRIDE"])()
        for pre, vals in (("PS_", ps), ("PO_", po)):
            for k, v in zip("BHWC", vals):
                self.strides[ENUMS["EA_VGG_" + pre + k]] = v



def _conv(g, cd, x, dp, dec, w, bias, aux, out, dec_out):
    lib.ea_vgg_conv3x3(g.geo, g.strides, _DT[cd], ops.ptr(x), ops.ptr(dp), ops.ptr(dec), w.data_ptr(),
                       ops.ptr(bias), ops.ptr(aux), out.data_ptr(), ops.ptr(dec_out), ops.stream())


class VGG2L(torch.nn.Module):
    """encoders.py:178-237.  Parameters created in the reference's order."""

    def __init__(self, in_channel: int = 1):
        super().__init__()
        if in_channel != 1:
            raise NotImplementedError(_NOT_BUILT.format(f"in_channel={in_channel}") + " (only in_channel=1)")
        self.conv1_1 = torch.nn.Conv2d(in_channel, 64, 3, stride=1, padding=1)
        self.conv1_2 = torch.nn.Conv2d(64, 64, 3, stride=1, padding=1)
        self.conv2_1 = torch.nn.Conv2d(64, 128, 3, stride=1, padding=1)
        self.conv2_2 = torch.nn.Conv2d(128, 128, 3, stride=1, padding=1)
        self.in_channel = in_channel
        # test hook: keep the last training forward's activations and decisions (and, after its
        # backward, the gradients between the layers) in _last
        self.keep_decisions = False
        self._b = None
        self._packs = None
        self._last = None

    def bind(self, arena, prefix, cd):
        self._b = Bound(arena, prefix, cd)
        dev = arena.data.device
        self._packs = {}
        for name in _GEMM_LAYERS:
            co, ci = getattr(self, name).weight.shape[:2]
            # forward (Co, 9, Ci) and input-gradient (Ci, 9, Co) operands in the compute dtype
            self._packs[name] = (empty(co, 9, ci, dtype=cd, device=dev), empty(ci, 9, co, dtype=cd, device=dev))

    def refresh(self):
        """After the weights changed: repack the GEMM operands, on the stream."""
        for name in _GEMM_LAYERS:
            w = self._b.w(f"{name}.weight")
            co, ci = getattr(self, name).weight.shape[:2]
            wp, wd = self._packs[name]
            ops.permute3(w, wp, co, ci, 9)  # (Co, Ci, 9) -> (Co, 9, Ci)
            ops.permute3(w, wd, 1, co, ci * 9)  # (Co, Ci * 9) -> (Ci, 9, Co); the kernel flips the taps

    def forward(self, xs_pad: torch.Tensor, lens: torch.Tensor, anchor):
        """xs_pad (B, T, F) f32, lens (B,) int64 on the device -> (x (T' * B, 128 * F') f32 time-major,
        lens', T')."""
        x = VGG2LFn.apply(xs_pad, anchor, self)
        lens = torch.div(torch.div(lens + 1, 2, rounding_mode="floor") + 1, 2, rounding_mode="floor")
        return x, lens, _half(_half(xs_pad.shape[1]))

    def _keep(self, key, **tensors):
        """The test hook's bookkeeping: with keep_decisions, a training-mode forward starts _last
        (it passes `shape`) and the backward of that same forward (key: its x1) adds to it."""
        if not self.keep_decisions:
            return
        if "shape" in tensors:
            self._last = dict(tensors) if self.training else None
        elif self._last is not None and self._last["x1"] is key:
            self._last.update(tensors)

    def decisions(self):
        """The decisions saved by the last training-mode forward (keep_decisions set before it), in
        the reference's NCHW layout: relu0..3 bool (pre-activation > 0 of conv1_1, conv1_2, conv2_1,
        conv2_2), pool0..1 int64 in 0..3 = 2 * dt + df of each window's winner."""
        if self._last is None:
            raise RuntimeError("VGG2L.decisions(): set keep_decisions and run a training-mode forward first")
        x1, dec1, x3, dec2, (B, H, W) = (self._last[k] for k in ("x1", "dec1", "x3", "dec2", "shape"))
        H2, W2 = _half(H), _half(W)
        H4, W4 = _half(H2), _half(W2)
        dec1 = dec1.view(B, H2, W2, 64).permute(0, 3, 1, 2).long()
        dec2 = dec2.view(H4, B, 128, W4).permute(1, 2, 0, 3).long()

        def relu_bits(dec, h, w):
            full = torch.zeros(*dec.shape[:2], 2 * dec.shape[2], 2 * dec.shape[3], dtype=torch.bool, device=dec.device)
            for pos in range(4):
                full[:, :, pos >> 1::2, pos & 1::2] = ((dec >> (2 + pos)) & 1).bool()
            return full[:, :, :h, :w]

        return dict(relu0=(x1.view(B, H, W, 64) > 0).permute(0, 3, 1, 2), relu1=relu_bits(dec1, H, W),
                    relu2=(x3.view(B, H2, W2, 128) > 0).permute(0, 3, 1, 2), relu3=relu_bits(dec2, H2, W2),
                    pool0=dec1 & 3, pool1=dec2 & 3)


def _wgrad(m, name, g, cd, x, dy, dp, dec):
    """name's weight gradient: pixel-range partials, summed in order, then (Co, 9, Ci) -> (Co, Ci, 9)
    into the gradient arena."""
    b = m._b
    co, ci = g.cout, g.cin
    n = ctypes.c_int(0)
    lib.ea_vgg_wgrad_splits(g.geo, ctypes.addressof(n))
    part = empty(n.value, co * 9 * ci, device=x.device)
    lib.ea_vgg_wgrad(g.geo, g.strides, _DT[cd], x.data_ptr(), ops.ptr(dy), ops.ptr(dp), ops.ptr(dec),
                     part.data_ptr(), n.value, ops.stream())
    dw = empty(co, 9 * ci, device=x.device)
    lib.ea_reduce_partials(n.value, co * 9 * ci, part.data_ptr(), co * 9 * ci, dw.data_ptr(), 0, ops.stream())
    ops.permute3(dw, b.g(f"{name}.weight"), co, 9, ci, accumulate=True)


def _pool_dbias(m, name, g, dp, dec, Q):
    nparts = max(1, min(256, Q // 64))
    part = empty(nparts, g.cout, device=dp.device)
    lib.ea_vgg_pool_dbias(g.geo, g.strides, dp.data_ptr(), dec.data_ptr(), part.data_ptr(), nparts, ops.stream())
    lib.ea_reduce_partials(nparts, g.cout, part.data_ptr(), g.cout, m._b.g(f"{name}.bias").data_ptr(), 1, ops.stream())


class VGG2LFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, anchor, m: VGG2L):
        b = m._b
        if b is None:
            raise RuntimeError("VGG2L: bind(arena, prefix, cd) first (ESPnetASRModel.prepare)")
        cd = b.cd
        feats = feats.float().contiguous()
        B, H, W = feats.shape
        H2, W2 = _half(H), _half(W)
        H4, W4 = _half(H2), _half(W2)
        dev = feats.device
        x1 = empty(B * H * W, 64, dtype=cd, device=dev)
        lib.ea_vgg_conv1_fwd(B, H, W, feats.data_ptr(), b.f("conv1_1.weight").data_ptr(),
                             b.f("conv1_1.bias").data_ptr(), x1.data_ptr(), ops.dt(x1), ops.stream())
        p1 = empty(B * H2 * W2, 64, dtype=cd, device=dev)
        dec1 = torch.empty(B * H2 * W2, 64, dtype=torch.uint8, device=dev)
        s1 = _nhwc_strides(H2, W2, 64)
        _conv(_Geo(B, H, W, 64, 64, epi=VGG_EPI_POOL, out_dtype=cd, po=s1), cd, x1, None, None,
              m._packs["conv1_2"][0], b.f("conv1_2.bias"), None, p1, dec1)
        x3 = empty(B * H2 * W2, 128, dtype=cd, device=dev)
        _conv(_Geo(B, H2, W2, 64, 128, epi=VGG_EPI_RELU, out_dtype=cd), cd, p1, None, None,
              m._packs["conv2_1"][0], b.f("conv2_1.bias"), None, x3, None)
        # rows t * B + b, columns c * F' + f: what RNNP / RNN read, in the reference's feature order
        out = empty(H4 * B, 128 * W4, device=dev)
        dec2 = torch.empty(H4 * B, 128 * W4, dtype=torch.uint8, device=dev)
        s2 = (128 * W4, B * 128 * W4, 1, W4)  # b, h, w, c
        _conv(_Geo(B, H2, W2, 128, 128, epi=VGG_EPI_POOL, out_dtype=torch.float32, po=s2), cd, x3, None, None,
              m._packs["conv2_2"][0], b.f("conv2_2.bias"), None, out, dec2)
        ctx.m = m
        ctx.meta = (B, H, W, s1, s2)
        ctx.save = (feats, x1, p1, dec1, x3, dec2)  # (dropped with the output when nothing records the node)
        m._keep(x1, x1=x1, p1=p1, dec1=dec1, x3=x3, out=out, dec2=dec2, shape=(B, H, W))
        return out

    @staticmethod
    def backward(ctx, dy):
        m = ctx.m
        b = m._b
        cd = b.cd
        B, H, W, s1, s2 = ctx.meta
        feats, x1, p1, dec1, x3, dec2 = ctx.save
        ctx.save = None
        H2, W2 = _half(H), _half(W)
        H4, W4 = _half(H2), _half(W2)
        dev = dy.device
        dy = dy.float().contiguous()
        # conv2_2: its gradient is dy through the second pool's decisions, read by the loaders
        g = _Geo(B, H2, W2, 128, 128, src=VGG_SRC_POOLED, ps=s2)
        _pool_dbias(m, "conv2_2", g, dy, dec2, B * H4 * W4)
        _wgrad(m, "conv2_2", g, cd, x3, None, dy, dec2)
        d3 = empty(B * H2 * W2, 128, dtype=cd, device=dev)  # d conv2_1 pre-activation
        _conv(_Geo(B, H2, W2, 128, 128, src=VGG_SRC_POOLED, epi=VGG_EPI_MASK, flip=1, out_dtype=cd, ps=s2), cd,
              None, dy, dec2, m._packs["conv2_2"][1], None, x3, d3, None)
        # conv2_1
        ops.colsum(d3, b.g("conv2_1.bias"), accumulate=True, defer=False)
        _wgrad(m, "conv2_1", _Geo(B, H2, W2, 64, 128), cd, p1, d3, None, None)
        dp1 = empty(B * H2 * W2, 64, device=dev)  # d pooled map of conv1_2, f32
        _conv(_Geo(B, H2, W2, 128, 64, flip=1), cd, d3, None, None, m._packs["conv2_1"][1], None, None, dp1, None)
        # conv1_2, through the first pool's decisions
        g = _Geo(B, H, W, 64, 64, src=VGG_SRC_POOLED, ps=s1)
        _pool_dbias(m, "conv1_2", g, dp1, dec1, B * H2 * W2)
        _wgrad(m, "conv1_2", g, cd, x1, None, dp1, dec1)
        d1 = empty(B * H * W, 64, dtype=cd, device=dev)  # d conv1_1 pre-activation
        _conv(_Geo(B, H, W, 64, 64, src=VGG_SRC_POOLED, epi=VGG_EPI_MASK, flip=1, out_dtype=cd, ps=s1), cd,
              None, dp1, dec1, m._packs["conv1_2"][1], None, x1, d1, None)
        # conv1_1: weight and bias gradients only, no gradient for the features
        P = B * H * W
        nparts = max(1, min(1024, P // 64))
        part = empty(nparts, 640, device=dev)
        lib.ea_vgg_conv1_wgrad(B, H, W, feats.data_ptr(), d1.data_ptr(), ops.dt(d1), part.data_ptr(), nparts,
                               ops.stream())
        lib.ea_reduce_partials(nparts, 576, part.data_ptr(), 640, b.g("conv1_1.weight").data_ptr(), 1, ops.stream())
        lib.ea_reduce_partials(nparts, 64, part.data_ptr() + 4 * 576, 640, b.g("conv1_1.bias").data_ptr(), 1,
                               ops.stream())
        m._keep(x1, d3=d3, dp1=dp1, d1=d1)
        return None, None, None


class VGGRNNEncoder(AbsEncoder):
    def __init__(
        self,
        input_size: int,
        rnn_type: str = "lstm",
        bidirectional: bool = True,
        use_projection: bool = True,
        num_layers: int = 4,
        hidden_size: int = 320,
        output_size: int = 320,
        dropout: float = 0.0,
        in_channel: int = 1,
    ):
        super().__init__()
        self._output_size = output_size
        self.rnn_type = rnn_type
        self.bidirectional = bidirectional
        self.use_projection = use_projection
        if rnn_type not in {"lstm", "gru"}:
            raise ValueError(f"Not supported rnn_type={rnn_type}")
        if rnn_type != "lstm":
            raise NotImplementedError(_NOT_BUILT.format(f"rnn_type={rnn_type!r}") + " (only rnn_type='lstm')")
        if in_channel != 1:
            raise NotImplementedError(_NOT_BUILT.format(f"in_channel={in_channel}") + " (only in_channel=1)")
        subsample = [1] * (num_layers + 1)  # vgg_rnn_encoder.py:48: not used for VGGRNN
        typ = ("b" if bidirectional else "") + rnn_type
        idim = get_vgg2l_odim(input_size, in_channel=in_channel)
        vgg = VGG2L(in_channel)  # created first, as in the reference's list: a seeded build is identical
        if use_projection:
            rnn = RNNP(idim, num_layers, hidden_size, output_size, subsample, dropout, typ=typ)
        else:
            rnn = RNN(idim, num_layers, hidden_size, output_size, dropout, typ=typ)
        self.enc = torch.nn.ModuleList([vgg, rnn])
        self._anchor = None

    def output_size(self) -> int:
        return self._output_size

    # ------------------------------------------------------------------ binding
    def arena_groups(self, prefix=""):
        return []

    def bind(self, arena, prefix, cd, anchor):
        for i, m in enumerate(self.enc):
            m.bind(arena, f"{prefix}enc.{i}.", cd)
        self._anchor = anchor
        arena.update_hooks.append(self._weights_changed)
        self._weights_changed()

    def _weights_changed(self):
        self.enc[0].refresh()
        for lay in self.enc[1].lstm_layers():
            lay.refresh()

    # ------------------------------------------------------------------ forward
    def forward(self, xs_pad: torch.Tensor, ilens: torch.Tensor, prev_states=None,
                seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        """vgg_rnn_encoder.py:85-104.  xs_pad (B, T, F) f32 on the GPU, ilens (B,) -> ((B, T', D), olens, None)."""
        if prev_states is not None:
            raise NotImplementedError(_NOT_BUILT.format("prev_states (streaming)"))
        if self._anchor is None:
            raise RuntimeError("VGGRNNEncoder: bind(arena, prefix, cd, anchor) first (ESPnetASRModel.prepare)")
        B, T, _ = xs_pad.shape
        if B == 0 or T == 0:
            raise ValueError(f"empty batch: {tuple(xs_pad.shape)}")
        lens = ilens.to(xs_pad.device, torch.long).contiguous()
        x, lens, T = self.enc[0](xs_pad, lens, self._anchor)
        x, lens, T = self.enc[1](x, lens, T, B, self._anchor, seed=seed)
        out = x.view(T, B, -1).transpose(0, 1)
        pad = torch.arange(T, device=out.device)[None, :] >= lens[:, None]
        return out.masked_fill(pad.unsqueeze(-1), 0.0).contiguous(), lens, None
