"""RNNEncoder — drop-in for espnet2/asr/encoder/rnn_encoder.py: the BLSTM / BLSTMP encoder of the
`encoder: rnn` recipes, RNN and RNNP of espnet/nets/pytorch_backend/rnn/encoders.py.

Same constructor, defaults, module names, state_dict keys and parameter creation order (a seeded
build is bit-identical; a reference checkpoint loads): use_projection=True is RNNP (enc.0.birnn{i}
or enc.0.rnn{i}, one-layer torch.nn.LSTMs, and enc.0.bt{i}), use_projection=False is RNN
(enc.0.nbrnn, a multi-layer torch.nn.LSTM, and enc.0.l_last).  RNN and RNNP take idim, so a front
end (VGG2L) can be put before them.  Built: rnn_type lstm, one or two directions, any num_layers /
hidden_size / output_size / subsample / dropout.  rnn_type gru and prev_states (streaming) raise
NotImplementedError.

Forward (time-major rows t * B + b, f32 between the nodes, bf16 matrix operands under amp):

    BiLSTMLayerFn        one (bi)directional layer: the input projection of all steps is one GEMM
                         per direction, the recurrence T launches of ea_lstm_bicell_fwd carrying
                         both directions, masked by the lengths in device memory (lm/rnn_train.py)
    [::sub], len update  after layer i with subsample[i + 1] > 1 (RNNP)
    OutLinearFn          bt{i} / l_last; DropFn (RNNP: after every projection but the last, active
                         in eval mode too, as the reference's F.dropout without `training=`; RNN:
                         nn.LSTM's inter-layer dropout, training only); TanhFn
    masked_fill          frames past the output length are exactly 0

The lengths stay on the device: the forward and the backward make no host synchronisation, and
the kernels need no sorting by length.  Two differences from the reference follow:
the output's time extent follows from the padded input extent T by the subsampling law (T ->
ceil(T / sub) per layer), not from max(ilens) (pad_packed_sequence trims to it), so it equals the
reference's whenever max(ilens) == T, which is what the collate function produces; and a row
whose length reaches 0 is all masked, where pack_padded_sequence raises.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ...layers.common import Bound, site_seed
from ...lm.rnn_train import BiLSTMLayerFn, DropFn, LinearHead, LSTMLayer, OutLinearFn, TanhFn
from .abs_encoder import AbsEncoder

_NOT_BUILT = "espnet_amd RNNEncoder: {} is not built"


def _lstm_only(typ: str):
    if "lstm" not in typ:
        raise NotImplementedError(_NOT_BUILT.format(f"rnn_type={typ.lstrip('b')!r}") + " (only rnn_type='lstm')")


def _directions(rnn, b: Bound, name: str, k: int, cd):
    """The LSTMLayer of each direction of layer k of the nn.LSTM `name`."""
    sfx = ["", "_reverse"] if rnn.bidirectional else [""]
    return [LSTMLayer(rnn, b.w(f"{name}.weight_ih_l{k}{s}"), cd, k=k, reverse=bool(s)) for s in sfx]


class RNNP(torch.nn.Module):
    """RNN with projection layers (encoders.py:13-91).  Parameters created in the reference's order."""

    def __init__(self, idim, elayers, cdim, hdim, subsample, dropout, typ="blstm"):
        super().__init__()
        _lstm_only(typ)
        bidir = typ[0] == "b"
        for i in range(elayers):
            inputdim = idim if i == 0 else hdim
            rnn = torch.nn.LSTM(inputdim, cdim, num_layers=1, bidirectional=bidir, batch_first=True)
            setattr(self, "%s%d" % ("birnn" if bidir else "rnn", i), rnn)
            setattr(self, "bt%d" % i, torch.nn.Linear(2 * cdim if bidir else cdim, hdim))
        self.elayers = elayers
        self.cdim = cdim
        self.subsample = subsample
        self.typ = typ
        self.bidir = bidir
        self.dropout = dropout
        self._layers = None

    def bind(self, arena, prefix, cd):
        b = Bound(arena, prefix, cd)
        name = "birnn" if self.bidir else "rnn"
        self._layers = [_directions(getattr(self, f"{name}{i}"), b, f"{name}{i}", 0, cd) for i in range(self.elayers)]
        self._heads = [LinearHead(getattr(self, f"bt{i}"), b.w(f"bt{i}.weight"), cd) for i in range(self.elayers)]

    def lstm_layers(self):
        return [lay for dirs in self._layers for lay in dirs]

    def dropout_seeds(self, seed: int):
        """The ea_scale_dropout stream of layer i's projection output, (T_i * B, hdim) time-major."""
        return [site_seed(seed, 710, i) for i in range(self.elayers)]

    def forward(self, x, lens, T, B, anchor, seed=0):
        """x (T * B, idim) f32 time-major, lens (B,) int64 on the device -> (x (T' * B, hdim), lens', T')."""
        p, seeds = float(self.dropout), self.dropout_seeds(seed)
        for i in range(self.elayers):
            x = BiLSTMLayerFn.apply(x, self._layers[i], lens, T, B, anchor if i == 0 else None)
            sub = int(self.subsample[i + 1])
            if sub > 1:
                x = x.view(T, B, -1)[::sub]
                T = x.shape[0]
                x = x.reshape(T * B, -1)
                lens = torch.div(lens + 1, sub, rounding_mode="floor")
            x = OutLinearFn.apply(x, self._heads[i])
            if i < self.elayers - 1:
                if p > 0.0:  # F.dropout(xs_pad, p=self.dropout): active in eval mode too
                    x = DropFn.apply(x, p, seeds[i])
                x = TanhFn.apply(x)
        return x, lens, T


class RNN(torch.nn.Module):
    """RNN without per-layer projections (encoders.py:94-162)."""

    def __init__(self, idim, elayers, cdim, hdim, dropout, typ="blstm"):
        super().__init__()
        _lstm_only(typ)
        bidir = typ[0] == "b"
        self.nbrnn = torch.nn.LSTM(idim, cdim, elayers, batch_first=True, dropout=dropout, bidirectional=bidir)
        self.l_last = torch.nn.Linear(cdim * 2 if bidir else cdim, hdim)
        self.typ = typ
        self.elayers = elayers
        self.dropout = dropout
        self._layers = None

    def bind(self, arena, prefix, cd):
        b = Bound(arena, prefix, cd)
        self._layers = [_directions(self.nbrnn, b, "nbrnn", k, cd) for k in range(self.elayers)]
        self._head = LinearHead(self.l_last, b.w("l_last.weight"), cd)

    def lstm_layers(self):
        return [lay for dirs in self._layers for lay in dirs]

    def dropout_seeds(self, seed: int):
        """The stream of nn.LSTM's dropout on layer k's output (k < elayers - 1), (T * B, ndir * cdim)."""
        return [site_seed(seed, 711, k) for k in range(self.elayers - 1)]

    def forward(self, x, lens, T, B, anchor, seed=0):
        p, seeds = (float(self.dropout) if self.training else 0.0), self.dropout_seeds(seed)
        for k in range(self.elayers):
            x = BiLSTMLayerFn.apply(x, self._layers[k], lens, T, B, anchor if k == 0 else None)
            if p > 0.0 and k < self.elayers - 1:
                x = DropFn.apply(x, p, seeds[k])
        return TanhFn.apply(OutLinearFn.apply(x, self._head)), lens, T


class RNNEncoder(AbsEncoder):
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
        subsample: Optional[Sequence[int]] = (2, 2, 1, 1),
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
        if subsample is None:
            subsample = np.ones(num_layers + 1, dtype=np.int64)
        else:  # rnn_encoder.py:48-58: truncated to the layers, 1 put in front, padded with 1
            subsample = list(subsample)[:num_layers]
            subsample = np.pad(np.array(subsample, dtype=np.int64), [1, num_layers - len(subsample)],
                               mode="constant", constant_values=1)
        typ = ("b" if bidirectional else "") + rnn_type
        if use_projection:
            self.enc = torch.nn.ModuleList([RNNP(input_size, num_layers, hidden_size, output_size, subsample,
                                                 dropout, typ=typ)])
        else:
            self.enc = torch.nn.ModuleList([RNN(input_size, num_layers, hidden_size, output_size, dropout, typ=typ)])
        self._anchor = None

    def output_size(self) -> int:
        return self._output_size

    # ------------------------------------------------------------------ binding
    def arena_groups(self, prefix=""):
        return []  # no fused weights: every GEMM reads one parameter

    def bind(self, arena, prefix, cd, anchor):
        for i, m in enumerate(self.enc):
            m.bind(arena, f"{prefix}enc.{i}.", cd)
        self._anchor = anchor
        arena.update_hooks.append(self._weights_changed)
        self._weights_changed()

    def _weights_changed(self):
        for m in self.enc:
            for lay in m.lstm_layers():
                lay.refresh()

    # ------------------------------------------------------------------ forward
    def forward(self, xs_pad: torch.Tensor, ilens: torch.Tensor, prev_states=None,
                seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        """rnn_encoder.py:93-112.  xs_pad (B, T, F) f32 on the GPU, ilens (B,) -> ((B, T', D), olens, None)."""
        if prev_states is not None:
            raise NotImplementedError(_NOT_BUILT.format("prev_states (streaming)"))
        if self._anchor is None:
            raise RuntimeError("RNNEncoder: bind(arena, prefix, cd, anchor) first (ESPnetASRModel.prepare)")
        B, T, _ = xs_pad.shape
        if B == 0 or T == 0:
            raise ValueError(f"empty batch: {tuple(xs_pad.shape)}")
        lens = ilens.to(xs_pad.device, torch.long).contiguous()
        x = xs_pad.float().transpose(0, 1).reshape(T * B, -1)
        for m in self.enc:
            x, lens, T = m(x, lens, T, B, self._anchor, seed=seed)
        out = x.view(T, B, -1).transpose(0, 1)
        pad = torch.arange(T, device=out.device)[None, :] >= lens[:, None]
        return out.masked_fill(pad.unsqueeze(-1), 0.0).contiguous(), lens, None
