"""TransducerDecoder — drop-in for espnet2/asr/decoder/transducer_decoder.py: the label decoder of
the `decoder: transducer` recipes, an embedding and a stack of one-layer LSTMs.

Same constructor, defaults, state_dict keys (embed.weight, decoder.{k}.weight_ih_l0, ...) and
parameter creation order.  Built: rnn_type lstm, the training forward.  gru raises
NotImplementedError; score / batch_score / beam search belong to transducer decoding, which is not
built.

Training forward over (B, U1) labels (time-major rows u * B + b inside, f32 between the nodes, bf16
matrix operands under amp), all on lm/rnn_train.py's nodes:

    EmbedFn (+ DropFn dropout_embed)     the padding row embed_pad receives no gradient
    LSTMLayerFn (+ DropFn dropout) x N   zero initial state

Steps past a label sequence's length are computed and ignored by the loss, as in the reference.
"""
from __future__ import annotations

import torch

from ...layers.common import Bound, site_seed
from ...lm.rnn_train import DropFn, EmbedFn, EmbedTable, LSTMLayer, LSTMLayerFn
from .transformer_decoder import AbsDecoder


class TransducerDecoder(AbsDecoder):
    def __init__(self, vocab_size: int, rnn_type: str = "lstm", num_layers: int = 1, hidden_size: int = 320,
                 dropout: float = 0.0, dropout_embed: float = 0.0, embed_pad: int = 0):
        if rnn_type not in {"lstm", "gru"}:
            raise ValueError(f"Not supported: rnn_type={rnn_type}")
        if rnn_type != "lstm":
            raise NotImplementedError(f"espnet_amd TransducerDecoder: rnn_type={rnn_type!r} is not built "
                                      "(only rnn_type='lstm')")
        super().__init__()
        # creation order of transducer_decoder.py:43-56
        self.embed = torch.nn.Embedding(vocab_size, hidden_size, padding_idx=embed_pad)
        self.dropout_embed = torch.nn.Dropout(p=dropout_embed)
        self.decoder = torch.nn.ModuleList([torch.nn.LSTM(hidden_size, hidden_size, 1, batch_first=True)
                                            for _ in range(num_layers)])
        self.dropout_dec = torch.nn.ModuleList([torch.nn.Dropout(p=dropout) for _ in range(num_layers)])
        self.dlayers = num_layers
        self.dunits = hidden_size
        self.dtype = rnn_type
        self.odim = vocab_size
        self.ignore_id = -1
        self.blank_id = embed_pad
        self._b = None

    def set_device(self, device):
        self.device = device

    # ------------------------------------------------------------------ binding
    def arena_groups(self, prefix=""):
        return []

    def bind(self, arena, prefix, cd):
        self._b = b = Bound(arena, prefix, cd)
        self._embed = EmbedTable(self.embed, arena.device)
        self._layers = [LSTMLayer(rnn, b.w(f"decoder.{k}.weight_ih_l0"), cd, k=0) for k, rnn in enumerate(self.decoder)]
        self._anchor = torch.zeros(1, device=arena.device, requires_grad=True)
        arena.update_hooks.append(self._weights_changed)
        self._weights_changed()

    def _weights_changed(self):
        for lay in self._layers:
            lay.refresh()

    # ------------------------------------------------------------------ training
    def forward(self, labels: torch.Tensor, seed: int = 0) -> torch.Tensor:
        """labels (B, U1), blank first -> dec_out (B, U1, D_dec) f32."""
        if self._b is None:
            raise RuntimeError("TransducerDecoder: bind(arena, prefix, cd) first (ESPnetASRModel.prepare)")
        B, L = labels.shape
        if B == 0 or L == 0:
            raise ValueError(f"empty batch: {tuple(labels.shape)}")
        dev = self._embed.weight.device
        tok = labels.to(dev, torch.long).t().clamp(0, self.odim - 1).contiguous().view(-1)  # row u * B + b
        pe = float(self.dropout_embed.p) if self.training else 0.0
        x = EmbedFn.apply(self._anchor, tok, self._embed)
        if pe > 0.0:
            x = DropFn.apply(x, pe, site_seed(seed, 710, 0))
        for k, lay in enumerate(self._layers):
            x, _, _ = LSTMLayerFn.apply(x, lay, L, B, None, None)
            p = float(self.dropout_dec[k].p) if self.training else 0.0
            if p > 0.0:
                x = DropFn.apply(x, p, site_seed(seed, 711, k))
        return x.view(L, B, self.dunits).transpose(0, 1)

    def score(self, *args, **kwargs):
        raise NotImplementedError("espnet_amd TransducerDecoder: transducer decoding (score / beam search) is not built")

    batch_score = score
