"""TransducerDecoder — drop-in for espnet2/asr/decoder/transducer_decoder.py: the label decoder of
the `decoder: transducer` recipes, an embedding and a stack of one-layer LSTMs.

Same constructor, defaults, state_dict keys (embed.weight, decoder.{k}.weight_ih_l0, ...) and
parameter creation order.  Built: rnn_type lstm, the training forward and the decoding interface
(init_state, score, batch_score, select_state, create_batch_states, with the label-sequence cache).  gru
raises NotImplementedError.

Training forward over (B, U1) labels (time-major rows u * B + b inside, f32 between the nodes, bf16
matrix operands under amp), all on lm/rnn_train.py's nodes:

    EmbedFn (+ DropFn dropout_embed)     the padding row embed_pad receives no gradient
    LSTMLayerFn (+ DropFn dropout) x N   zero initial state

Steps past a label sequence's length are computed and ignored by the loss, as in the reference.

Decoding (eval mode, asr/transducer/beam_search_transducer.py): step() runs one label of n hypotheses on the
fused step kernel ea_lstm_step, one launch per layer, on operands packed as lm/seq_rnn_lm.py packs them (the
embedding table with padded rows, the [W_ih | W_hh] tile pack in the compute dtype).  A step's states live in
one (2, N, n, Hp) buffer; the (N, n, D_dec) states handed out are views of it.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import torch

from ... import hip_ops as ops
from ..._lib import BF16, F32, lib
from ...layers.common import Bound, site_seed
from ...lm.lstm_pack import pack_lstm_bias, pack_lstm_weights, rup
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
        self.device = torch.device("cpu")
        self._b = self._dec = None

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
        self.device = arena.device
        arena.update_hooks.append(self._weights_changed)
        self._weights_changed()
        if not self.__dict__.get("_hooked", False):
            self.register_load_state_dict_post_hook(lambda m, _: m.__dict__.update(_dec=None))
            self.__dict__["_hooked"] = True

    def _weights_changed(self):
        for lay in self._layers:
            lay.refresh()
        self._dec = None  # the decoding packs: rebuilt at the next decoding call

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

    # ------------------------------------------------------------------ decoding (transducer_decoder.py:77-298)
    def init_state(self, batch_size: int):
        """-> zero states ((N, B, D_dec), (N, B, D_dec))."""
        z = torch.zeros(2, self.dlayers, batch_size, self.dunits, device=self.device)
        return z[0], z[1]

    def _packs(self):
        """The step kernel's operands, made at the first decoding call after the weights changed."""
        if self._b is None:
            raise RuntimeError("TransducerDecoder: bind(arena, prefix, cd) first (ESPnetASRModel.prepare)")
        if self.training:
            raise RuntimeError("TransducerDecoder: decoding runs in eval mode (no dropout in the step kernel)")
        if self._dec is None:
            with torch.no_grad():
                emb = torch.zeros(self.odim, rup(self.dunits), device=self._embed.weight.device)
                emb[:, :self.dunits] = self.embed.weight.detach()
                self._dec = (emb, [pack_lstm_weights(r.weight_ih_l0, r.weight_hh_l0, self._b.cd) for r in self.decoder],
                             [pack_lstm_bias(r.bias_ih_l0, r.bias_hh_l0) for r in self.decoder])
        return self._dec

    def step(self, tokens: torch.Tensor, state):
        """One label of n hypotheses through the layers: tokens (n) int64 on the device, state ((N, n, D_dec),
        (N, n, D_dec)) -> (dec_out (n, D_dec), the new state).  One ea_lstm_step launch per layer; layer 0
        reads its rows from the embedding table by token id."""
        emb, wpack, bias = self._packs()
        n, L, H, Hp = tokens.shape[0], self.dlayers, self.dunits, emb.shape[1]
        h, c = (t if t.dtype == torch.float32 and t.stride(2) == 1 and t.stride(1) >= H else t.float().contiguous()
                for t in state)
        if h.stride(1) != c.stride(1):
            h, c = h.contiguous(), c.contiguous()
        if h.shape != (L, n, H) or c.shape != (L, n, H) or tokens.dtype != torch.int64 or not tokens.is_contiguous():
            raise ValueError(f"tokens {tuple(tokens.shape)} {tokens.dtype}, state {tuple(h.shape)}, {tuple(c.shape)}")
        buf = torch.empty(2, L, n, Hp, device=emb.device)
        wd, st = (BF16 if self._b.cd == torch.bfloat16 else F32), ops.stream()
        for k in range(L):
            x, tp = (emb, tokens.data_ptr()) if k == 0 else (buf[0, k - 1], None)
            lib.ea_lstm_step(wd, n, H, H, wpack[k].data_ptr(), bias[k].data_ptr(), x.data_ptr(), Hp, tp, 1, self.odim,
                             h[k].data_ptr(), c[k].data_ptr(), h.stride(1), n, None, buf[0, k].data_ptr(),
                             buf[1, k].data_ptr(), Hp, None, st)
        return buf[0, L - 1, :, :H], (buf[0, :, :, :H], buf[1, :, :, :H])

    def score(self, hyp, cache: Dict[str, Any]):
        """One-step forward of a hypothesis; cache: (dec_out, state) per label sequence.
        -> dec_out (D_dec), the new state ((N, 1, D_dec), (N, 1, D_dec)), label (1,)."""
        label = torch.full((1,), hyp.yseq[-1], dtype=torch.long, device=self.device)
        str_labels = "_".join(map(str, hyp.yseq))
        if str_labels in cache:
            dec_out, dec_state = cache[str_labels]
        else:
            with torch.no_grad():
                dec_out, dec_state = self.step(label, hyp.dec_state)
            cache[str_labels] = (dec_out, dec_state)
        return dec_out[0], dec_state, label

    def batch_score(self, hyps: List[Any], dec_states, cache: Dict[str, Any], use_lm: bool):
        """One-step forward of hypotheses, the uncached label sequences in one step of the kernel.
        -> dec_out (B, D_dec), states ((N, B, D_dec), (N, B, D_dec)), the LM's labels (B, 1) or None."""
        keys = ["_".join(map(str, h.yseq)) for h in hyps]
        todo = [i for i, key in enumerate(keys) if key not in cache]
        if todo:
            labels = torch.tensor([hyps[i].yseq[-1] for i in todo], dtype=torch.long).to(self.device)
            prev = self.create_batch_states(self.init_state(len(todo)), [hyps[i].dec_state for i in todo])
            with torch.no_grad():
                dec_out, new_states = self.step(labels, prev)
            for j, i in enumerate(todo):
                cache[keys[i]] = (dec_out[j:j + 1], self.select_state(new_states, j))
        done = [cache[key] for key in keys]
        dec_out = torch.cat([d[0] for d in done], dim=0)
        dec_states = self.create_batch_states(dec_states, [d[1] for d in done])
        lm_labels = torch.tensor([h.yseq[-1] for h in hyps], dtype=torch.long).to(self.device).view(-1, 1) if use_lm else None
        return dec_out, dec_states, lm_labels

    def select_state(self, states, idx: int):
        """-> the state of hypothesis idx ((N, 1, D_dec), (N, 1, D_dec))."""
        return states[0][:, idx:idx + 1, :], states[1][:, idx:idx + 1, :]

    def create_batch_states(self, states, new_states: List[Any], check_list: Optional[List] = None):
        """[N x ((N, 1, D_dec), (N, 1, D_dec))] -> ((N, B, D_dec), (N, B, D_dec))."""
        return torch.cat([s[0] for s in new_states], dim=1), torch.cat([s[1] for s in new_states], dim=1)
