"""SequentialRNNLM — drop-in for espnet2/lm/seq_rnn_lm.py as a decoding scorer (the
`scorers["lm"]` of espnet2/bin/asr_inference.py:149-183), the LM task's default (`lm: seq_rnn`).

Same constructor, state_dict layout (encoder.weight, rnn.{weight_ih,weight_hh,bias_ih,bias_hh}_l{k},
decoder.{weight,bias}) and scorer interface (zero_state, forward -> (logits, (h, c)), score,
batch_score).  The HIP path of one decoding step over n hypotheses: one fused LSTM launch per
layer (ea_lstm_step: both matrix products, the biases, the gates and the cell update; layer 0
reads its rows straight from the embedding table by token id, every layer gathers its parent's
state by index), the output Linear on the few-row GEMM and the row log-softmax: nlayers + 2
launches.

The kernels read packed copies made in prepare(): the LSTM weights in the slice-major tile
layout of include/espnet_amd.h (lstm_pack.py), the embedding table and decoder.weight
with their rows zero padded to a multiple of EA_LSTM_KG.  A step's states live in one
(2, nlayers, n, Hp) buffer; batch_score returns views of it and recognises them when they come
back, so the beam's reordering costs an index vector and no copy.

prepare(train=True) adds the training path (rnn_train.py's nodes, on the handles _bind_train
builds: an LSTMLayer per layer, the embedding table, the output head): in training mode with
autograd, forward runs the embedding, the dropouts, one autograd node per LSTM layer (one GEMM for the
input projection of all time steps, then ea_lstm_cell_fwd / ea_lstm_cell_bwd once per step) and
the output Linear over the whole padded batch.  The recurrent kernels' packs of weight_hh are
rebuilt on the device after every optimizer step (ParamArena.update_hooks) and the scorer's
packs lazily at the next eval call, so one object trains, validates and scores.  Under
torch.no_grad() a model in training mode takes the scorer's path (no dropout, nothing saved).  Without
train=True the model is a decoding scorer: a training-mode forward with autograd raises.
rnn_type other than lstm and tie_weights raise.
"""
from __future__ import annotations

from typing import Any, List, Optional, Tuple

import torch
from torch import nn

from .. import hip_ops as ops
from .._lib import BF16, F32, lib
from ..arena import ParamArena
from ..layers.common import Bound, site_seed
from .lstm_pack import HHPacks, pack_lstm_bias, pack_lstm_hh, pack_lstm_hh_t, pack_lstm_weights, rup
from .rnn_train import DropFn, EmbedFn, EmbedTable, LinearHead, LSTMLayer, LSTMLayerFn, OutLinearFn

# the pack functions stay importable from this module, where callers found them before lstm_pack.py
__all__ = ["SequentialRNNLM", "HHPacks", "pack_lstm_bias", "pack_lstm_hh", "pack_lstm_hh_t", "pack_lstm_weights"]


def _pad_cols(w: torch.Tensor, dtype) -> torch.Tensor:
    out = torch.zeros(w.shape[0], rup(w.shape[1]), dtype=dtype, device=w.device)
    out[:, :w.shape[1]] = w.detach()
    return out


class SequentialRNNLM(nn.Module):
    def __init__(self, vocab_size: int, unit: int = 650, nhid: int = None, nlayers: int = 2,
                 dropout_rate: float = 0.0, tie_weights: bool = False, rnn_type: str = "lstm",
                 ignore_id: int = 0):
        super().__init__()
        ninp = unit
        if nhid is None:
            nhid = unit
        rnn_type = rnn_type.upper()
        if rnn_type not in ("LSTM", "GRU", "RNN_TANH", "RNN_RELU"):
            raise ValueError(
                """An invalid option for `--model` was supplied,
                    options are ['LSTM', 'GRU', 'RNN_TANH' or 'RNN_RELU']""")
        if rnn_type != "LSTM":
            raise NotImplementedError(f"espnet_amd SequentialRNNLM: rnn_type={rnn_type.lower()!r} is not built "
                                      "(only rnn_type='lstm')")
        if tie_weights:
            raise NotImplementedError("espnet_amd SequentialRNNLM: tie_weights=True is not built")
        self.drop = nn.Dropout(dropout_rate)
        self.encoder = nn.Embedding(vocab_size, ninp, padding_idx=ignore_id)
        self.rnn = nn.LSTM(ninp, nhid, nlayers, dropout=dropout_rate, batch_first=True)
        self.decoder = nn.Linear(nhid, vocab_size)
        self.rnn_type = rnn_type
        self.vocab_size = vocab_size
        self.ninp = ninp
        self.nhid = nhid
        self.nlayers = nlayers
        self.arena = None

    def zero_state(self):
        """Initialize LM state filled with zero values (seq_rnn_lm.py:81-90)."""
        h = torch.zeros((self.nlayers, self.nhid), dtype=torch.float)
        c = torch.zeros((self.nlayers, self.nhid), dtype=torch.float)
        return h, c

    # ------------------------------------------------------------------ device copies
    def prepare(self, device="cuda", amp: bool = False, train: bool = False, seed: int = 0, *, owner=None):
        """Move the parameters into a flat arena on the GPU and build the packed operands
        (amp: bf16 LSTM and output-Linear weights, half the bytes streamed per step).
        train: also build the training path (bf16 weight shadow under amp, the recurrent
        kernels' packs, dropout streams drawn from `seed` and the step counter).
        owner: the module that holds this one as its attribute `lm` (ESPnetLanguageModel); the
        arena is then laid out over the owner's parameter names, which the optimizer uses."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("espnet_amd runs on the GPU only (no CPU fallback)")
        self._cd, self._device = (torch.bfloat16 if amp else torch.float32), device
        self._train, self._seed, self._nstep, self._stale = bool(train), int(seed), 0, False
        self._prefix = "" if owner is None else "lm."
        self.arena = ParamArena(self if owner is None else owner, device, shadow_dtype=self._cd if train else None)
        if train:
            self._bind_train(Bound(self.arena, self._prefix, self._cd))
        self._recent = {}  # storage pointer -> (state buffer, states handed out) of the last two steps
        self._handed = {}  # id(state tuple) -> (the tuple, its buffer, its row)
        self.repack()
        if not self.__dict__.get("_hooked", False):
            self.register_load_state_dict_post_hook(lambda m, _: m.repack() if m.arena is not None else None)
            self.__dict__["_hooked"] = True
        return self

    def _bind_train(self, b: Bound):
        """The training nodes' handles (rnn_train.py) over the arena views of b."""
        dev = b.arena.device
        self._anchor = torch.zeros(1, device=dev, requires_grad=True)
        self._embed = EmbedTable(self.encoder, dev)
        self._layers = [LSTMLayer(self.rnn, b.w(f"rnn.weight_ih_l{k}"), b.cd, k) for k in range(self.nlayers)]
        self._head = LinearHead(self.decoder, b.w("decoder.weight"), b.cd)
        b.arena.update_hooks.append(self._weights_changed)

    def _weights_changed(self):
        """After an optimizer step (or a shadow refresh): the recurrent packs now, on the
        stream, the scorer's packs at the next eval call."""
        for lay in self._layers:
            lay.refresh()
        self._stale = True

    @torch.no_grad()
    def repack(self):
        cd = self._cd
        self._stale = False
        if self._train:
            self.arena.refresh_shadow()  # (runs the update hooks: the recurrent packs)
            self._stale = False
        self._emb = _pad_cols(self.encoder.weight, torch.float32)
        self._wpack, self._bias = [], []
        for k in range(self.nlayers):
            w_ih, w_hh = getattr(self.rnn, f"weight_ih_l{k}"), getattr(self.rnn, f"weight_hh_l{k}")
            self._wpack.append(pack_lstm_weights(w_ih, w_hh, cd))
            self._bias.append(pack_lstm_bias(getattr(self.rnn, f"bias_ih_l{k}"), getattr(self.rnn, f"bias_hh_l{k}")))
        self._wdec = _pad_cols(self.decoder.weight, cd)
        self._bdec = self.decoder.bias.detach().float().contiguous()
        Hp = rup(self.nhid)
        self._zero = torch.zeros(2, self.nlayers, 1, Hp, device=self._device)
        self._src0 = {}
        self._recent.clear()
        self._handed.clear()

    def packed_bytes(self) -> int:
        """Bytes one decoding step streams: the packed LSTM weights and the padded decoder.weight."""
        return sum(w.numel() * w.element_size() for w in self._wpack) + self._wdec.numel() * self._wdec.element_size()

    # ------------------------------------------------------------------ one step
    def _step(self, tok: torch.Tensor, ldtok: int, n: int, prev: torch.Tensor, src: Optional[torch.Tensor]):
        """One token of n hypotheses through the layers.  tok: int64 device tensor whose element
        r * ldtok is row r's id; prev: (2, L, n_prev, Hp) states; src: int32 parent rows or None.
        -> (2, L, n, Hp) new states and the output Linear's operand (n, Hp)."""
        L, H, Hp = self.nlayers, self.nhid, prev.shape[3]
        n_prev = prev.shape[2]
        bf = self._cd == torch.bfloat16
        buf = torch.empty(2, L, n, Hp, device=self._device)
        hb = torch.empty(n, Hp, dtype=torch.bfloat16, device=self._device) if bf else None
        st = ops.stream()
        sp = ops.ptr(src)
        for k in range(L):
            last = k == L - 1
            if k == 0:
                x, ldx, I, tp = self._emb, self._emb.shape[1], self.ninp, tok.data_ptr()
            else:
                x, ldx, I, tp = buf[0, k - 1], Hp, H, None
            lib.ea_lstm_step(BF16 if bf else F32, n, I, H, self._wpack[k].data_ptr(), self._bias[k].data_ptr(),
                             x.data_ptr(), ldx, tp, ldtok, self.vocab_size, prev[0, k].data_ptr(),
                             prev[1, k].data_ptr(), Hp, n_prev, sp, buf[0, k].data_ptr(), buf[1, k].data_ptr(), Hp,
                             hb.data_ptr() if (bf and last) else None, st)
        return buf, (hb if bf else buf[0, L - 1])

    def _logits(self, xo: torch.Tensor) -> torch.Tensor:
        y = torch.empty(xo.shape[0], self.vocab_size, device=self._device)
        ops.linear(xo, self._wdec, y, epi=ops.make_epi(bias=self._bdec))
        return y

    def _check(self):
        if self.arena is None:
            raise RuntimeError("SequentialRNNLM.prepare(device) first")
        if torch.is_grad_enabled() and self.training:
            raise NotImplementedError("espnet_amd SequentialRNNLM is a decoding scorer (no training): "
                                      "prepare(device, train=True) builds the training path")
        if self._stale:
            self.repack()

    def _remember(self, buf: torch.Tensor, states: List[Any]):
        """Keep the last two steps' buffers and the state tuples handed out for them alive: a
        state that comes back as the very object is recognised by identity (a dict lookup per
        hypothesis), any other view of a kept buffer by its storage offsets (_parents)."""
        if len(self._recent) >= 2:
            _, old = self._recent.pop(next(iter(self._recent)))
            for s in old:
                del self._handed[id(s)]
        self._recent[buf.untyped_storage().data_ptr()] = (buf, states)
        for i, s in enumerate(states):
            self._handed[id(s)] = (s, buf, i)

    def _parents_by_identity(self, states: List[Any]):
        first = self._handed.get(id(states[0]))
        if first is None:
            return None
        base, idx = first[1], []
        for s in states:
            e = self._handed.get(id(s))
            if e is None or e[0] is not s or e[1] is not base:
                return None
            idx.append(e[2])
        return base, idx

    def _parents(self, states: List[Any]):
        """The common (2, L, n_prev, Hp) buffer the states are views of and their rows in it, or
        None when they are not all views of one recent step's buffer."""
        first = states[0]
        if first is None or not isinstance(first[0], torch.Tensor) or first[0].device.type != "cuda":
            return None
        base = self._recent.get(first[0].untyped_storage().data_ptr())
        if base is None:
            return None
        base = base[0]
        _, L, n_prev, Hp = base.shape
        sptr, coff = base.untyped_storage().data_ptr(), L * n_prev * Hp
        shape, stride = (L, self.nhid), (n_prev * Hp, 1)
        idx = []
        for s in states:
            if s is None:
                return None
            h, c = s
            for t in (h, c):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != shape \
                        or t.stride() != stride or t.device != base.device \
                        or t.untyped_storage().data_ptr() != sptr:
                    return None
            i, rem = divmod(h.storage_offset(), Hp)
            if rem or i >= n_prev or c.storage_offset() != coff + i * Hp:
                return None
            idx.append(i)
        return base, idx

    def _stack(self, states: List[Any]) -> torch.Tensor:
        """Fallback: states of mixed origin (None = zeros, (L, H) or (L, 1, H) tensors) copied into
        a fresh (2, L, n, Hp) buffer."""
        L, H = self.nlayers, self.nhid
        prev = torch.zeros(2, L, len(states), rup(H), device=self._device)
        for i, s in enumerate(states):
            if s is None:
                continue
            for j in (0, 1):
                prev[j, :, i, :H].copy_(s[j].reshape(L, H))
        return prev

    def batch_score(self, ys: torch.Tensor, states: List[Any], xs: torch.Tensor) -> Tuple[torch.Tensor, List[Any]]:
        """seq_rnn_lm.py:129-173: next-token log-probabilities (n, vocab) of every prefix and the
        list of (h[:, i], c[:, i]) views of this step's state buffer."""
        self._check()
        with torch.no_grad():
            return self._batch_score(ys, states)

    def _batch_score(self, ys, states):
        ys = ys.to(self._device, torch.int64)
        if ys.stride(-1) != 1:
            ys = ys.contiguous()
        n, T = ys.shape
        if len(states) != n:
            raise ValueError(f"{len(states)} states for {n} prefixes")
        src = None
        if all(s is None for s in states):
            prev = self._zero
            src = self._src0.get(n)
            if src is None:
                src = self._src0[n] = torch.zeros(n, dtype=torch.int32, device=self._device)
        else:
            found = self._parents_by_identity(states) or self._parents(states)
            if found is None:
                prev = self._stack(states)
            else:
                prev, idx = found
                if idx != list(range(n)):
                    src = torch.tensor(idx, dtype=torch.int32).to(self._device, non_blocking=True)
        tok = ys[:, T - 1:]
        buf, xo = self._step(tok, ys.stride(0), n, prev, src)
        lg = self._logits(xo)
        out = torch.empty_like(lg)
        lib.ea_softmax_rows(n, lg.shape[1], lg.data_ptr(), lg.shape[1], out.data_ptr(), 1, ops.stream())
        # (h[:, i], c[:, i]) of the (L, n, H) state, seq_rnn_lm.py:168: two unbinds, not 2n slices
        hc = buf[:, :, :, :self.nhid]
        new = list(zip(hc[0].unbind(1), hc[1].unbind(1)))
        self._remember(buf, new)
        return out, new

    def score(self, y: torch.Tensor, state: Any, x: torch.Tensor) -> Tuple[torch.Tensor, Any]:
        """seq_rnn_lm.py:106-127 for one prefix; state: None, (L, H) tensors (batch_score's and
        zero_state's) or the (L, 1, H) tensors the reference's score returns."""
        logp, st = self.batch_score(y.unsqueeze(0), [state], None)
        return logp[0], st[0]

    def forward(self, input: torch.Tensor, hidden: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """(B, T) ids, hidden None or (h, c) of (L, B, H) -> ((B, T, vocab) logits, (h, c)).
        Loops over T with the step kernel (T x nlayers launches and one output Linear): this is
        the scoring interface for whole sentences, not the decoding path, which is batch_score."""
        if self.arena is not None and self._train and self.training and torch.is_grad_enabled():
            return self._forward_train(input, hidden)
        self._check()
        with torch.no_grad():
            return self._forward(input, hidden)

    def dropout_seeds(self, nstep: int) -> dict:
        """The ea_scale_dropout streams of training forward number `nstep` (0 = the first after
        prepare): "embed" (self.drop on the embedding, (T*B, ninp) time-major), "rnn{k}"
        (nn.LSTM's dropout on layer k's output, k < nlayers - 1, (T*B, nhid)) and "out"
        (self.drop on the last layer's output)."""
        base = site_seed(self._seed, 0, nstep)
        seeds = {"embed": site_seed(base, 1, 0), "out": site_seed(base, 1, 1)}
        seeds.update({f"rnn{k}": site_seed(base, 2, k) for k in range(self.nlayers - 1)})
        return seeds

    def _forward_train(self, input, hidden):
        """The training forward over the whole padded batch (nn.LSTM without packing, as the
        reference runs it): time-major rows inside, (B, T, vocab) logits out.  hidden: constants."""
        V, L, H = self.vocab_size, self.nlayers, self.nhid
        ids = input.to(self._device, torch.int64)
        B, T = ids.shape
        if B == 0 or T == 0:
            raise ValueError(f"empty batch: {tuple(ids.shape)}")
        tok = ids.t().clamp(0, V - 1).contiguous().view(-1)  # row t * B + b
        seeds = self.dropout_seeds(self._nstep)
        self._nstep += 1
        p, p_rnn = float(self.drop.p), float(self.rnn.dropout)
        x = EmbedFn.apply(self._anchor, tok, self._embed)
        if p > 0.0:
            x = DropFn.apply(x, p, seeds["embed"])
        hn, cn = [], []
        for k in range(L):
            h0 = c0 = None
            if hidden is not None:
                h0 = hidden[0][k].detach().to(self._device, torch.float32)
                c0 = hidden[1][k].detach().to(self._device, torch.float32)
            x, h, c = LSTMLayerFn.apply(x, self._layers[k], T, B, h0, c0)
            hn.append(h)
            cn.append(c)
            if k < L - 1 and p_rnn > 0.0:
                x = DropFn.apply(x, p_rnn, seeds[f"rnn{k}"])
        if p > 0.0:
            x = DropFn.apply(x, p, seeds["out"])
        y = OutLinearFn.apply(x, self._head)
        return y.view(T, B, V).transpose(0, 1), (torch.stack(hn), torch.stack(cn))

    def _forward(self, input, hidden):
        ids = input.to(self._device, torch.int64).contiguous()
        B, T = ids.shape
        L, H, Hp = self.nlayers, self.nhid, rup(self.nhid)
        prev = torch.zeros(2, L, B, Hp, device=self._device)
        if hidden is not None:
            for j in (0, 1):
                prev[j, :, :, :H].copy_(hidden[j].reshape(L, B, H))
        hs = torch.empty(B, T, Hp, dtype=self._cd, device=self._device)
        for t in range(T):
            prev, xo = self._step(ids[:, t:], T, B, prev, None)
            hs[:, t].copy_(xo)
        lg = self._logits(hs.view(B * T, Hp)).view(B, T, self.vocab_size)
        return lg, (prev[0, :, :, :H].contiguous(), prev[1, :, :, :H].contiguous())
