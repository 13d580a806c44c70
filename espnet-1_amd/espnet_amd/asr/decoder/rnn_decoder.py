"""RNNDecoder — drop-in for espnet2/asr/decoder/rnn_decoder.py: the attention-RNN decoder of the
`decoder: rnn` recipes (LSTM cells over a location-aware attention, AttLoc of
espnet/nets/pytorch_backend/rnn/attentions.py:249-379).

Same constructor, defaults, state_dict keys and parameter creation order (a seeded build is
bit-identical; a reference checkpoint loads).  Built: rnn_type lstm, any num_layers / hidden_size,
dropout, att_conf with atype location and num_att 1.  gru, sampling_probability > 0,
context_residual, replace_sos, num_encs > 1 and every other atype raise NotImplementedError.

Training forward (time-major rows i * B + b, f32 between the nodes, bf16 matrix operands under amp):

    EmbedFn (+ DropFn)          eys of all L steps
    AttLocLSTM0Fn               attention + layer 0, the only recurrent pair (the query is layer 0's
                                hidden state): mlp_enc and the embedding half of layer 0's input
                                projection are ONE GEMM each over all rows; per step mlp_dec of the
                                query, ea_attloc_fwd, the context half of the projection and
                                the cell step; the backward walks the steps in reverse (the cell
                                step, ea_attloc_bwd) and takes every weight gradient from GEMMs /
                                column sums over all steps after the loop.  The state buffers, both
                                cell steps and layer 0's weight gradients are lm/rnn_train.py's
                                LSTMTape, as in LSTMLayerFn
    LSTMLayerFn x (layers - 1)  zero initial state (+ DropFn between)
    DropFn, OutLinearFn         logits; OutMaskFn zeroes the rows past ys_in_lens

The nodes take the handles bind() builds (lm/rnn_train.py): an LSTMLayer per cell, whose HHPacks of
weight_hh are rebuilt after every optimizer step (ParamArena.update_hooks), the EmbedTable of embed
and the LinearHead of output.  Lengths stay on the device; forward and backward make no host
synchronisation.

Decoding: init_state / score / batch_score with the reference's state dict (c_prev, z_prev, a_prev,
workspace).  batch_score runs the running hypotheses as the rows of ONE step (one ea_attloc_fwd,
one ea_lstm_cell_fwd per layer) over an encoder memory whose mlp_enc projection is computed once per
utterance (the reference's reset() / pre_compute_enc_h protocol).
"""
from __future__ import annotations

from typing import Any, List, Tuple

import torch

from ... import hip_ops as ops
from ..._lib import EPI_RESID, lib
from ...layers.common import Bound, site_seed
from ...lm.lstm_pack import rup
from ...lm.rnn_train import (DropFn, EmbedFn, EmbedTable, LinearHead, LSTMLayer, LSTMLayerFn, LSTMTape, OutLinearFn,
                               f32c)
from .transformer_decoder import AbsDecoder

_ATT_DEFAULTS = dict(atype="location", num_att=1, num_encs=1, aheads=4, adim=320, awin=5, aconv_chans=10,
                     aconv_filts=100, han_mode=False, han_type=None, han_heads=4, han_dim=320,
                     han_conv_chans=-1, han_conv_filts=100, han_win=5)


class AttLoc(torch.nn.Module):
    """The parameters of the reference's AttLoc, created in its order (attentions.py:264-278)."""

    def __init__(self, eprojs, dunits, att_dim, aconv_chans, aconv_filts):
        super().__init__()
        self.mlp_enc = torch.nn.Linear(eprojs, att_dim)
        self.mlp_dec = torch.nn.Linear(dunits, att_dim, bias=False)
        self.mlp_att = torch.nn.Linear(aconv_chans, att_dim, bias=False)
        self.loc_conv = torch.nn.Conv2d(1, aconv_chans, (1, 2 * aconv_filts + 1), padding=(0, aconv_filts),
                                        bias=False)
        self.gvec = torch.nn.Linear(att_dim, 1)
        self.dunits, self.eprojs, self.att_dim = dunits, eprojs, att_dim
        self.aconv_chans, self.aconv_filts = aconv_chans, aconv_filts


def build_attention_list(eprojs: int, dunits: int, atype: str = "location", num_att: int = 1, num_encs: int = 1,
                         aheads: int = 4, adim: int = 320, awin: int = 5, aconv_chans: int = 10,
                         aconv_filts: int = 100, han_mode: bool = False, han_type=None, han_heads: int = 4,
                         han_dim: int = 320, han_conv_chans: int = -1, han_conv_filts: int = 100, han_win: int = 5):
    """rnn_decoder.py:14-79 for what is built: one location attention.  aheads / awin and the han_*
    keys are accepted and unused, as the reference's initial_att leaves them for `location`."""
    if num_encs != 1:
        raise NotImplementedError(f"espnet_amd RNNDecoder: att_conf num_encs={num_encs} is not built (one encoder)")
    if atype != "location":
        raise NotImplementedError(f"espnet_amd RNNDecoder: att_conf atype={atype!r} is not built "
                                  "(only atype='location')")
    if num_att != 1:
        raise NotImplementedError(f"espnet_amd RNNDecoder: att_conf num_att={num_att} is not built (num_att=1)")
    return torch.nn.ModuleList([AttLoc(eprojs, dunits, adim, aconv_chans, aconv_filts)])


def _attloc_ws(B, T, A, C, dev, bwd=False):
    n = B * T * (1 + (3 + (A + 63) // 64) * C) if bwd else B * T * (1 + C)
    return torch.empty(max(n, 1), device=dev)


def _attloc_fwd(dec, md, hs, shs, pre, spre, hlens, q, aprev, w, c, B, T):
    """One ea_attloc_fwd: hs (.., E) / pre (.., A) rows of the memory (utterance strides shs / spre,
    0 = shared), q (B, A) f32 the projected query, aprev (B, T) or None -> w (B, T), c (B, E) views."""
    att = dec.att_list[0]
    b = dec._b
    E, A, C, F = att.eprojs, att.att_dim, att.aconv_chans, att.aconv_filts
    ws = _attloc_ws(B, T, A, C, w.device)
    lib.ea_attloc_fwd(md, B, T, E, A, C, F, hs.data_ptr(), hs.stride(-2), shs, pre.data_ptr(), pre.stride(-2), spre,
                      hlens.data_ptr(), q.data_ptr(), q.stride(0), ops.ptr(aprev), 0 if aprev is None else aprev.stride(0),
                      b.f("att_list.0.loc_conv.weight").data_ptr(), b.f("att_list.0.mlp_att.weight").data_ptr(),
                      b.f("att_list.0.gvec.weight").data_ptr(), b.f("att_list.0.gvec.bias").data_ptr(),
                      w.data_ptr(), w.stride(0), c.data_ptr(), c.stride(0), ws.data_ptr(), ws.numel(), ops.stream())


class AttLocLSTM0Fn(torch.autograd.Function):
    """Attention + LSTM layer 0 over the L steps: (eys (L*B, H) f32, hs_pad (B, T, E) f32) -> z0 of
    every step (L*B, H).  query_seeds: the dropout stream of each step's query (dropout_dec[0])."""

    @staticmethod
    def forward(ctx, eys, hs_pad, dec, hlens, L, B, p, query_seeds):
        b, att, lay = dec._b, dec.att_list[0], dec._layers[0]
        cd, bf, wd, w_ih = lay.cd, lay.bf, lay.wd, lay.w_ih
        H, dev = lay.H, eys.device
        T, E, A = hs_pad.shape[1], att.eprojs, att.att_dim
        w_dec = b.w("att_list.0.mlp_dec.weight")
        bsum = lay.bias_sum()
        hs_c = ops.cast(hs_pad.reshape(B * T, E), cd)
        pre = torch.empty(B * T, A, dtype=cd, device=dev)
        ops.linear(hs_c, b.w("att_list.0.mlp_enc.weight"), pre, epi=ops.make_epi(bias=b.f("att_list.0.mlp_enc.bias")))
        # layer 0's input rows [eys | c]: the embedding half now, the context half step by step
        x0 = torch.empty(L * B, lay.I, dtype=cd, device=dev)
        ops.scale_dropout(eys, x0[:, :H])
        xproj = lay.input_proj(x0[:, :H], w_ih[:, :H], bsum)
        tape = LSTMTape(lay, L, B, dev)
        zs, zin = tape.hs, tape.hin
        # the queries dropout(z0_{i-1}) in the compute dtype: the states themselves when p = 0
        qs = torch.empty(L, B, H, dtype=cd, device=dev) if p > 0.0 else zin[:L, :, :H]
        if p > 0.0:
            qs[0].zero_()
        q = torch.empty(L, B, A, device=dev)
        q[0].zero_()  # the first query is the zero state
        w = torch.empty(L, B, T, device=dev)
        cf = None if not bf else torch.empty(B, E, device=dev)
        cell = tape.fwd_steps(xproj)
        for i in range(L):
            rows = slice(i * B, (i + 1) * B)
            if i > 0:
                if p > 0.0:
                    ops.scale_dropout(zs[i, :, :H], qs[i], p=p, seed=query_seeds[i])
                ops.linear(qs[i], w_dec, q[i])
            ci = cf if bf else x0[rows, H:]
            _attloc_fwd(dec, wd, hs_c, T * E, pre, T * A, hlens, q[i], w[i - 1] if i else None, w[i], ci, B, T)
            if bf:
                ops.scale_dropout(cf, x0[rows, H:])
            ops.linear(x0[rows, H:], w_ih[:, H:], xproj[rows], epi=ops.make_epi(beta=1.0))
            cell(i)
        ctx.save = (dec, hlens, T, p, query_seeds, hs_c, pre, x0, tape, qs, q, w)
        dec._last_att_w = w.detach()
        return tape.outputs()

    @staticmethod
    def backward(ctx, dy):
        dec, hlens, T, p, query_seeds, hs_c, pre, x0, tape, qs, q, w = ctx.save
        ctx.save = None
        b, att, lay = dec._b, dec.att_list[0], tape.layer
        cd, wd, w_ih, L, B = lay.cd, lay.wd, lay.w_ih, tape.T, tape.B
        H, G, dev = lay.H, lay.G, dy.device
        E, A, C, F = att.eprojs, att.att_dim, att.aconv_chans, att.aconv_filts
        st = ops.stream()
        w_dec = b.w("att_list.0.mlp_dec.weight")
        dz = f32c(dy).contiguous().clone()  # (L*B, H): step i's rows also collect the next query's gradient
        cell = tape.bwd_steps(dz, H)
        dgn = tape.dgn
        dctx = torch.empty(B, E, device=dev)
        dwc = torch.empty(2, B, T, device=dev)  # the attention-weight gradient carried to the step before
        dq = torch.empty(L, B, A, device=dev)
        dpre = torch.zeros(B * T, A, device=dev)
        dhs = torch.zeros(B, T, E, device=dev)
        nK = C * (2 * F + 1)
        part = torch.zeros(B, A * C + nK + A + 1, device=dev)
        ws = _attloc_ws(B, T, A, C, dev, bwd=True)
        kw, mw, gw = (b.f(f"att_list.0.{n}.weight").data_ptr() for n in ("loc_conv", "mlp_att", "gvec"))
        for i in range(L - 1, -1, -1):
            last = i == L - 1
            cell(i)
            ops.linear_dx(dgn[i][:, :G], w_ih[:, H:], dctx)
            lib.ea_attloc_bwd(wd, B, T, E, A, C, F, hs_c.data_ptr(), E, T * E, pre.data_ptr(), A, T * A,
                              hlens.data_ptr(), q[i].data_ptr(), A, w[i - 1].data_ptr() if i else None, T,
                              w[i].data_ptr(), T, kw, mw, gw, dctx.data_ptr(), E,
                              None if last else dwc[(i + 1) & 1].data_ptr(), T, dpre.data_ptr(), A, T * A,
                              dhs.data_ptr(), E, T * E, dq[i].data_ptr(), A, dwc[i & 1].data_ptr() if i else None, T,
                              part.data_ptr(), part.stride(0), ws.data_ptr(), ws.numel(), st)
            if i > 0:  # dz0_{i-1} += dropout-mask(dq_i . W_dec)
                ops.linear_dx(ops.cast(dq[i], cd), w_dec, dz[(i - 1) * B:i * B],
                              epi=ops.make_epi(EPI_RESID, resid=dz[(i - 1) * B:i * B], drop_p=p, seed=query_seeds[i]))
        dgm = tape.dgm
        deys = None
        if ctx.needs_input_grad[0]:
            deys = torch.empty(L * B, H, device=dev)
            ops.linear_dx(dgm, w_ih[:, :H], deys)
        zprev = tape.weight_grads(x0)
        ops.linear_dw(ops.cast(dq.view(L * B, A), cd), qs.reshape(L * B, H) if p > 0.0 else zprev,
                      att.mlp_dec.weight.grad, accumulate=True)
        dpre_c = ops.cast(dpre, cd)
        ops.linear_dw(dpre_c, hs_c, att.mlp_enc.weight.grad, accumulate=True)
        ops.colsum(dpre, att.mlp_enc.bias.grad, accumulate=True)
        dhs2 = dhs.view(B * T, E)
        ops.linear_dx(dpre_c, b.w("att_list.0.mlp_enc.weight"), dhs2, epi=ops.make_epi(beta=1.0))
        # the utterances' partial sums, in row order
        o = 0
        for grad, n in ((att.mlp_att.weight.grad, A * C), (att.loc_conv.weight.grad, nK), (att.gvec.weight.grad, A),
                        (att.gvec.bias.grad, 1)):
            ops.colsum(part[:, o:o + n], grad.view(-1), accumulate=True)
            o += n
        return deys, (dhs if ctx.needs_input_grad[1] else None), None, None, None, None, None, None


class OutMaskFn(torch.autograd.Function):
    """z_all.masked_fill_(make_pad_mask(ys_in_lens, z_all, 1), 0) (rnn_decoder.py:245-248): rows of
    (B, L, V) past the target length are exactly 0 and receive no gradient."""

    @staticmethod
    def forward(ctx, y, lens):
        L = y.shape[1]
        keep = (torch.arange(L, device=y.device)[None, :] < lens[:, None]).unsqueeze(-1)
        ctx.keep = keep
        return y.masked_fill(~keep, 0.0)

    @staticmethod
    def backward(ctx, dy):
        return dy.masked_fill(~ctx.keep, 0.0), None


class RNNDecoder(AbsDecoder):
    def __init__(
        self,
        vocab_size: int,
        encoder_output_size: int,
        rnn_type: str = "lstm",
        num_layers: int = 1,
        hidden_size: int = 320,
        sampling_probability: float = 0.0,
        dropout: float = 0.0,
        context_residual: bool = False,
        replace_sos: bool = False,
        num_encs: int = 1,
        att_conf: dict = None,
    ):
        if rnn_type not in {"lstm", "gru"}:
            raise ValueError(f"Not supported: rnn_type={rnn_type}")
        if rnn_type != "lstm":
            raise NotImplementedError(f"espnet_amd RNNDecoder: rnn_type={rnn_type!r} is not built "
                                      "(only rnn_type='lstm')")
        if sampling_probability > 0:
            raise NotImplementedError(f"espnet_amd RNNDecoder: sampling_probability={sampling_probability} is not "
                                      "built (scheduled sampling)")
        if context_residual:
            raise NotImplementedError("espnet_amd RNNDecoder: context_residual=True is not built")
        if replace_sos:
            raise NotImplementedError("espnet_amd RNNDecoder: replace_sos=True is not built")
        if num_encs != 1:
            raise NotImplementedError(f"espnet_amd RNNDecoder: num_encs={num_encs} is not built (one encoder)")
        if num_layers < 1 or dropout < 0:
            raise ValueError(f"num_layers={num_layers}, dropout={dropout}")
        super().__init__()
        att_conf = dict(_ATT_DEFAULTS) if att_conf is None else dict(att_conf)
        eprojs = encoder_output_size
        self.dtype = rnn_type
        self.dunits = hidden_size
        self.dlayers = num_layers
        self.context_residual = context_residual
        self.sos = vocab_size - 1
        self.eos = vocab_size - 1
        self.odim = vocab_size
        self.sampling_probability = sampling_probability
        self.dropout = dropout
        self.num_encs = num_encs
        self.replace_sos = replace_sos
        # creation order of rnn_decoder.py:118-146
        self.embed = torch.nn.Embedding(vocab_size, hidden_size)
        self.dropout_emb = torch.nn.Dropout(p=dropout)
        self.decoder = torch.nn.ModuleList()
        self.dropout_dec = torch.nn.ModuleList()
        self.decoder += [torch.nn.LSTMCell(hidden_size + eprojs, hidden_size)]
        self.dropout_dec += [torch.nn.Dropout(p=dropout)]
        for _ in range(1, self.dlayers):
            self.decoder += [torch.nn.LSTMCell(hidden_size, hidden_size)]
            self.dropout_dec += [torch.nn.Dropout(p=dropout)]
        self.output = torch.nn.Linear(hidden_size, vocab_size)
        self.att_list = build_attention_list(eprojs=eprojs, dunits=hidden_size, **att_conf)
        self._b = None

    # ------------------------------------------------------------------ binding
    def arena_groups(self, prefix=""):
        return []  # no fused weights: every GEMM reads one parameter (or a column slice of one)

    def bind(self, arena, prefix, cd):
        self._b = b = Bound(arena, prefix, cd)
        self._embed = EmbedTable(self.embed, arena.device)
        self._layers = [LSTMLayer(cell, b.w(f"decoder.{k}.weight_ih"), cd) for k, cell in enumerate(self.decoder)]
        self._head = LinearHead(self.output, b.w("output.weight"), cd)
        self._mem = None
        self._last_att_w = None
        self._anchor = torch.zeros(1, device=arena.device, requires_grad=True)
        arena.update_hooks.append(self._weights_changed)
        self._weights_changed()

    def _weights_changed(self):
        for lay in self._layers:
            lay.refresh()
        self._mem = None  # a cached mlp_enc projection belongs to the old weights

    # ------------------------------------------------------------------ training
    def dropout_seeds(self, seed: int, L: int) -> dict:
        """The ea_scale_dropout streams of one forward: "emb" (dropout_emb, (L*B, H) time-major),
        "query" (dropout_dec[0] on the attention query, one stream per step i >= 1 over (B, H)),
        "layer{l}" (dropout_dec[l-1] on layer l's input, (L*B, H)) and "out" (dropout_dec[-1])."""
        s = {"emb": site_seed(seed, 700, 0), "out": site_seed(seed, 700, 1),
             "query": [site_seed(seed, 701, i) for i in range(L)]}
        s.update({f"layer{l}": site_seed(seed, 702, l) for l in range(1, self.dlayers)})
        return s

    def forward(self, hs_pad: torch.Tensor, hlens: torch.Tensor, ys_in_pad: torch.Tensor,
                ys_in_lens: torch.Tensor, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._b is None:
            raise RuntimeError("RNNDecoder: bind(arena, prefix, cd) first (ESPnetASRModel.prepare)")
        V, dev = self.odim, hs_pad.device
        B, L = ys_in_pad.shape
        if B == 0 or L == 0 or hs_pad.shape[1] == 0:
            raise ValueError(f"empty batch: {tuple(ys_in_pad.shape)}, {tuple(hs_pad.shape)}")
        hlens = hlens.to(dev, torch.long)
        ys_in_lens = ys_in_lens.to(dev, torch.long)
        tok = ys_in_pad.to(dev, torch.long).t().clamp(0, V - 1).contiguous().view(-1)  # row i * B + b
        p = float(self.dropout) if self.training else 0.0
        seeds = self.dropout_seeds(seed, L)
        x = EmbedFn.apply(self._anchor, tok, self._embed)
        if p > 0.0:
            x = DropFn.apply(x, p, seeds["emb"])
        x = AttLocLSTM0Fn.apply(x, hs_pad.contiguous().float(), self, hlens, L, B, p, seeds["query"])
        for l in range(1, self.dlayers):
            if p > 0.0:
                x = DropFn.apply(x, p, seeds[f"layer{l}"])
            x, _, _ = LSTMLayerFn.apply(x, self._layers[l], L, B, None, None)
        if p > 0.0:
            x = DropFn.apply(x, p, seeds["out"])
        y = OutLinearFn.apply(x, self._head)
        return OutMaskFn.apply(y.view(L, B, V).transpose(0, 1), ys_in_lens), ys_in_lens

    # ------------------------------------------------------------------ decoding
    def zero_state(self, hs_pad):
        return hs_pad.new_zeros(hs_pad.size(0), self.dunits)

    def _zero_states(self, dev):
        z = [torch.zeros(1, self.dunits, device=dev) for _ in range(self.dlayers)]
        c = [torch.zeros(1, self.dunits, device=dev) for _ in range(self.dlayers)]
        return dict(c_prev=c[:], z_prev=z[:], a_prev=None, workspace=(0, z, c))

    def init_state(self, x):
        """rnn_decoder.py:251-278: zero states, no previous attention; the encoder memory of this
        utterance is projected once (the reference's reset())."""
        self._mem = None
        if self._b is not None and x.is_cuda:
            self._memory(x)
        return self._zero_states(x.device)

    @torch.no_grad()
    def _memory(self, x):
        """(hs, pre_enc) in the compute dtype of the memory x (T, E); cached for the very tensor
        init_state / the last call saw, recomputed for any other."""
        m = self._mem
        if m is not None and m[0].data_ptr() == x.data_ptr() and m[0].shape == x.shape \
                and m[0].stride() == x.stride() and m[1] == x._version:
            return m[2], m[3]
        b, att = self._b, self.att_list[0]
        hs = ops.cast(x.contiguous().float(), b.cd)
        pre = torch.empty(x.shape[0], att.att_dim, dtype=b.cd, device=x.device)
        ops.linear(hs, b.w("att_list.0.mlp_enc.weight"), pre, epi=ops.make_epi(bias=b.f("att_list.0.mlp_enc.bias")))
        self._mem = (x, x._version, hs, pre)
        return hs, pre

    @torch.no_grad()
    def batch_score(self, ys: torch.Tensor, states: List[Any], xs: torch.Tensor) -> Tuple[torch.Tensor, List[Any]]:
        """Next-token log-probabilities (n, V) of n prefixes ys (n, L) over xs (n, T, E), every row
        the same memory, and their new state dicts (views of this step's buffers)."""
        if self._b is None:
            raise RuntimeError("RNNDecoder: bind(arena, prefix, cd) first (ESPnetASRModel.prepare)")
        b, att = self._b, self.att_list[0]
        cd, bf, wd = b.cd, self._layers[0].bf, self._layers[0].wd
        n = ys.shape[0]
        if len(states) != n or xs.shape[0] != n:
            raise ValueError(f"{len(states)} states, {xs.shape[0]} memories for {n} prefixes")
        if n > 1 and xs.stride(0) != 0 and not all(torch.equal(xs[0], xs[i]) for i in range(1, n)):
            raise NotImplementedError("RNNDecoder.batch_score: the hypotheses share one encoder memory")
        x = xs[0]
        dev = x.device
        T, E = x.shape
        H, A, NL, V = self.dunits, att.att_dim, self.dlayers, self.odim
        Hp, G, st = rup(H), 4 * H, ops.stream()
        hs, pre = self._memory(x)
        states = [self._zero_states(dev) if s is None else s for s in states]  # (None: a greedy loop's start)
        zp = torch.zeros(NL, n, Hp, device=dev)
        cp = torch.zeros(NL, n, Hp, device=dev)
        for l in range(NL):
            zp[l, :, :H].copy_(torch.cat([s["z_prev"][l].reshape(1, H) for s in states]))
            cp[l, :, :H].copy_(torch.cat([s["c_prev"][l].reshape(1, H) for s in states]))
        zpc = ops.cast(zp.view(NL * n, Hp), cd).view(NL, n, Hp)
        aprev = None
        if any(s["a_prev"] is not None for s in states):
            aprev = torch.cat([torch.full((1, T), 1.0 / T, device=dev) if s["a_prev"] is None
                               else s["a_prev"].reshape(1, T).to(dev, torch.float32) for s in states])
        tok = ys[:, -1].to(dev, torch.long).clamp(0, V - 1).contiguous()
        ey = torch.empty(n, H, device=dev)
        lib.ea_embed_fwd(n, H, 1, tok.data_ptr(), b.f("embed.weight").data_ptr(), 1.0, self._embed.pe0.data_ptr(), 0.0, 0,
                         ey.data_ptr(), st)
        x0 = torch.empty(n, H + E, dtype=cd, device=dev)
        ops.scale_dropout(ey, x0[:, :H])
        q = torch.empty(n, A, device=dev)
        ops.linear(zpc[0, :, :H], b.w("att_list.0.mlp_dec.weight"), q)
        w = torch.empty(n, T, device=dev)
        c = torch.empty(n, E, device=dev) if bf else x0[:, H:]
        hlens = torch.full((n,), T, dtype=torch.long, device=dev)
        _attloc_fwd(self, wd, hs, 0, pre, 0, hlens, q, aprev, w, c, n, T)
        if bf:
            ops.scale_dropout(c, x0[:, H:])
        zn = torch.empty(NL, n, Hp, device=dev)
        cn = torch.empty(NL, n, Hp, device=dev)
        zb = torch.empty(NL, n, Hp, dtype=torch.bfloat16, device=dev) if bf else None
        gates = torch.empty(n, G, device=dev)
        xin = x0
        # the layers are this step's rows: each has its own pack and reads the cast copy zpc of the
        # previous states, so LSTMTape's step (one pack, hs[t] -> hs[t + 1]) does not fit these buffers
        for l, lay in enumerate(self._layers):
            xproj = torch.empty(n, G, device=dev)
            ops.linear(xin, lay.w_ih, xproj, epi=ops.make_epi(bias=lay.bias_sum()))
            lib.ea_lstm_cell_fwd(wd, n, H, lay.hh.fwd.data_ptr(), xproj.data_ptr(), G, zpc[l].data_ptr(),
                                 cp[l].data_ptr(), Hp, zn[l].data_ptr(), cn[l].data_ptr(), Hp,
                                 zb[l].data_ptr() if bf else None, gates.data_ptr(), G, st)
            xin = (zb if bf else zn)[l, :, :H]
        logits = torch.empty(n, V, device=dev)
        ops.linear(xin, b.w("output.weight"), logits, epi=ops.make_epi(bias=b.f("output.bias")))
        logp = torch.empty(n, V, device=dev)
        lib.ea_softmax_rows(n, V, logits.data_ptr(), V, logp.data_ptr(), 1, st)
        new = []
        for i in range(n):
            z = [zn[l, i:i + 1, :H] for l in range(NL)]
            cc = [cn[l, i:i + 1, :H] for l in range(NL)]
            new.append(dict(c_prev=cc[:], z_prev=z[:], a_prev=w[i:i + 1], workspace=(0, z, cc)))
        return logp, new

    def score(self, yseq, state, x):
        """rnn_decoder.py:280-332 for one prefix: batch_score's step with one row."""
        logp, st = self.batch_score(yseq.unsqueeze(0), [state], x.unsqueeze(0))
        return logp[0], st[0]
