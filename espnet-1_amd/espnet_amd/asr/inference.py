"""Inference consumers of the trained model, on the same HIP kernels:

* ``ctc_greedy`` — espnet2/asr/ctc.py:119-127 argmax + the greedy CTC collapse (repeats
  merged, blanks dropped) over each utterance's encoder frames.
* ``attention_greedy`` — espnet/nets/beam_search.py:346-432 with beam_size 1, the decoder as
  the only scorer (ctc_weight 0, no LM, no length bonus): a hypothesis grows by the best
  next token (decoder.batch_score, transformer_decoder.py:194-229) until <eos>, with <eos>
  forced at maxlen (post_process, :462-467); maxlen = encoder frames for maxlenratio 0.
  Each utterance is encoded alone, as Speech2Text does (a padded batch would let the
  conformer's depthwise convolution see padding frames).

* ``transducer_decode`` — espnet2/asr/transducer/beam_search_transducer.py for a `decoder: transducer`
  model: the greedy search and the default beam search over the joint-step kernels
  (csrc/transducer_step.hip); greedy over several utterances runs batched.

All run the model in eval mode (dropout off, BatchNorm running statistics).
"""
from __future__ import annotations

from typing import List, Tuple

import torch


def _encode(model, speech, speech_lengths):
    """model.encode for the decoders: an encoder with intermediate-CTC taps returns
    ((encoder_out, intermediate_outs), lens) (espnet_model.py:409-410); decoding uses
    encoder_out, as asr_inference.py does."""
    enc, olens = model.encode(speech, speech_lengths)
    if isinstance(enc, tuple):
        enc = enc[0]
    return enc, olens


def _attention_decoder_only(model):
    if getattr(model, "use_transducer_decoder", False):
        raise NotImplementedError("decoder: transducer: transducer decoding (greedy / beam search over the joint "
                                  "network) is not built; ctc_greedy serves a model trained with ctc_weight > 0")


def _collapse(ids, blank=0):
    out, prev = [], None
    for t in ids:
        if t != prev and t != blank:
            out.append(int(t))
        prev = t
    return out


@torch.no_grad()
def ctc_greedy(model, speech: torch.Tensor, speech_lengths: torch.Tensor) -> List[List[int]]:
    was = model.training
    model.eval()
    try:
        res = []
        for b in range(speech.shape[0]):
            le = int(speech_lengths[b])
            enc, olens = _encode(model, speech[b:b + 1, :le], speech_lengths[b:b + 1])
            ids = model.ctc.argmax(enc)[0, :int(olens[0])].tolist()
            res.append(_collapse(ids, model.blank_id))
        return res
    finally:
        model.train(was)


@torch.no_grad()
def attention_greedy(model, speech: torch.Tensor, speech_lengths: torch.Tensor, maxlenratio: float = 0.0,
                     minlenratio: float = 0.0) -> List[Tuple[List[int], float]]:
    _attention_decoder_only(model)
    if minlenratio != 0.0:
        raise NotImplementedError("minlenratio > 0 (beam_search.py retry loop) is not implemented")
    was = model.training
    model.eval()
    try:
        res = []
        sos, eos = model.sos, model.eos
        for b in range(speech.shape[0]):
            le = int(speech_lengths[b])
            enc, olens = _encode(model, speech[b:b + 1, :le], speech_lengths[b:b + 1])
            T = enc.shape[1]
            if maxlenratio == 0:
                maxlen = T
            elif maxlenratio < 0:
                maxlen = -1 * int(maxlenratio)
            else:
                maxlen = max(1, int(maxlenratio * T))
            yseq = [sos]
            score = 0.0
            st = [None]  # the decoder's key/value cache row, carried from step to step
            for i in range(maxlen):
                ys = torch.tensor([yseq], dtype=torch.long, device=enc.device)
                logp, st = model.decoder.batch_score(ys, st, enc)
                tok = int(torch.argmax(logp[0]))
                score += float(logp[0, tok])
                yseq.append(tok)
                if i == maxlen - 1 and tok != eos:
                    yseq.append(eos)
                if yseq[-1] == eos:
                    break
            res.append((yseq[1:-1], score))
        return res
    finally:
        model.train(was)


def _batched_greedy(model, encs: List[torch.Tensor]) -> List[Tuple[List[int], float]]:
    """BeamSearchTransducer.greedy_search over up to EA_RNNT_STEP_MAX_ROWS utterances at once: iteration t
    is one joint step with row i at frame min(t, T_i - 1) of its utterance, one decoder step of every row
    on the token it would emit and one project_dec; a row that emits takes the new state and D row, the
    others keep theirs (torch.where by mask).  Nothing synchronises with the host until the one copy of the
    (B, Tmax) tokens and scores at the end."""
    dec, jn = model.decoder, model.joint_network
    B, dev = len(encs), encs[0].device
    lens = [int(e.shape[0]) for e in encs]
    Tmax = max(lens)
    E = torch.zeros(B, Tmax, jn.joint_space_size, device=dev)
    for i, e in enumerate(encs):
        E[i, :lens[i]] = jn.project_enc(e.float())
    E = E.view(B * Tmax, -1)
    tl = torch.tensor(lens, dtype=torch.int32).to(dev)
    t_idx = torch.arange(Tmax, dtype=torch.int32, device=dev)[:, None]
    frames = (torch.arange(B, dtype=torch.int32, device=dev) * Tmax)[None, :] + torch.minimum(t_idx, tl[None, :] - 1)
    live = t_idx < tl[None, :]  # (Tmax, B): a row with t >= T_i is dead
    dec.set_device(dev)
    dec_out, state = dec.step(torch.full((B,), dec.blank_id, dtype=torch.long, device=dev), dec.init_state(B))
    D = jn.project_dec(dec_out)
    out = torch.zeros(2, Tmax, B, dtype=torch.int32, device=dev)  # token (0: none), the score's bits
    for t in range(Tmax):
        r = jn.step(E, frames[t], D, 1)
        tok, val = r.top_id[:, 0], r.top_value[:, 0]
        emit = (val > r.lp_blank) & live[t]  # blank, at index 0, wins ties (torch.max: the first maximum)
        new_out, new_state = dec.step(tok.long(), state)
        new_D = jn.project_dec(new_out)
        state = tuple(torch.where(emit[None, :, None], a, b) for a, b in zip(new_state, state))
        D = torch.where(emit[:, None], new_D, D)
        out[0, t] = torch.where(emit, tok, 0)
        out[1, t] = torch.where(emit, val, 0.0).view(torch.int32)
    out = out.cpu()
    toks, vals = out[0].t().tolist(), out[1].view(torch.float32).t().tolist()
    return [([y for y in toks[i] if y], float(sum(v for y, v in zip(toks[i], vals[i]) if y))) for i in range(B)]


@torch.no_grad()
def transducer_decode(model, speech: torch.Tensor, speech_lengths: torch.Tensor, beam_size: int = 1, nbest: int = 1,
                      score_norm: bool = True) -> List[List[Tuple[List[int], float]]]:
    """Decoding of a `decoder: transducer` model (espnet2/bin/asr_inference.py with a transducer decoder:
    BeamSearchTransducer, search_type "default"): per utterance the n-best list of (yseq without the leading
    blank, score).  Each utterance is encoded alone.  beam_size <= 1 is the greedy search; more than one
    utterance then runs batched, EA_RNNT_STEP_MAX_ROWS at a time (_batched_greedy)."""
    from .._lib import RNNT_STEP_MAX_ROWS
    from .transducer.beam_search_transducer import BeamSearchTransducer
    if not getattr(model, "use_transducer_decoder", False):
        raise ValueError("transducer_decode: the model has no transducer decoder (attention_greedy / "
                         "attention_beam_search / ctc_greedy serve the others)")
    search = BeamSearchTransducer(model.decoder, model.joint_network, beam_size, score_norm=score_norm, nbest=nbest)
    was = model.training
    model.eval()
    try:
        encs = []
        for b in range(speech.shape[0]):
            le = int(speech_lengths[b])
            enc, olens = _encode(model, speech[b:b + 1, :le], speech_lengths[b:b + 1])
            encs.append(enc[0, :int(olens[0])])
        if beam_size <= 1 and len(encs) > 1:
            res = []
            for i in range(0, len(encs), RNNT_STEP_MAX_ROWS):
                res += [[r] for r in _batched_greedy(model, encs[i:i + RNNT_STEP_MAX_ROWS])]
            return res
        return [[(h.yseq[1:], float(h.score)) for h in search(enc)] for enc in encs]
    finally:
        model.train(was)


@torch.no_grad()
def attention_beam_search(model, speech: torch.Tensor, speech_lengths: torch.Tensor, beam_size: int,
                          length_bonus: float = 0.0, maxlenratio: float = 0.0, minlenratio: float = 0.0,
                          ctc_weight: float = 0.0, batch: bool = False, lm=None, lm_weight: float = 1.0):
    """Speech2Text-style decoding (espnet2/bin/asr_inference.py:140-175) with BeamSearch
    (espnet/nets/beam_search.py) over the decoder (weight 1 - ctc_weight), the CTC prefix
    scorer (ctc_weight, pre-beam "full") and LengthBonus (length_bonus): per utterance the
    n-best list of Hypothesis records (yseq with <sos>/<eos>, score, per-scorer scores)."""
    from .beam_search import BatchBeamSearch, BeamSearch, CTCPrefixScorer, LengthBonus
    _attention_decoder_only(model)
    if batch:  # espnet/nets/batch_beam_search.py under its own name (the same batched search)
        BeamSearch = BatchBeamSearch  # noqa: N806
    was = model.training
    model.eval()
    try:
        V = model.vocab_size
        scorers = {"decoder": model.decoder, "ctc": CTCPrefixScorer(model.ctc, model.eos),
                   "length_bonus": LengthBonus(V)}
        weights = {"decoder": 1.0 - ctc_weight, "ctc": ctc_weight, "length_bonus": length_bonus}
        if lm is not None:  # shallow fusion (asr_inference.py:149-183: scorers["lm"], lm_weight)
            scorers["lm"], weights["lm"] = lm, lm_weight
        bs = BeamSearch(scorers=scorers, weights=weights,
                        beam_size=beam_size, vocab_size=V, sos=model.sos, eos=model.eos, pre_beam_score_key="full")
        res = []
        for b in range(speech.shape[0]):
            le = int(speech_lengths[b])
            enc, _ = _encode(model, speech[b:b + 1, :le], speech_lengths[b:b + 1])
            res.append(bs(enc[0], maxlenratio=maxlenratio, minlenratio=minlenratio))
        return res
    finally:
        model.train(was)
