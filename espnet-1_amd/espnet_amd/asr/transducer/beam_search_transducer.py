"""BeamSearchTransducer — drop-in for espnet2/asr/transducer/beam_search_transducer.py: the greedy search
(beam_size <= 1, :221-253) and the default beam search (:255-354) over TransducerDecoder and JointNetwork.

Same constructor.  Built: search_type "default" without an LM, beam_size up to EA_RNNT_STEP_MAX_K (16: the
joint-step kernel's selection width).  tsd / alsd / nsc / maes, an LM and wider beams raise NotImplementedError.

Per utterance E = lin_enc(enc_out) is one GEMM.  Each expansion of a hypothesis is one decoder step when
its label sequence misses the cache (ea_lstm_step per layer), one project_dec (the few-row GEMM, kept with
the hypothesis' label sequence), one joint step (csrc/transducer_step.hip: two launches giving lp_blank and
the top beam_k non-blank log-probabilities with their ids) and one small device-to-host copy of those.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple, Union

import torch

from ..._lib import RNNT_STEP_MAX_K


@dataclass
class Hypothesis:
    """Default hypothesis definition for Transducer search algorithms."""

    score: float
    yseq: List[int]
    dec_state: Union[Tuple[torch.Tensor, Optional[torch.Tensor]], List[Optional[torch.Tensor]], torch.Tensor]
    lm_state: Union[Dict[str, Any], List[Any]] = None


class BeamSearchTransducer:
    def __init__(self, decoder, joint_network, beam_size: int, lm: torch.nn.Module = None, lm_weight: float = 0.1,
                 search_type: str = "default", max_sym_exp: int = 2, u_max: int = 50, nstep: int = 1,
                 prefix_alpha: int = 1, expansion_gamma: int = 2.3, expansion_beta: int = 2, score_norm: bool = True,
                 nbest: int = 1, token_list: Optional[List[str]] = None):
        self.decoder = decoder
        self.joint_network = joint_network
        self.beam_size = beam_size
        self.hidden_size = decoder.dunits
        self.vocab_size = decoder.odim
        self.sos = self.vocab_size - 1
        self.token_list = token_list
        self.blank_id = decoder.blank_id
        if self.blank_id != 0:
            raise NotImplementedError(f"espnet_amd BeamSearchTransducer: blank_id={self.blank_id} is not built "
                                      "(the joint-step kernel uses blank = 0)")
        if lm is not None:
            raise NotImplementedError("espnet_amd BeamSearchTransducer: lm is not built (no LM shallow fusion in the "
                                      "transducer search)")
        if beam_size > RNNT_STEP_MAX_K:
            raise NotImplementedError(f"espnet_amd BeamSearchTransducer: beam_size={beam_size} is not built (up to "
                                      f"{RNNT_STEP_MAX_K}, the joint-step kernel's selection width)")
        if self.beam_size <= 1:
            self.search_algorithm = self.greedy_search
        elif search_type == "default":
            self.search_algorithm = self.default_beam_search
        elif search_type in ("tsd", "alsd", "nsc", "maes"):
            raise NotImplementedError(f"espnet_amd BeamSearchTransducer: search_type={search_type!r} is not built "
                                      "(only 'default' and the greedy search)")
        else:
            raise NotImplementedError
        self.use_lm = False
        self.lm = None
        self.lm_weight = lm_weight
        self.score_norm = score_norm
        self.nbest = nbest

    @torch.no_grad()
    def __call__(self, enc_out: torch.Tensor) -> List[Hypothesis]:
        """enc_out (T, D_enc) -> the n-best hypotheses."""
        self.decoder.set_device(enc_out.device)
        return self.search_algorithm(enc_out)

    def sort_nbest(self, hyps: List[Hypothesis]) -> List[Hypothesis]:
        if self.score_norm:
            hyps.sort(key=lambda x: x.score / len(x.yseq), reverse=True)
        else:
            hyps.sort(key=lambda x: x.score, reverse=True)
        return hyps[: self.nbest]

    def _frames(self, enc_out):
        """-> (E (T, J), frame[t]: the (1,) int32 device views that address its rows)."""
        E = self.joint_network.project_enc(enc_out.float())
        return E, torch.arange(E.shape[0], dtype=torch.int32, device=E.device).split(1)

    def _joint_operand(self, hyp, cache, cache_d):
        """decoder.score and lin_dec of its output, the latter kept per label sequence like the former."""
        dec_out, state, _ = self.decoder.score(hyp, cache)
        key = "_".join(map(str, hyp.yseq))
        D = cache_d.get(key)
        if D is None:
            D = cache_d[key] = self.joint_network.project_dec(dec_out[None])
        return D, state

    def greedy_search(self, enc_out: torch.Tensor) -> List[Hypothesis]:
        """At most one symbol per frame; the score sums the emitted tokens' log-probabilities."""
        E, frames = self._frames(enc_out)
        hyp = Hypothesis(score=0.0, yseq=[self.blank_id], dec_state=self.decoder.init_state(1))
        cache, cache_d = {}, {}
        D, state = self._joint_operand(hyp, cache, cache_d)
        for frame in frames:
            lp_blank, top, ids = self.joint_network.step(E, frame, D, 1).host()
            if top[0][0] > lp_blank[0]:  # torch.max returns the first maximum: blank, at index 0, wins ties
                hyp.yseq.append(ids[0][0])
                hyp.score += top[0][0]
                hyp.dec_state = state
                D, state = self._joint_operand(hyp, cache, cache_d)
        return [hyp]

    def default_beam_search(self, enc_out: torch.Tensor) -> List[Hypothesis]:
        """The beam search of https://arxiv.org/pdf/1211.3711.pdf as the reference modifies it."""
        beam = min(self.beam_size, self.vocab_size)
        beam_k = min(beam, self.vocab_size - 1)
        E, frames = self._frames(enc_out)
        kept_hyps = [Hypothesis(score=0.0, yseq=[self.blank_id], dec_state=self.decoder.init_state(1))]
        cache, cache_d = {}, {}
        for frame in frames:
            hyps = kept_hyps
            kept_hyps = []
            while True:
                max_hyp = max(hyps, key=lambda x: x.score)
                hyps.remove(max_hyp)
                D, state = self._joint_operand(max_hyp, cache, cache_d)
                lp_blank, top, ids = self.joint_network.step(E, frame, D, beam_k).host()
                kept_hyps.append(Hypothesis(score=max_hyp.score + lp_blank[0], yseq=max_hyp.yseq[:],
                                            dec_state=max_hyp.dec_state, lm_state=max_hyp.lm_state))
                for logp, k in zip(top[0], ids[0]):
                    hyps.append(Hypothesis(score=max_hyp.score + logp, yseq=max_hyp.yseq[:] + [k], dec_state=state,
                                           lm_state=max_hyp.lm_state))
                hyps_max = float(max(hyps, key=lambda x: x.score).score)
                kept_most_prob = sorted([hyp for hyp in kept_hyps if hyp.score > hyps_max], key=lambda x: x.score)
                if len(kept_most_prob) >= beam:
                    kept_hyps = kept_most_prob
                    break
        return self.sort_nbest(kept_hyps)
