"""ESPnetLanguageModel — espnet2/lm/espnet_model.py on the HIP path: the LM task's model.

nll builds the sentence pair x = <eos> w1 .. wn, t = w1 .. wn <sos> (sos = eos = vocab_size - 1),
runs the LM over the whole padded batch and masks the loss by length.  The cross-entropy is
ea_lsm_loss_fwd / ea_lsm_loss_bwd with smoothing 0.  That kernel masks rows by target id where
the reference masks by length, and the two differ when ignore_id occurs inside a sentence; so the
kernel is given -1 as its ignore id and the targets of the padded positions are set to -1 from
the lengths: a token equal to ignore_id inside a sentence is scored, as in the reference.

Only the mean loss is differentiable (forward); the per-token nll that nll / batchify_nll
return carries no gradient (the reference computes perplexities from it under no_grad).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from ..asr.espnet_model import AbsESPnetModel
from .rnn_train import CrossEntropyFn
from .seq_rnn_lm import SequentialRNNLM


class ESPnetLanguageModel(AbsESPnetModel):
    def __init__(self, lm: nn.Module, vocab_size: int, ignore_id: int = 0):
        super().__init__()
        self.lm = lm
        self.sos = vocab_size - 1
        self.eos = vocab_size - 1
        # the pad id of the collated text (0 by default, the id ASR keeps for the CTC blank)
        self.ignore_id = ignore_id
        self.arena = None

    def prepare(self, device="cuda", amp: bool = False, seed: int = 0):
        """Prepare the LM for training on `device`; exposes its arena for the optimizer."""
        if not isinstance(self.lm, SequentialRNNLM):
            raise NotImplementedError(f"espnet_amd {type(self.lm).__name__} is a decoding scorer (no training): "
                                      "the LM task trains lm: seq_rnn")
        self.lm.prepare(device, amp=amp, train=True, seed=seed, owner=self)
        self.arena, self._device = self.lm.arena, self.lm._device
        return self

    # ------------------------------------------------------------------ the sentence pair
    def make_xt(self, text: torch.Tensor, text_lengths: torch.Tensor, max_length: Optional[int] = None):
        """espnet_model.py:38-51 -> (x, t, x_lengths), each on text's device.  Without
        max_length the batch is cut to its longest sentence when text_lengths are in host
        memory.  Lengths on the device are not read back (that would stall the launch queue once
        per step): the padded width is kept, which is the longest sentence for a collated batch;
        an over-padded device batch gives a wider nll than the reference's, zero in the extra
        columns, and the same loss."""
        if max_length is None:
            if text_lengths.device.type == "cpu":
                text = text[:, :int(text_lengths.max())]
        else:
            text = text[:, :int(max_length)]
        lengths = text_lengths.to(text.device)
        x = F.pad(text, [1, 0], "constant", self.eos)
        t = F.pad(text, [0, 1], "constant", self.ignore_id)
        t.scatter_(1, lengths.view(-1, 1).to(torch.int64), self.sos)
        return x, t, lengths + 1

    def nll(self, text: torch.Tensor, text_lengths: torch.Tensor, max_length: Optional[int] = None
            ) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (nll (Batch, Length + 1), 0 past each sentence's end; x_lengths)."""
        nll, x_lengths, _ = self._nll(text, text_lengths, max_length)
        return nll, x_lengths

    def _nll(self, text, text_lengths, max_length=None):
        if self.arena is None:
            raise RuntimeError("ESPnetLanguageModel.prepare(device) first")
        dev = self._device
        x, t, x_lengths = self.make_xt(text, text_lengths, max_length)
        x, t, x_lengths = x.to(dev), t.to(dev), x_lengths.to(dev)
        B, L = x.shape
        y, _ = self.lm(x, None)  # (B, L, V): a transposed view of time-major rows when training
        V = y.shape[-1]
        pad = torch.arange(L, device=dev).unsqueeze(0) >= x_lengths.unsqueeze(1)  # make_pad_mask
        # time-major rows, masked positions -> -1 (the kernel's ignore id here)
        tgt = t.clamp(0, V - 1).masked_fill(pad, -1).t().contiguous().view(-1)
        rows = y.transpose(0, 1).reshape(L * B, V)
        if rows.dtype != torch.float32 or not rows.is_contiguous():
            rows = rows.float().contiguous()
        loss, nll_rows = CrossEntropyFn.apply(rows, tgt)
        return nll_rows.view(L, B).t(), x_lengths, loss

    def batchify_nll(self, text: torch.Tensor, text_lengths: torch.Tensor, batch_size: int = 100
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
        """espnet_model.py:72-112: nll in slices of batch_size sentences, all padded to the
        longest sentence of the whole input."""
        total_num = text.size(0)
        if total_num <= batch_size:
            nll, x_lengths = self.nll(text, text_lengths)
        else:
            nlls, x_lengths = [], []
            max_length = int(text_lengths.max())
            for start in range(0, total_num, batch_size):
                end = min(start + batch_size, total_num)
                batch_nll, batch_x_lengths = self.nll(text[start:end, :], text_lengths[start:end],
                                                      max_length=max_length)
                nlls.append(batch_nll)
                x_lengths.append(batch_x_lengths)
            nll = torch.cat(nlls)
            x_lengths = torch.cat(x_lengths)
        assert nll.size(0) == total_num
        assert x_lengths.size(0) == total_num
        return nll, x_lengths

    def forward(self, text: torch.Tensor, text_lengths: torch.Tensor, **kwargs
                ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor], torch.Tensor]:
        """-> (loss = nll.sum() / ntokens, {"loss"}, ntokens)."""
        _, x_lengths, loss = self._nll(text, text_lengths)
        ntokens = x_lengths.sum()
        return loss, dict(loss=loss.detach()), ntokens

    def collect_feats(self, text: torch.Tensor, text_lengths: torch.Tensor, **kwargs) -> Dict[str, torch.Tensor]:
        return {}
