"""AbsEncoder (espnet2/asr/encoder/abs_encoder.py) and what the Conv2dSubsampling encoders
(Conformer, E-Branchformer, Transformer) share: the subsampling front, the arena binding, the
layer loop with after_norm, and the reference's option tables.

`SubsamplingEncoder.__init__` creates no module and no parameter: each encoder's constructor
builds `embed`, `encoders`, `after_norm` itself, in the reference's order (the seeded
initialisation and the state_dict key order follow attribute creation order).
"""
from __future__ import annotations

import torch
from torch import nn

from ... import hip_ops as ops
from ..._lib import lib
from ...layers.common import Bound, LayerNormFn, multisequential_draw, site_seed

# the reference's input_layer names (conformer_encoder.py:145-202 and the other encoders' same chain)
INPUT_LAYERS = ("linear", "conv2d", "conv2d1", "conv2d2", "conv2d6", "conv2d8", "embed")


class TooShortUttError(Exception):
    """subsampling.py:14-28"""

    def __init__(self, message, actual_size, limit):
        super().__init__(message)
        self.actual_size = actual_size
        self.limit = limit


class AbsEncoder(nn.Module):
    def output_size(self) -> int:
        raise NotImplementedError


class AfterNorm(nn.LayerNorm):
    def bind(self, arena, prefix, cd):
        self._b = Bound(arena, prefix, cd)


def resolve_rel_pos_type(rel_pos_type, pos_enc_layer_type, attn_layer_type):
    """conformer_encoder.py:117-126 / e_branchformer_encoder.py:215-224: `legacy` renames the
    rel-pos choices to their legacy variants, `latest` refuses them.  -> (pos_enc_layer_type,
    attention layer type)."""
    if rel_pos_type == "legacy":
        if pos_enc_layer_type == "rel_pos":
            pos_enc_layer_type = "legacy_rel_pos"
        if attn_layer_type == "rel_selfattn":
            attn_layer_type = "legacy_rel_selfattn"
    elif rel_pos_type == "latest":
        assert attn_layer_type != "legacy_rel_selfattn"
        assert pos_enc_layer_type != "legacy_rel_pos"
    else:
        raise ValueError("unknown rel_pos_type: " + rel_pos_type)
    return pos_enc_layer_type, attn_layer_type


class SubsamplingEncoder(AbsEncoder):
    """Conv2dSubsampling `embed` -> `encoders` (a Sequential of `layer_class` blocks) ->
    `after_norm`.  A subclass sets `layer_class` and `_output_size` and builds the three modules."""

    layer_class = None

    def output_size(self) -> int:
        return self._output_size

    def arena_groups(self, prefix=""):
        g = []
        for i in range(len(self.encoders)):
            g += self.layer_class.arena_groups(f"{prefix}encoders.{i}.")
        return g

    def bind(self, arena, prefix, cd, anchor):
        self.embed.bind(arena, prefix + "embed.", cd)
        self.embed._anchor = anchor
        for i, layer in enumerate(self.encoders):
            layer.bind(arena, f"{prefix}encoders.{i}.", cd)
        self.after_norm.bind(arena, prefix + "after_norm.", cd)
        if getattr(self, "conditioning_layer", None) is not None:
            self.conditioning_layer.bind(arena, prefix + "conditioning_layer.", cd)
        self._cd = cd

    def front(self, xs_pad, ilens, seed, layerdrop_draw=True):
        """Short-utterance check, subsampled lengths and `embed`; then the host generator draw of
        the reference's MultiSequential.forward (before any positional table is made).
        -> (x (B, T', d) f32, olens (B,) int64)."""
        B, T, _ = xs_pad.shape
        if T < 7:  # check_short_utt, subsampling.py:31-43
            raise TooShortUttError(f"has {T} frames and is too short for subsampling "
                                   f"(it needs more than 7 frames), return empty results", T, 7)
        xs_pad = xs_pad.contiguous()
        olens = torch.empty(B, dtype=torch.long, device=xs_pad.device)
        lib.ea_subsample_lens(B, T, ilens.data_ptr(), olens.data_ptr(), ops.stream())
        x = self.embed(xs_pad, seed)
        if layerdrop_draw:
            multisequential_draw(len(self.encoders))
        return x, olens

    def rel_pos_emb(self, x, seed):
        """The rel-pos table of `embed`'s positional encoding for x's length, in the compute dtype."""
        return self.embed.out[1].pos_emb(x.shape[1], x.device, self._cd, self.training, site_seed(seed, 0, 9))

    def run_layers(self, x, *args):
        """x through every block (`args`: what the block takes after x), then after_norm."""
        for layer in self.encoders:
            x = layer(x, *args)
        return LayerNormFn.apply(x, self.after_norm)
