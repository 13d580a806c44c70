"""ConformerEncoder — drop-in for espnet2/asr/encoder/conformer_encoder.py:49-377.

Same constructor signature, option validation and state_dict layout; forward runs the
HIP path: Conv2dSubsampling (SubsampleFn) -> N x ConformerBlockFn -> after_norm, with an
InterCTCTapFn (layers/interctc.py) behind every layer in interctc_layer_idx.
Only the configuration the reference's ASR recipes train (input_layer conv2d,
rel_pos_type latest or legacy, (legacy_)rel_pos / (legacy_)rel_selfattn, macaron, conv module,
normalize_before, intermediate / self-conditioned CTC) is implemented; other choices raise NotImplementedError
instead of silently diverging.
"""
from __future__ import annotations

import logging
from typing import List, Optional, Tuple, Union

import torch
from torch import nn

from ...layers.common import LayerNormFn
from ...layers.conformer import (ConvolutionModule, EncoderLayer, LayerNorm,
                                 PositionwiseFeedForward, RelPositionMultiHeadedAttention)
from ...layers.interctc import InterCTCTapFn, TapState
from ...layers.subsampling import Conv2dSubsampling, LegacyRelPositionalEncoding, RelPositionalEncoding
from .abs_encoder import INPUT_LAYERS, AfterNorm, SubsamplingEncoder, resolve_rel_pos_type


class ConditioningLayer(nn.Linear):
    """Linear(vocab_size, output_size) of self-conditioned CTC (espnet_model.py:105-108):
    x + conditioning_layer(softmax(ctc_lo(after_norm(x)))) at every tap; run by InterCTCTapFn."""

    _b = None

    def bind(self, arena, prefix, cd):
        from ...layers.common import Bound
        self._b = Bound(arena, prefix, cd)


class ConformerEncoder(SubsamplingEncoder):
    layer_class = EncoderLayer

    def __init__(
        self,
        input_size: int,
        output_size: int = 256,
        attention_heads: int = 4,
        linear_units: int = 2048,
        num_blocks: int = 6,
        dropout_rate: float = 0.1,
        positional_dropout_rate: float = 0.1,
        attention_dropout_rate: float = 0.0,
        input_layer: str = "conv2d",
        normalize_before: bool = True,
        concat_after: bool = False,
        positionwise_layer_type: str = "linear",
        positionwise_conv_kernel_size: int = 3,
        macaron_style: bool = False,
        rel_pos_type: str = "legacy",
        pos_enc_layer_type: str = "rel_pos",
        selfattention_layer_type: str = "rel_selfattn",
        activation_type: str = "swish",
        use_cnn_module: bool = True,
        zero_triu: bool = False,
        cnn_module_kernel: int = 31,
        padding_idx: int = -1,
        interctc_layer_idx: List[int] = [],
        interctc_use_conditioning: bool = False,
        stochastic_depth_rate: Union[float, List[float]] = 0.0,
        layer_drop_rate: float = 0.0,
        max_pos_emb_len: int = 5000,
    ):
        super().__init__()
        self._output_size = output_size
        # option resolution as conformer_encoder.py:117-143
        pos_enc_layer_type, selfattention_layer_type = resolve_rel_pos_type(
            rel_pos_type, pos_enc_layer_type, selfattention_layer_type)
        if pos_enc_layer_type not in ("abs_pos", "scaled_abs_pos", "rel_pos", "legacy_rel_pos"):
            raise ValueError("unknown pos_enc_layer: " + pos_enc_layer_type)
        if selfattention_layer_type not in ("selfattn", "legacy_rel_selfattn", "rel_selfattn"):
            raise ValueError("unknown encoder_attn_layer: " + selfattention_layer_type)
        if input_layer not in INPUT_LAYERS and not isinstance(input_layer, nn.Module) and input_layer is not None:
            raise ValueError("unknown input_layer: " + str(input_layer))
        unsupported = []
        # conformer_encoder.py:155-196: each rel-pos attention asserts its own positional encoding
        if pos_enc_layer_type == "rel_pos":
            assert selfattention_layer_type == "rel_selfattn"
        elif pos_enc_layer_type == "legacy_rel_pos":
            assert selfattention_layer_type == "legacy_rel_selfattn"
            logging.warning("Using legacy_rel_pos and it will be deprecated in the future.")
        if selfattention_layer_type == "rel_selfattn":
            assert pos_enc_layer_type == "rel_pos"
        elif selfattention_layer_type == "legacy_rel_selfattn":
            assert pos_enc_layer_type == "legacy_rel_pos"
            logging.warning("Using legacy_rel_selfattn and it will be deprecated in the future.")
        legacy = selfattention_layer_type == "legacy_rel_selfattn"
        if (pos_enc_layer_type, selfattention_layer_type) not in (("rel_pos", "rel_selfattn"),
                                                                  ("legacy_rel_pos", "legacy_rel_selfattn")):
            unsupported.append(f"{pos_enc_layer_type}/{selfattention_layer_type}")
        if input_layer != "conv2d":
            unsupported.append(f"input_layer={input_layer}")
        if positionwise_layer_type != "linear":
            unsupported.append(f"positionwise_layer_type={positionwise_layer_type}")
        if activation_type != "swish":
            unsupported.append(f"activation_type={activation_type}")
        if stochastic_depth_rate not in (0, 0.0) or layer_drop_rate > 0:
            unsupported.append("stochastic depth/layer drop")
        if not normalize_before or concat_after or not use_cnn_module:
            unsupported.append("normalize_before=False/concat_after/use_cnn_module=False")
        if unsupported:
            raise NotImplementedError("espnet_amd ConformerEncoder implements the ASR recipes' "
                                      "configuration only; unsupported: " + ", ".join(unsupported))
        if output_size % 8:
            raise ValueError("output_size must be a multiple of 8 (16-B aligned MFMA operands)")
        pos_enc_class = LegacyRelPositionalEncoding if legacy else RelPositionalEncoding
        self.embed = Conv2dSubsampling(input_size, output_size, dropout_rate,
                                       pos_enc_class(output_size, positional_dropout_rate, max_pos_emb_len))
        self.normalize_before = normalize_before
        layers = []
        for lnum in range(num_blocks):
            layers.append(EncoderLayer(
                output_size,
                RelPositionMultiHeadedAttention(attention_heads, output_size, attention_dropout_rate, zero_triu,
                                                legacy=legacy),
                PositionwiseFeedForward(output_size, linear_units, dropout_rate),
                PositionwiseFeedForward(output_size, linear_units, dropout_rate) if macaron_style else None,
                ConvolutionModule(output_size, cnn_module_kernel),
                dropout_rate, normalize_before, concat_after, 0.0))
            layers[-1].layer_idx = lnum + 1
        self.encoders = nn.Sequential(*layers)
        self.after_norm = AfterNorm(output_size, eps=1e-12)
        self.interctc_layer_idx = interctc_layer_idx
        if len(interctc_layer_idx) > 0:  # conformer_encoder.py:292-293
            assert 0 < min(interctc_layer_idx) and max(interctc_layer_idx) < num_blocks
        self.interctc_use_conditioning = interctc_use_conditioning
        self.conditioning_layer = None  # ESPnetASRModel creates it (a ConditioningLayer), as the reference does
        self._taps = TapState()

    def forward(self, xs_pad: torch.Tensor, ilens: torch.Tensor, prev_states=None, ctc=None,
                seed: int = 0, interctc_targets=None) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        """conformer_encoder.py:300-377.  xs_pad (B,T,F) f32 on the GPU, ilens (B,) int64.

        With interctc_layer_idx the first result is (x, [(layer, y_layer), ...]) like the
        reference's, the y the taps' after_norm outputs.  `ctc`: the model's CTC head — the taps
        run its projection here (layers/interctc.py), for the conditioning and, given
        `interctc_targets` = (text (B, Lmax) padded with -1, text_lengths), for their losses,
        left in `self.interctc_losses` as [(layer, loss)] (espnet_model.py:242-286 computes them
        from the returned y; here the loss shares the tap's logits with the conditioning)."""
        taps = self.interctc_layer_idx
        # (with taps the reference loops over the layers itself, conformer_encoder.py:345: no
        # MultiSequential.forward, so no layer-drop draw from the host generator)
        x, olens = self.front(xs_pad, ilens, seed, layerdrop_draw=not taps)
        pos = self.rel_pos_emb(x, seed)
        if not taps:
            return self.run_layers(x, pos, olens, seed), olens, None
        if ctc is None and self.interctc_use_conditioning:
            raise ValueError("interctc_use_conditioning needs the CTC head: encoder(..., ctc=model.ctc)")
        ys = ylens = None
        Lmax = 0
        if interctc_targets is not None and ctc is not None:
            ys, ylens = interctc_targets
            ys = ys.contiguous()
            Lmax = int(ys.shape[1])
        # the taps and the final after_norm / CTC head write the same gradients: the lowest tap
        # reports them ready (TapState), when this forward builds a graph through the taps
        in_graph = ctc is not None and torch.is_grad_enabled() and x.requires_grad and (
            self.interctc_use_conditioning or ys is not None)
        self._taps.arm(in_graph, self.after_norm, ctc)
        intermediate_outs, losses = [], []
        for li, layer in enumerate(self.encoders):
            x = layer(x, pos, olens, seed)
            if li + 1 in taps:
                if ctc is None:
                    intermediate_outs.append((li + 1, LayerNormFn.apply(x, self.after_norm)))
                    continue
                x, loss_ic, y = InterCTCTapFn.apply(x, olens, ys, ylens, self, ctc, Lmax, not intermediate_outs)
                intermediate_outs.append((li + 1, y))
                if ys is not None:
                    losses.append((li + 1, loss_ic))
        self.interctc_losses = losses
        x = LayerNormFn.apply(x, self.after_norm)
        return (x, intermediate_outs), olens, None
