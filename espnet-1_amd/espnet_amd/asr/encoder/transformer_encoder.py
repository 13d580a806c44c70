"""TransformerEncoder — drop-in for espnet2/asr/encoder/transformer_encoder.py:37-232
(BASELINE.json configs[0]: the Transformer-tiny of egs2/mini_an4).

Same constructor signature and state_dict layout (embed.conv.{0,2}, embed.out.0,
encoders.{i}.{self_attn,feed_forward,norm1,norm2}, after_norm); forward runs the HIP
path: Conv2dSubsampling with the absolute PositionalEncoding (subsampling.py:57-69 with
PositionalEncoding(odim, dropout_rate) — the reference passes the encoder's dropout_rate,
not positional_dropout_rate, to it) -> N x TransformerBlockFn -> after_norm.  Options the
ASR recipes do not use (other input layers, conv1d feed-forward, concat_after,
normalize_before=False, interCTC) raise NotImplementedError.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import nn

from ...layers.conformer import MultiHeadedAttention, PositionwiseFeedForward
from ...layers.decoder import PositionalEncoding
from ...layers.subsampling import Conv2dSubsampling
from ...layers.transformer import TransformerEncoderLayer
from .abs_encoder import INPUT_LAYERS, AfterNorm, SubsamplingEncoder


class TransformerEncoder(SubsamplingEncoder):
    layer_class = TransformerEncoderLayer

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
        input_layer: Optional[str] = "conv2d",
        pos_enc_class=None,
        normalize_before: bool = True,
        concat_after: bool = False,
        positionwise_layer_type: str = "linear",
        positionwise_conv_kernel_size: int = 1,
        padding_idx: int = -1,
        interctc_layer_idx: List[int] = [],
        interctc_use_conditioning: bool = False,
    ):
        super().__init__()
        self._output_size = output_size
        if input_layer not in INPUT_LAYERS and input_layer is not None:
            raise ValueError("unknown input_layer: " + str(input_layer))
        if positionwise_layer_type not in ("linear", "conv1d", "conv1d-linear"):
            raise NotImplementedError("Support only linear or conv1d.")
        unsupported = []
        if input_layer != "conv2d":
            unsupported.append(f"input_layer={input_layer}")
        if positionwise_layer_type != "linear":
            unsupported.append(f"positionwise_layer_type={positionwise_layer_type}")
        if pos_enc_class is not None and pos_enc_class is not PositionalEncoding:
            unsupported.append("pos_enc_class")
        if not normalize_before or concat_after:
            unsupported.append("normalize_before=False/concat_after")
        if interctc_layer_idx:
            unsupported.append("interctc")
        if unsupported:
            raise NotImplementedError("espnet_amd TransformerEncoder implements the ASR recipes' "
                                      "configuration only; unsupported: " + ", ".join(unsupported))
        if output_size % 8:
            raise ValueError("output_size must be a multiple of 8 (16-B aligned MFMA operands)")
        self.embed = Conv2dSubsampling(input_size, output_size, dropout_rate,
                                       PositionalEncoding(output_size, dropout_rate))
        self.normalize_before = normalize_before
        layers = []
        for lnum in range(num_blocks):
            layers.append(TransformerEncoderLayer(
                output_size, MultiHeadedAttention(attention_heads, output_size, attention_dropout_rate),
                PositionwiseFeedForward(output_size, linear_units, dropout_rate, activation="relu"),
                dropout_rate, normalize_before, concat_after))
            layers[-1].layer_idx = lnum + 1
        self.encoders = nn.Sequential(*layers)
        self.after_norm = AfterNorm(output_size, eps=1e-12)
        self.interctc_layer_idx = interctc_layer_idx
        self.interctc_use_conditioning = interctc_use_conditioning
        self.conditioning_layer = None

    def forward(self, xs_pad: torch.Tensor, ilens: torch.Tensor, prev_states=None, ctc=None,
                seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        """transformer_encoder.py:184-232.  xs_pad (B,T,F) f32 on the GPU, ilens (B,) int64."""
        x, olens = self.front(xs_pad, ilens, seed)
        return self.run_layers(x, olens, seed), olens, None
