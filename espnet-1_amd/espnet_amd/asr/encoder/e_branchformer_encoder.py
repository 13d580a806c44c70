"""EBranchformerEncoder — drop-in for espnet2/asr/encoder/e_branchformer_encoder.py:180-430.

Same constructor signature, defaults, option validation and state_dict layout; forward runs the
HIP path: Conv2dSubsampling (SubsampleFn) -> N x EBranchformerBlockFn -> after_norm.  Only the
configuration the reference's LibriSpeech E-Branchformer recipes train is implemented
(rel_selfattn / rel_pos / latest, input_layer conv2d, linear position-wise layers with swish,
use_ffn with or without the macaron FFN, identity gate activation, no linear after the
convolution, no layer drop); every other valid choice raises NotImplementedError naming the
option instead of silently diverging, invalid ones raise what the reference raises.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import nn

from ...layers.conformer import PositionwiseFeedForward, RelPositionMultiHeadedAttention
from ...layers.ebranchformer import CONV_KERNELS, ConvolutionalGatingMLP, EBranchformerEncoderLayer
from ...layers.subsampling import Conv2dSubsampling, RelPositionalEncoding
from .abs_encoder import INPUT_LAYERS, AfterNorm, SubsamplingEncoder, resolve_rel_pos_type

# espnet/nets/pytorch_backend/nets_utils.py get_activation
_ACTIVATIONS = ("hardtanh", "tanh", "relu", "selu", "swish")


class EBranchformerEncoder(SubsamplingEncoder):
    layer_class = EBranchformerEncoderLayer

    def __init__(
        self,
        input_size: int,
        output_size: int = 256,
        attention_heads: int = 4,
        attention_layer_type: str = "rel_selfattn",
        pos_enc_layer_type: str = "rel_pos",
        rel_pos_type: str = "latest",
        cgmlp_linear_units: int = 2048,
        cgmlp_conv_kernel: int = 31,
        use_linear_after_conv: bool = False,
        gate_activation: str = "identity",
        num_blocks: int = 12,
        dropout_rate: float = 0.1,
        positional_dropout_rate: float = 0.1,
        attention_dropout_rate: float = 0.0,
        input_layer: Optional[str] = "conv2d",
        zero_triu: bool = False,
        padding_idx: int = -1,
        layer_drop_rate: float = 0.0,
        max_pos_emb_len: int = 5000,
        use_ffn: bool = False,
        macaron_ffn: bool = False,
        ffn_activation_type: str = "swish",
        linear_units: int = 2048,
        positionwise_layer_type: str = "linear",
        merge_conv_kernel: int = 3,
    ):
        super().__init__()
        self._output_size = output_size
        # option resolution and validation as e_branchformer_encoder.py:215-352
        pos_enc_layer_type, attention_layer_type = resolve_rel_pos_type(
            rel_pos_type, pos_enc_layer_type, attention_layer_type)
        if pos_enc_layer_type == "rel_pos":
            assert attention_layer_type == "rel_selfattn"
        elif pos_enc_layer_type == "legacy_rel_pos":
            assert attention_layer_type == "legacy_rel_selfattn"
        elif pos_enc_layer_type not in ("abs_pos", "scaled_abs_pos"):
            raise ValueError("unknown pos_enc_layer: " + pos_enc_layer_type)
        if input_layer not in INPUT_LAYERS and not isinstance(input_layer, nn.Module) and input_layer is not None:
            raise ValueError("unknown input_layer: " + input_layer)
        if ffn_activation_type not in _ACTIVATIONS:  # get_activation's lookup
            raise KeyError(ffn_activation_type)
        if positionwise_layer_type != "linear" and positionwise_layer_type is not None:
            raise ValueError("Support only linear.")
        if attention_layer_type == "legacy_rel_selfattn":
            assert pos_enc_layer_type == "legacy_rel_pos"
        elif attention_layer_type == "rel_selfattn":
            assert pos_enc_layer_type == "rel_pos"
        elif attention_layer_type == "fast_selfattn":
            assert pos_enc_layer_type in ["abs_pos", "scaled_abs_pos"]
        elif attention_layer_type != "selfattn":
            raise ValueError("unknown encoder_attn_layer: " + attention_layer_type)
        if gate_activation != "identity" and gate_activation not in _ACTIVATIONS:
            raise KeyError(gate_activation)
        # what the HIP path implements
        unsupported = []
        if attention_layer_type != "rel_selfattn" or pos_enc_layer_type != "rel_pos":
            unsupported.append(f"attention_layer_type={attention_layer_type} / pos_enc_layer_type={pos_enc_layer_type}"
                               f" (rel_pos_type={rel_pos_type})")
        if input_layer != "conv2d":
            unsupported.append(f"input_layer={input_layer}")
        if positionwise_layer_type != "linear":
            unsupported.append(f"positionwise_layer_type={positionwise_layer_type}")
        if ffn_activation_type != "swish":
            unsupported.append(f"ffn_activation_type={ffn_activation_type}")
        if not use_ffn:
            unsupported.append("use_ffn=False")
        if use_linear_after_conv:
            unsupported.append("use_linear_after_conv=True")
        if gate_activation != "identity":
            unsupported.append(f"gate_activation={gate_activation}")
        if layer_drop_rate > 0:
            unsupported.append(f"layer_drop_rate={layer_drop_rate}")
        if zero_triu:
            unsupported.append("zero_triu=True")
        if cgmlp_conv_kernel not in CONV_KERNELS:
            unsupported.append(f"cgmlp_conv_kernel={cgmlp_conv_kernel} (implemented: {CONV_KERNELS})")
        if merge_conv_kernel not in CONV_KERNELS:
            unsupported.append(f"merge_conv_kernel={merge_conv_kernel} (implemented: {CONV_KERNELS})")
        if cgmlp_linear_units % 16:
            unsupported.append(f"cgmlp_linear_units={cgmlp_linear_units} (a multiple of 16)")
        if unsupported:
            raise NotImplementedError("espnet_amd EBranchformerEncoder implements the LibriSpeech recipes' "
                                      "configuration only; unsupported: " + ", ".join(unsupported))
        if output_size % 8:
            raise ValueError("output_size must be a multiple of 8 (16-B aligned MFMA operands)")
        self.embed = Conv2dSubsampling(input_size, output_size, dropout_rate,
                                       RelPositionalEncoding(output_size, positional_dropout_rate, max_pos_emb_len))
        layers = []
        for lnum in range(num_blocks):
            # argument order = the reference's construction order (attn, cgmlp, ffn, macaron ffn)
            layers.append(EBranchformerEncoderLayer(
                output_size,
                RelPositionMultiHeadedAttention(attention_heads, output_size, attention_dropout_rate, zero_triu),
                ConvolutionalGatingMLP(output_size, cgmlp_linear_units, cgmlp_conv_kernel, dropout_rate,
                                       use_linear_after_conv, gate_activation),
                PositionwiseFeedForward(output_size, linear_units, dropout_rate) if use_ffn else None,
                PositionwiseFeedForward(output_size, linear_units, dropout_rate) if use_ffn and macaron_ffn else None,
                dropout_rate, merge_conv_kernel))
            layers[-1].layer_idx = lnum + 1
        self.encoders = nn.Sequential(*layers)
        self.after_norm = AfterNorm(output_size, eps=1e-12)

    def forward(self, xs_pad: torch.Tensor, ilens: torch.Tensor, prev_states=None,
                seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        """e_branchformer_encoder.py:384-430.  xs_pad (B,T,F) f32 on the GPU, ilens (B,) int64."""
        x, olens = self.front(xs_pad, ilens, seed)  # (with repeat()'s MultiSequential draw, repeat.py:27)
        pos = self.rel_pos_emb(x, seed)
        return self.run_layers(x, pos, olens, seed), olens, None
