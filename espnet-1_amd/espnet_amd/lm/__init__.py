"""Language models (espnet2/lm): decoding scorers for shallow fusion, and the LM task's model
(ESPnetLanguageModel) that trains `lm: seq_rnn`."""
from .seq_rnn_lm import SequentialRNNLM  # noqa: F401
from .transformer_lm import TransformerLM  # noqa: F401
from .espnet_model import ESPnetLanguageModel  # noqa: F401

LM_CHOICES = {"seq_rnn": SequentialRNNLM, "transformer": TransformerLM}


def build_lm(lm: str = None, lm_conf: dict = None, vocab_size: int = None):
    """The LM task's class choice (espnet2/tasks/lm.py:24-33: `lm: seq_rnn | transformer`,
    default seq_rnn) applied to a recipe's `lm` / `lm_conf` block."""
    name = "seq_rnn" if lm is None else lm
    if name not in LM_CHOICES:
        raise ValueError(f"lm must be one of {sorted(LM_CHOICES)}: {lm!r}")
    if vocab_size is None:
        raise ValueError("build_lm needs vocab_size (the length of the token list)")
    return LM_CHOICES[name](vocab_size=vocab_size, **(lm_conf or {}))


def lm_state_dict(path, map_location="cpu"):
    """The LM's own state_dict from a file the LM task wrote: a model file ({n}epoch.pth,
    valid.loss.best.pth, valid.loss.ave.pth) or checkpoint.pth (its "model" entry), with the
    ESPnetLanguageModel prefix `lm.` removed — what build_lm(...).load_state_dict takes, as
    espnet2/bin/asr_inference.py:149-183 takes `lm.lm` of the LM task's model."""
    import torch
    sd = torch.load(path, map_location=map_location, weights_only=True)
    if "model" in sd and isinstance(sd["model"], dict):
        sd = sd["model"]
    return {k[3:] if k.startswith("lm.") else k: v for k, v in sd.items()}
