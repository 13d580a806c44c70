"""Language models for shallow fusion in decoding (espnet2/lm)."""
from .seq_rnn_lm import SequentialRNNLM  # noqa: F401
from .transformer_lm import TransformerLM  # noqa: F401

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
