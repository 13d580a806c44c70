"""LMTask — mirrors espnet2/tasks/lm.py: the `lm` class choice (:24-32), the task options
(:45-129), the collate function / data names (:131-173) and build_model (:175-207).

    python -m espnet_amd.bin.lm_train --config conf/train_lm.yaml --token_list tokens.txt \
        --train_data_path_and_name_and_type dump/lm_train.txt,text,text ...

What trains: `lm: seq_rnn` with rnn_type lstm (the LM task's default), --optim adam, on one GPU.
Steps are launched eagerly (the captured-step runner is shaped after the ASR batch).  Refused
by name: --ngpu > 1 and the distributed options, --optim other than adam (AbsTask), `lm:
transformer` (a decoding scorer: ESPnetLanguageModel.prepare raises), --token_type bpe (no
tokenizer model here; integer text, char and word work).
"""
from __future__ import annotations

import argparse
import logging
from typing import Tuple

import numpy as np

from ..lm import LM_CHOICES
from ..lm.espnet_model import ESPnetLanguageModel
from ..train.class_choices import ClassChoices
from ..train.collate_fn import CommonCollateFn
from ..train.trainer import Trainer
from ..utils.nested_dict_action import NestedDictAction
from ..utils.types import str2bool, str_or_none
from .abs_task import AbsTask, _default_kwargs
from .asr import _IntTextPreprocessor


class _LMTextPreprocessor(_IntTextPreprocessor):
    """The ASR task's text preprocessor (integer text passes through, "char" uses the token
    list) with "word" beside it: split at whitespace as WordTokenizer does
    (espnet2/text/word_tokenizer.py), words outside the token list -> "<unk>", which the list
    must hold as TokenIDConverter requires (espnet2/text/token_id_converter.py)."""

    def __call__(self, uid, data):
        text = data.get("text")
        if self.token_type != "word" or text is None or isinstance(text, np.ndarray) or self.token_list is None:
            return super().__call__(uid, data)
        unk = self.tok2id.get("<unk>")
        if unk is None:
            raise RuntimeError("Unknown symbol '<unk>' doesn't exist in the token_list")
        data["text"] = np.array([self.tok2id.get(w, unk) for w in str(text).split()], dtype=np.int64)
        return data


lm_choices = ClassChoices("lm", dict(LM_CHOICES), default="seq_rnn")
model_choices = ClassChoices("model", dict(lm=ESPnetLanguageModel), default="lm")


class LMTrainer(Trainer):
    """The generic trainer without the captured-step runner: every LM step is launched eagerly.
    At the start of an epoch the model's forward counter, which seeds its dropout streams, is set
    from the optimizer's applied-update count, so a resumed run goes on with new streams instead
    of repeating the first run's (one device read per epoch)."""
    capture_steps = False

    @classmethod
    def train_one_epoch(cls, model, iterator, optimizers, schedulers, *args, options=None, **kwargs):
        lm = getattr(model, "lm", None)
        if lm is not None and hasattr(lm, "_nstep"):
            lm._nstep = max(lm._nstep, optimizers[0].step_count * (options.accum_grad if options else 1))
        return super().train_one_epoch(model, iterator, optimizers, schedulers, *args, options=options, **kwargs)


class LMTask(AbsTask):
    num_optimizers: int = 1
    class_choices_list = [lm_choices, model_choices]
    trainer = LMTrainer

    @classmethod
    def add_task_arguments(cls, parser: argparse.ArgumentParser):
        g = parser.add_argument_group(description="Task related")
        required = parser.get_default("required")
        required += ["token_list"]
        g.add_argument("--token_list", type=str_or_none, default=None, help="A text mapping int-id to token")
        g.add_argument("--init", type=lambda x: str_or_none(x.lower()), default=None,
                       choices=["chainer", "xavier_uniform", "xavier_normal", "kaiming_uniform", "kaiming_normal",
                                None], help="The initialization method")
        g = parser.add_argument_group(description="Preprocess related")
        g.add_argument("--use_preprocessor", type=str2bool, default=True,
                       help="Tokenise string text with the token list")
        g.add_argument("--token_type", type=str, default="bpe", choices=["bpe", "char", "word"])
        g.add_argument("--bpemodel", type=str_or_none, default=None,
                       help="A sentencepiece model (refused: text must be tokenised already)")
        parser.add_argument("--non_linguistic_symbols", type=str_or_none, help="non_linguistic_symbols file path")
        parser.add_argument("--cleaner", type=str_or_none, choices=[None, "tacotron", "jaconv", "vietnamese"],
                            default=None, help="Apply text cleaning")
        parser.add_argument("--g2p", type=str_or_none, default=None, help="Specify g2p method if --token_type=phn")
        for cc in cls.class_choices_list:
            cc.add_arguments(g)
        # (--model_conf comes from the `model` class choice; its defaults are the model's)
        parser.set_defaults(model_conf=_default_kwargs(ESPnetLanguageModel))

    @classmethod
    def build_collate_fn(cls, args, train: bool):
        return CommonCollateFn(int_pad_value=0)  # lm.py:139

    @classmethod
    def build_preprocess_fn(cls, args, train: bool):
        if not getattr(args, "use_preprocessor", False):
            return None
        for key in ("non_linguistic_symbols", "cleaner", "g2p"):
            if getattr(args, key, None) is not None:
                raise NotImplementedError(f"--{key}: the build's text path tokenises with the token list only")
        if args.token_type == "bpe" and getattr(args, "bpemodel", None) is not None:
            raise NotImplementedError("--token_type bpe with --bpemodel: no sentencepiece tokenizer here "
                                      "(tokenise beforehand and give a text_int file, or use char / word)")
        token_list = args.token_list
        if isinstance(token_list, str):
            with open(token_list, encoding="utf-8") as f:
                token_list = [line.rstrip() for line in f]
        return _LMTextPreprocessor(args.token_type, token_list)

    @classmethod
    def required_data_names(cls, train: bool = True, inference: bool = False) -> Tuple[str, ...]:
        return ("text",)

    @classmethod
    def optional_data_names(cls, train: bool = True, inference: bool = False) -> Tuple[str, ...]:
        return ()

    @classmethod
    def check_single_gpu(cls, args):
        """The LM task runs on one GPU: anything that asks for more is refused by its name."""
        bad = []
        if getattr(args, "ngpu", 1) > 1:
            bad.append(f"--ngpu {args.ngpu}")
        for key, default in (("multiprocessing_distributed", False), ("dist_world_size", None), ("dist_rank", None),
                             ("dist_launcher", None), ("local_rank", None)):
            if getattr(args, key, default) not in (default, None):
                bad.append(f"--{key} {getattr(args, key)}")
        if bad:
            raise NotImplementedError("the LM task trains on a single GPU: " + ", ".join(bad) + " is not supported")

    @classmethod
    def main(cls, args: argparse.Namespace = None, cmd=None):
        if args is None:
            args = cls.get_parser().parse_args(cmd)
        cls.normalize_args(args)
        if not args.print_config:
            cls.check_single_gpu(args)
        super().main(args=args)

    @classmethod
    def main_worker(cls, args: argparse.Namespace):
        cls.check_single_gpu(args)
        super().main_worker(args)

    @classmethod
    def build_model(cls, args) -> ESPnetLanguageModel:
        return build_model(args)


def _get(args, key, default=None):
    if isinstance(args, dict):
        return args.get(key, default)
    return getattr(args, key, default)


def build_model(args) -> ESPnetLanguageModel:
    """lm.py:175-207 (nothing is appended to the token list: the last id is <sos/eos>)."""
    token_list = _get(args, "token_list")
    if isinstance(token_list, str):
        with open(token_list, encoding="utf-8") as f:
            token_list = [line.rstrip() for line in f]
        if isinstance(args, argparse.Namespace):
            args.token_list = list(token_list)  # keep the saved config portable
    elif isinstance(token_list, (tuple, list)):
        token_list = list(token_list)
    else:
        raise RuntimeError("token_list must be str or dict")
    vocab_size = len(token_list)
    logging.info(f"Vocabulary size: {vocab_size}")
    if _get(args, "init") is not None:
        raise NotImplementedError(f"--init {_get(args, 'init')}: the recipes use torch's default initialisation")
    lm_class = lm_choices.get_class(_get(args, "lm", "seq_rnn") or "seq_rnn")
    lm = lm_class(vocab_size=vocab_size, **(_get(args, "lm_conf") or {}))
    model_class = model_choices.get_class(_get(args, "model", "lm") or "lm")
    return model_class(lm=lm, vocab_size=vocab_size, **(_get(args, "model_conf") or {}))
