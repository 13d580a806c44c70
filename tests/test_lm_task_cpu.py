"""LMTask on the CPU: the parser reads the recipes' train_lm YAMLs, build_model builds them with
the reference's parameter counts, the sentence pair of ESPnetLanguageModel.nll equals the
reference's construction (espnet2/lm/espnet_model.py:38-51, restated here with its loop), the
`text` loader with word / char preprocessing, and the refusals name their option."""
import argparse
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from goldens import GOLDEN, load
from rnn_lm_goldens import RECIPES


def _tokens(tmp_path, V):
    p = tmp_path / "tokens.txt"
    p.write_text("\n".join(["<blank>", "<unk>"] + [f"w{i}" for i in range(V - 3)] + ["<sos/eos>"]) + "\n")
    return str(p)


def _args(tmp_path, key, V, extra=()):
    from espnet_amd.tasks.lm import LMTask
    cmd = ["--config", os.path.join(GOLDEN, f"rnn_lm_{key}.yaml"), "--token_list", _tokens(tmp_path, V),
           "--output_dir", str(tmp_path / "exp"), *extra]
    return LMTask.normalize_args(LMTask.get_parser().parse_args(cmd))


@pytest.mark.parametrize("key", RECIPES)
def test_parser_loads_recipe_and_build_model_has_the_reference_parameter_count(tmp_path, key):
    from espnet_amd.lm import ESPnetLanguageModel, SequentialRNNLM
    from espnet_amd.tasks.lm import LMTask
    cfg, d = load("rnn_lm_recipes")
    V = cfg["vocab_size"]
    args = _args(tmp_path, key, V)
    assert args.lm == "seq_rnn" and args.model == "lm" and args.model_conf == {"ignore_id": 0}
    assert args.batch_type in ("folded", "numel", "sorted", "unsorted", "length")
    with torch.device("meta"):
        model = LMTask.build_model(args)
    assert isinstance(model, ESPnetLanguageModel) and isinstance(model.lm, SequentialRNNLM)
    assert len(args.token_list) == V  # the path was replaced by the list, nothing appended
    assert model.sos == model.eos == V - 1 and model.lm.vocab_size == V
    assert sum(p.numel() for p in model.parameters()) == int(d["nparams." + key])
    assert len(model.state_dict()) == int(d["nkeys." + key])
    assert all(k.startswith("lm.") for k in model.state_dict())


def test_task_interface():
    from espnet_amd.tasks.lm import LMTask, lm_choices, model_choices
    from espnet_amd.train.collate_fn import CommonCollateFn
    assert LMTask.required_data_names() == ("text",) and LMTask.optional_data_names() == ()
    assert set(lm_choices.classes) == {"seq_rnn", "transformer"} and lm_choices.default == "seq_rnn"
    assert set(model_choices.classes) == {"lm"}
    assert LMTask.trainer.capture_steps is False
    collate = LMTask.build_collate_fn(argparse.Namespace(), True)
    assert isinstance(collate, CommonCollateFn)
    ids, b = collate([("a", {"text": np.array([3, 4, 5])}), ("b", {"text": np.array([6])})])
    assert b["text"].tolist() == [[3, 4, 5], [6, 0, 0]] and b["text_lengths"].tolist() == [3, 1]
    cfg = LMTask.get_default_config()
    assert cfg["lm"] == "seq_rnn" and cfg["lm_conf"]["unit"] == 650 and cfg["lm_conf"]["nlayers"] == 2


def _reference_xt(text, text_lengths, V, ignore_id=0, max_length=None):
    """espnet2/lm/espnet_model.py:38-51."""
    sos = eos = V - 1
    text = text[:, :text_lengths.max()] if max_length is None else text[:, :max_length]
    x = F.pad(text, [1, 0], "constant", eos)
    t = F.pad(text, [0, 1], "constant", ignore_id)
    for i, n in enumerate(text_lengths):
        t[i, n] = sos
    return x, t, text_lengths + 1


def test_sentence_pair_matches_the_reference_construction():
    from espnet_amd.lm import ESPnetLanguageModel, SequentialRNNLM
    V = 13
    model = ESPnetLanguageModel(SequentialRNNLM(vocab_size=V, unit=4, nlayers=1), V)
    gen = torch.Generator().manual_seed(0)
    lens = torch.tensor([5, 1, 3, 4])
    text = torch.zeros(4, 7, dtype=torch.int64)  # over-padded: two columns past the longest sentence
    for i, n in enumerate(lens.tolist()):
        text[i, :n] = torch.randint(0, V - 1, (n,), generator=gen)  # id 0 may occur inside a sentence
    for max_length in (None, 5, 7):
        got = model.make_xt(text.clone(), lens, max_length)
        want = _reference_xt(text.clone(), lens, V, max_length=max_length)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and torch.equal(a, b), max_length
    assert got[0].shape == (4, 8) and int(got[0][0, 0]) == V - 1 and int(got[1][1, 1]) == V - 1


def test_batchify_nll_splits_and_pads_to_the_overall_longest():
    from espnet_amd.lm import ESPnetLanguageModel, SequentialRNNLM
    V = 9
    calls = []

    class Probe(ESPnetLanguageModel):
        def nll(self, text, text_lengths, max_length=None):
            x, t, xl = self.make_xt(text, text_lengths, max_length)
            calls.append((text.shape[0], max_length, tuple(x.shape)))
            return torch.ones(x.shape) * (torch.arange(x.shape[1])[None] < xl[:, None]), xl

    model = Probe(SequentialRNNLM(vocab_size=V, unit=4, nlayers=1), V)
    lens = torch.tensor([2, 6, 1, 3, 4])
    text = torch.ones(5, 6, dtype=torch.int64)
    nll, xl = model.batchify_nll(text, lens, batch_size=2)
    assert calls == [(2, 6, (2, 7)), (2, 6, (2, 7)), (1, 6, (1, 7))]
    assert nll.shape == (5, 7) and xl.tolist() == [3, 7, 2, 4, 5] and nll.sum(1).tolist() == [3, 7, 2, 4, 5]
    calls.clear()
    nll, xl = model.batchify_nll(text, lens, batch_size=100)
    assert calls == [(5, None, (5, 7))] and nll.shape == (5, 7)
    assert model.collect_feats(text, lens) == {}


def test_text_loader_with_word_and_char_preprocessing(tmp_path):
    from espnet_amd.fileio.datasets import ESPnetDataset
    from espnet_amd.tasks.lm import LMTask
    (tmp_path / "lm_train.txt").write_text("utt1 the cat  sat\nutt2 dog\nutt3\n")
    words = ["<blank>", "<unk>", "the", "cat", "sat", "<sos/eos>"]
    chars = ["<blank>", "<unk>", "<space>", "a", "c", "t", "<sos/eos>"]
    for token_type, tokens, want in (("word", words, {"utt1": [2, 3, 4], "utt2": [1], "utt3": []}),
                                     ("char", chars, {"utt1": [5, 1, 1, 2, 4, 3, 5, 2, 2, 1, 3, 5], "utt2": [1, 1, 1]})):
        args = argparse.Namespace(use_preprocessor=True, token_type=token_type, token_list=tokens, bpemodel=None,
                                  non_linguistic_symbols=None, cleaner=None, g2p=None)
        ds = ESPnetDataset([(str(tmp_path / "lm_train.txt"), "text", "text")],
                           preprocess=LMTask.build_preprocess_fn(args, True))
        assert ds.has_name("text") and list(ds) == ["utt1", "utt2", "utt3"]
        for uid, ids in want.items():
            u, data = ds[uid]
            assert u == uid and data["text"].dtype == np.int64 and data["text"].tolist() == ids, (token_type, uid)
    # integer text passes through whatever the token type
    args = argparse.Namespace(use_preprocessor=True, token_type="bpe", token_list=words, bpemodel=None)
    pre = LMTask.build_preprocess_fn(args, True)
    assert pre("u", {"text": np.array([4, 2])})["text"].tolist() == [4, 2]
    with pytest.raises(RuntimeError, match="<unk>"):
        a = argparse.Namespace(use_preprocessor=True, token_type="word", token_list=["a", "b"], bpemodel=None)
        LMTask.build_preprocess_fn(a, True)("u", {"text": "a c"})


def test_refusals_name_their_option(tmp_path):
    from espnet_amd.lm import ESPnetLanguageModel, TransformerLM
    from espnet_amd.tasks.lm import LMTask
    key, V = RECIPES[0], 50
    base = ["--config", os.path.join(GOLDEN, f"rnn_lm_{key}.yaml"), "--token_list", _tokens(tmp_path, V),
            "--output_dir", str(tmp_path / "exp")]
    with pytest.raises(NotImplementedError, match="--ngpu 2"):
        LMTask.main(cmd=base + ["--ngpu", "2"])
    with pytest.raises(NotImplementedError, match="--multiprocessing_distributed"):
        LMTask.main(cmd=base + ["--ngpu", "1", "--multiprocessing_distributed", "true"])
    with pytest.raises(NotImplementedError, match="--dist_world_size 2"):
        LMTask.main(cmd=base + ["--ngpu", "1", "--dist_world_size", "2"])
    with pytest.raises(NotImplementedError, match="--optim sgd"):
        LMTask.build_optimizers(_args(tmp_path, key, V, ["--optim", "sgd"]), None)
    tlm = TransformerLM(vocab_size=V, embed_unit=8, att_unit=8, unit=16, layer=1)
    with pytest.raises(NotImplementedError, match="no training"):
        ESPnetLanguageModel(tlm, V).prepare("cuda")
    args = argparse.Namespace(use_preprocessor=True, token_type="bpe", token_list=["<unk>", "a"], bpemodel=None)
    with pytest.raises(NotImplementedError, match="token_type=bpe"):
        LMTask.build_preprocess_fn(args, True)("u", {"text": "a a"})
    args.bpemodel = "bpe.model"
    with pytest.raises(NotImplementedError, match="--token_type bpe"):
        LMTask.build_preprocess_fn(args, True)
    for rnn_type, tie in (("gru", False), ("lstm", True)):
        with pytest.raises(NotImplementedError):
            LMTask.build_model(dict(token_list=["a"] * V, lm="seq_rnn", lm_conf=dict(rnn_type=rnn_type, tie_weights=tie,
                                                                                 unit=8)))
