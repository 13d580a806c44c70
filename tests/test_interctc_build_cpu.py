"""Intermediate CTC / self-conditioned CTC on the CPU (no GPU needed): the models of the
reference fixtures build with the reference's state_dict layout, the two librispeech_100 recipe
configurations parse through the task and build with the reference's parameter count, and the
constructor checks hold."""
import os

import numpy as np
import pytest
import torch

from goldens import GOLDEN, load as load_one, section
from interctc_goldens import FIXTURES, load
from test_model_build import build


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_model_builds_with_reference_layout(name):
    cfg, d = load(name)
    torch.manual_seed(0)
    m = build(cfg)
    ref = section(d, "w")
    sd = m.state_dict()
    assert list(sd.keys()) == list(ref.keys())
    cond = cfg["encoder_conf"]["interctc_use_conditioning"]
    keys = list(sd.keys())
    assert ("encoder.conditioning_layer.weight" in keys) == cond
    if cond:  # the reference's position: right behind the encoder's own parameters
        i = keys.index("encoder.after_norm.bias")
        assert keys[i + 1:i + 3] == ["encoder.conditioning_layer.weight", "encoder.conditioning_layer.bias"]
        V, dm = cfg["vocab_size"], cfg["encoder_conf"]["output_size"]
        assert tuple(sd["encoder.conditioning_layer.weight"].shape) == (dm, V)
    for k, v in ref.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
        if "norm" in k or "running" in k or "num_batches" in k:
            continue  # the fixtures perturb norm parameters / BN statistics on purpose
        torch.testing.assert_close(sd[k].float(), torch.from_numpy(v).float(), rtol=0, atol=0,
                                   msg=f"init differs for {k}")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in ref.items()}, strict=True)
    assert sum(p.numel() for p in m.parameters()) == int(d["out.num_params"])
    assert m.encoder.interctc_layer_idx == cfg["encoder_conf"]["interctc_layer_idx"]
    assert m.interctc_weight == cfg["model_conf"]["interctc_weight"]


@pytest.mark.parametrize("recipe", ["train_conformer_interctc", "train_conformer_scctc"])
def test_recipe_config_builds(recipe):
    """The reference's recipe YAML parses unchanged and builds (input_size 80, 5000 tokens) a
    model with the reference's parameter count."""
    from espnet_amd.tasks.asr import ASRTask as T
    _, counts = load_one("interctc_recipes")
    args = T.get_parser().parse_args(["--config", os.path.join(GOLDEN, recipe + ".yaml"), "--input_size", "80",
                                      "--output_dir", "x", "--token_list", "t"])
    T.normalize_args(args)
    assert args.encoder_conf["interctc_layer_idx"] == [6, 12] and args.encoder_conf["num_blocks"] == 18
    assert args.model_conf == {"ctc_weight": 1.0, "interctc_weight": 0.66, "lsm_weight": 0.1,
                               "length_normalized_loss": False}
    assert args.accum_grad == 16 and args.best_model_criterion == [["valid", "cer_ctc", "min"]]
    args.token_list = ["<blank>", "<unk>"] + [f"t{i}" for i in range(4997)] + ["<sos/eos>"]
    torch.manual_seed(0)
    m = T.build_model(args)
    cond = recipe.endswith("scctc")
    assert bool(m.encoder.interctc_use_conditioning) == cond and (m.encoder.conditioning_layer is not None) == cond
    assert m.decoder is None and m.specaug is not None and m.encoder.interctc_layer_idx == [6, 12]
    assert sum(p.numel() for p in m.parameters()) == int(counts["nparams." + recipe])
    assert len(m.state_dict()) == int(counts["nkeys." + recipe])


def _cfg(**enc):
    cfg, _ = load("interctc_sc_hybrid")
    cfg = dict(cfg)
    cfg["encoder_conf"] = dict(cfg["encoder_conf"], **enc)
    return cfg


@pytest.mark.parametrize("idx", [[0, 2], [4], [1, 7]])
def test_tap_index_out_of_range_asserts(idx):
    """conformer_encoder.py:292-293: 0 < min(idx) and max(idx) < num_blocks (4 here)."""
    with pytest.raises(AssertionError):
        build(_cfg(interctc_layer_idx=idx))


def test_refusals_with_taps():
    from espnet_amd.asr.ctc import CTC
    from espnet_amd.asr.espnet_model import ESPnetASRModel
    from espnet_amd.asr.encoder.conformer_encoder import ConformerEncoder
    cfg = _cfg()
    V = cfg["vocab_size"]
    tok = ["<blank>", "<unk>"] + [f"t{i}" for i in range(V - 3)] + ["<sos/eos>"]

    def model(ctc_drop=0.0, **kw):
        enc = ConformerEncoder(input_size=80, **cfg["encoder_conf"])
        ctc = CTC(odim=V, encoder_output_size=64, dropout_rate=ctc_drop)
        conf = dict(ctc_weight=1.0, interctc_weight=0.5)
        conf.update(kw)
        return ESPnetASRModel(vocab_size=V, token_list=tok, encoder=enc, decoder=None, ctc=ctc, **conf)

    model()  # the configuration itself is accepted
    with pytest.raises(NotImplementedError, match="aux_ctc"):
        model(aux_ctc={"1": "text_aux"})
    with pytest.raises(NotImplementedError, match="dropout"):
        model(ctc_drop=0.1)
    with pytest.raises(NotImplementedError, match="lang token"):
        model(lang_token_id=3)
    with pytest.raises(NotImplementedError, match="transducer"):
        model(joint_network=torch.nn.Linear(2, 2))


def test_options_that_stay_refused():
    with pytest.raises(NotImplementedError):  # TransformerEncoder taps
        build(dict(_cfg(), encoder="transformer",
                   encoder_conf=dict(output_size=64, attention_heads=4, linear_units=128, num_blocks=4,
                                     input_layer="conv2d", normalize_before=True, interctc_layer_idx=[1, 3])))
    with pytest.raises(NotImplementedError):
        build(_cfg(stochastic_depth_rate=0.1))
    with pytest.raises(NotImplementedError):
        build(_cfg(layer_drop_rate=0.1))
