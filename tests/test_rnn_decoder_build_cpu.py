"""decoder: rnn on the CPU: the RNNDecoder's constructor, state_dict layout and seeded
initialisation against the reference's (tests/capture_rnn_decoder_goldens.py fixtures), every
refusal by the option's name, and ASRTask building a model from a config with `decoder: rnn`."""
import os

import numpy as np
import pytest
import torch
import yaml

import rnn_decoder_goldens as G
from goldens import GOLDEN, load, section

KEYS = ["embed.weight", "decoder.{l}", "output.weight", "output.bias", "att_list.0.mlp_enc.weight",
        "att_list.0.mlp_enc.bias", "att_list.0.mlp_dec.weight", "att_list.0.mlp_att.weight",
        "att_list.0.loc_conv.weight", "att_list.0.gvec.weight", "att_list.0.gvec.bias"]


def _dec(**kw):
    from espnet_amd.asr.decoder.rnn_decoder import RNNDecoder
    return RNNDecoder(vocab_size=11, encoder_output_size=16, **kw)


def _expected_keys(layers):
    out = []
    for k in KEYS:
        if k == "decoder.{l}":
            out += [f"decoder.{l}.{n}" for l in range(layers) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        else:
            out.append(k)
    return out


@pytest.mark.parametrize("name", G.STORED)
def test_state_dict_and_seeded_init_equal_the_reference(name):
    from espnet_amd.asr.decoder.rnn_decoder import RNNDecoder
    cfg, d = load(name)
    torch.manual_seed(cfg["seed"])
    dec = RNNDecoder(**G.decoder_kwargs(cfg))
    sd, w = dec.state_dict(), section(d, "w")
    assert list(sd) == list(w) == _expected_keys(cfg["layers"])
    for k, v in sd.items():
        assert v.shape == w[k].shape, k
        assert np.array_equal(v.numpy(), w[k]), f"{k}: seeded initialisation differs from the reference's"


def test_wide_fixture_regenerates_from_its_seed():
    from espnet_amd.asr.decoder.rnn_decoder import RNNDecoder
    cfg, d, dec, inp = G.build("rnn_dec_wide", RNNDecoder)  # (checks wsum.* of every parameter)
    assert inp["hs_pad"].shape == (2, 130, 256) and dec.dlayers == 1


def test_defaults_are_the_references():
    d = _dec()
    assert (d.dlayers, d.dunits, d.dropout, d.sos, d.eos, d.odim) == (1, 320, 0.0, 10, 10, 11)
    att = d.att_list[0]
    assert (att.att_dim, att.aconv_chans, att.aconv_filts) == (320, 10, 100)
    assert d.att_list[0].loc_conv.weight.shape == (10, 1, 1, 201)
    # aheads / awin / han_* are accepted and unused for `location`
    _dec(att_conf=dict(atype="location", aheads=8, awin=3, han_mode=False, han_type=None, han_heads=2, han_dim=7,
                       han_conv_chans=-1, han_conv_filts=9, han_win=2, adim=12, aconv_chans=2, aconv_filts=4))


@pytest.mark.parametrize("kw,word", [
    (dict(rnn_type="gru"), "rnn_type"),
    (dict(sampling_probability=0.1), "sampling_probability"),
    (dict(context_residual=True), "context_residual"),
    (dict(replace_sos=True), "replace_sos"),
    (dict(num_encs=2), "num_encs"),
    (dict(att_conf=dict(atype="dot")), "atype"),
    (dict(att_conf=dict(atype="coverage")), "atype"),
    (dict(att_conf=dict(atype="multi_head_loc")), "atype"),
    (dict(att_conf=dict(num_att=2)), "num_att"),
])
def test_refusals_name_the_option(kw, word):
    with pytest.raises(NotImplementedError, match=word):
        _dec(**kw)


def test_unknown_rnn_type_is_the_references_value_error():
    with pytest.raises(ValueError, match="Not supported: rnn_type=rnn"):
        _dec(rnn_type="rnn")


def test_forward_before_binding_raises():
    with pytest.raises(RuntimeError, match="bind"):
        _dec()(torch.zeros(1, 2, 16), torch.tensor([2]), torch.zeros(1, 1, dtype=torch.long), torch.tensor([1]))


def test_layer_handles_hold_the_modules_parameters():
    """The LSTMLayer handles of both recurrent models, built over a CPU arena: each holds the very
    Parameters of its module (identity, so the kernels' gradients land in the arena's views), and
    its I / H are the layer's (the decoder's layer 0 reads [eys | context])."""
    from espnet_amd.arena import ParamArena
    from espnet_amd.asr.decoder.rnn_decoder import RNNDecoder
    from espnet_amd.layers.common import Bound
    from espnet_amd.lm import SequentialRNNLM
    names = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
    lm = SequentialRNNLM(11, unit=5, nhid=3, nlayers=2)
    lm._bind_train(Bound(ParamArena(lm, "cpu"), "", torch.float32))
    dec = RNNDecoder(11, 6, num_layers=2, hidden_size=3)
    dec.bind(ParamArena(dec, "cpu"), "", torch.float32)
    assert len(lm._layers) == 2 and len(dec._layers) == 2
    for k, (lay, dlay) in enumerate(zip(lm._layers, dec._layers)):
        for n in names:
            assert getattr(lay, n) is getattr(lm.rnn, f"{n}_l{k}"), (k, n)
            assert getattr(dlay, n) is getattr(dec.decoder[k], n), (k, n)
            assert getattr(lay, n).grad is not None and getattr(dlay, n).grad is not None
        assert lay.w_ih.data_ptr() == lay.weight_ih.data_ptr() and dlay.w_ih.data_ptr() == dlay.weight_ih.data_ptr()
    assert [(lay.I, lay.H) for lay in lm._layers] == [(5, 3), (3, 3)]
    assert [(lay.I, lay.H) for lay in dec._layers] == [(9, 3), (3, 3)]
    assert lm._embed.weight is lm.encoder.weight and lm._head.weight is lm.decoder.weight
    assert dec._embed.weight is dec.embed.weight and dec._head.bias is dec.output.bias


def test_task_builds_the_recipe_decoder():
    """ASRTask + `decoder: rnn` with the decoder_conf of egs2/aishell/asr1/conf/train_asr_rnn.yaml
    over the tiny_hybrid encoder: the reference's parameter count."""
    from espnet_amd.asr.decoder.rnn_decoder import RNNDecoder
    from espnet_amd.tasks.asr import ASRTask, decoder_choices
    assert decoder_choices.get_class("rnn") is RNNDecoder
    cfg, d = load("rnn_dec_tiny")
    h = cfg["hyb"]
    with open(os.path.join(GOLDEN, "train_asr_rnn_aishell.yaml")) as f:
        recipe = yaml.safe_load(f)
    assert recipe["decoder"] == "rnn"
    V = h["vocab_size"]
    tok = ["<blank>", "<unk>"] + [f"t{i}" for i in range(V - 3)] + ["<sos/eos>"]
    m = ASRTask.build_model(dict(token_list=tok, input_size=h["input_size"], encoder="conformer",
                                 encoder_conf=h["encoder_conf"], decoder=recipe["decoder"],
                                 decoder_conf=recipe["decoder_conf"], model_conf=h["model_conf"]))
    assert isinstance(m.decoder, RNNDecoder) and m.decoder.dlayers == 2 and m.decoder.dunits == 1024
    assert sum(p.numel() for p in m.parameters()) == int(d["hyb.nparams_recipe"])


def test_print_config_accepts_decoder_rnn(capsys):
    from espnet_amd.bin.asr_train import main
    with pytest.raises(SystemExit) as e:
        main(["--print_config", "--decoder", "rnn"])
    assert e.value.code in (0, None)
    assert "decoder_conf" in capsys.readouterr().out


def test_hybrid_fixture_model_regenerates_from_its_seed():
    import test_rnn_decoder_gpu as T
    cfg, d, m = T.hybrid_model()
    assert type(m.decoder).__name__ == "RNNDecoder"
