"""Legacy relative-position attention (rel_pos_type: legacy) on the CPU, no GPU needed: the index
law and the extended table Pext reproduce the reference's legacy rel_shift exactly; the
positional table follows the reference's grow-and-stay rule; the conformer7 recipe (which leaves
rel_pos_type out) parses and builds with the reference's parameter and key counts; the fixture
models load strictly; a legacy/latest mix and zero_triu stay refused as the reference does."""
import logging
import os

import numpy as np
import pytest
import torch

from goldens import GOLDEN, load as load_one, section
from legacy_relpos_goldens import (FIXTURES, RECIPE, SHIFT_T, build_loaded, legacy_band, legacy_shift, load, pext,
                                   pext_fold)
from test_model_build import build


@pytest.mark.parametrize("T", SHIFT_T)
def test_index_law_is_the_reference_rel_shift(T):
    _, d = load_one("legacy_shift")
    x = torch.from_numpy(d[f"x.{T}"])
    y = torch.from_numpy(d[f"y.{T}"])
    assert x.dtype == torch.float64 and x.shape[-2:] == (T, T)
    assert torch.equal(legacy_shift(x), y)
    # the forced zero above the diagonal and nothing else forced
    if T >= 2:
        assert (torch.diagonal(y, 1, -2, -1) == 0).all()


@pytest.mark.parametrize("T", SHIFT_T)
def test_pext_band_form_is_the_index_law(T):
    """BD[r, k] = (q_r + v)·Pext[k] read at [i + (j > i), T-1-i+j], the form the kernels use, equals
    the index law applied to (q + v)·p^T — exactly, on small integers — and pext_fold is pext's
    adjoint."""
    g = torch.Generator().manual_seed(T)
    q = torch.randint(-4, 5, (2, 3, T, 4), generator=g).double()
    p = torch.randint(-4, 5, (T, 4), generator=g).double()
    px = pext(p)
    assert px.shape == (2 * T - 1, 4)
    assert torch.equal(px[:T], p)
    if T >= 2:
        assert (px[T] == 0).all() and torch.equal(px[T + 1:], p[:T - 2])
    assert torch.equal(legacy_band(q, px), legacy_shift(q @ p.t()))
    w = torch.randint(-4, 5, (2 * T - 1, 4), generator=g).double()
    assert float((pext(p) * w).sum()) == float((p * pext_fold(w)).sum())


def test_positional_table_grows_and_stays():
    """pos_emb = the first T rows of the reversed table, whose size is max_len until a longer
    utterance rebuilds it at that length; it then stays, so a later short utterance sees other
    rows than it would have at first."""
    from espnet_amd.layers.subsampling import LegacyRelPositionalEncoding
    cfg, d = load_one("legacy_shift")
    dm = cfg["d_model"]
    pe = LegacyRelPositionalEncoding(dm, 0.0, max_len=cfg["max_len"])
    np.testing.assert_array_equal(pe.table(10, "cpu")[:10].numpy(), d["pos.16.10"])
    pe = LegacyRelPositionalEncoding(dm, 0.0, max_len=cfg["max_len"])
    np.testing.assert_array_equal(pe.table(20, "cpu")[:20].numpy(), d["pos.16.20"])
    np.testing.assert_array_equal(pe.table(10, "cpu")[:10].numpy(), d["pos.16.20.10"])
    assert pe.table(10, "cpu").shape[0] == 20
    assert not np.array_equal(d["pos.16.20.10"], d["pos.16.10"])
    assert not list(pe.state_dict())  # the table is not a buffer


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_model_builds_with_reference_layout_and_init(name):
    from espnet_amd._lib import REL_LEGACY
    from espnet_amd.layers.subsampling import LegacyRelPositionalEncoding
    cfg, d = load(name)
    assert "rel_pos_type" not in cfg["encoder_conf"]
    torch.manual_seed(0)
    m = build(cfg)
    ref = section(d, "w")
    sd = m.state_dict()
    assert list(sd.keys()) == list(ref.keys())
    for k, v in ref.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
        if "norm" in k:
            continue  # the fixtures perturb the norm parameters on purpose
        torch.testing.assert_close(sd[k].float(), torch.from_numpy(v).float(), rtol=0, atol=0,
                                   msg=f"init differs for {k}")
    assert isinstance(m.encoder.embed.out[1], LegacyRelPositionalEncoding)
    assert all(layer.self_attn.rel_mode == REL_LEGACY for layer in m.encoder.encoders)
    _, _, m2 = build_loaded(name)  # strict=True
    assert sum(p.numel() for p in m2.parameters()) == int(d["out.num_params"])


def test_conformer7_recipe_builds(caplog):
    """train_asr_conformer7_n_fft512_hop_length256.yaml leaves rel_pos_type out: it parses
    unchanged and builds (input_size 80, 5000 tokens) the legacy encoder with the reference's
    parameter and state_dict key counts, logging the reference's deprecation warnings."""
    from espnet_amd._lib import REL_LEGACY
    from espnet_amd.asr.encoder.conformer_encoder import ConformerEncoder
    from espnet_amd.tasks.asr import ASRTask as T
    _, counts = load_one("legacy_recipes")
    args = T.get_parser().parse_args(["--config", os.path.join(GOLDEN, RECIPE + ".yaml"), "--input_size", "80",
                                      "--output_dir", "x", "--token_list", "t"])
    T.normalize_args(args)
    args.token_list = ["<blank>", "<unk>"] + [f"t{i}" for i in range(4997)] + ["<sos/eos>"]
    assert args.encoder == "conformer" and "rel_pos_type" not in args.encoder_conf
    torch.manual_seed(0)
    with caplog.at_level(logging.WARNING):
        m = T.build_model(args)
    assert isinstance(m.encoder, ConformerEncoder) and len(m.encoder.encoders) == 12
    assert m.encoder.encoders[0].self_attn.rel_mode == REL_LEGACY
    assert sum(p.numel() for p in m.parameters()) == int(counts["nparams." + RECIPE])
    assert len(m.state_dict()) == int(counts["nkeys." + RECIPE])
    assert "Using legacy_rel_pos and it will be deprecated in the future." in caplog.text
    assert "Using legacy_rel_selfattn and it will be deprecated in the future." in caplog.text


def _enc(**kw):
    from espnet_amd.asr.encoder.conformer_encoder import ConformerEncoder
    cfg, _ = load("legacy_tiny")
    return ConformerEncoder(input_size=80, **dict(cfg["encoder_conf"], num_blocks=1, **kw))


def test_legacy_latest_mix_and_zero_triu_stay_refused():
    _enc()  # the legacy pair itself is accepted
    _enc(rel_pos_type="legacy", pos_enc_layer_type="legacy_rel_pos", selfattention_layer_type="legacy_rel_selfattn")
    with pytest.raises(AssertionError):  # a latest positional encoding under a legacy attention
        _enc(rel_pos_type="latest", pos_enc_layer_type="rel_pos", selfattention_layer_type="legacy_rel_selfattn")
    with pytest.raises(AssertionError):
        _enc(rel_pos_type="latest", pos_enc_layer_type="legacy_rel_pos", selfattention_layer_type="rel_selfattn")
    with pytest.raises(AssertionError):  # rel_pos_type legacy renames only the plain names
        _enc(rel_pos_type="legacy", pos_enc_layer_type="abs_pos")
    with pytest.raises(NotImplementedError, match="zero_triu"):
        _enc(zero_triu=True)
    with pytest.raises(NotImplementedError):  # abs_pos / selfattn stay outside the implemented set
        _enc(pos_enc_layer_type="abs_pos", selfattention_layer_type="selfattn")
