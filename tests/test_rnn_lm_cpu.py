"""SequentialRNNLM without a GPU: the reference's state_dict layout and refusals, build_lm on
the recipes' lm / lm_conf blocks, and the packed weight layout of ea_lstm_step against a numpy
restatement that follows it."""
import numpy as np
import pytest
import torch

from goldens import load, section
from rnn_lm_goldens import RECIPES, SIZED, SMALL, load_lm, recipe, restate_forward


def test_state_dict_layout_equals_reference():
    from espnet_amd.lm import SequentialRNNLM
    for name in SMALL:
        cfg, d, lm = load_lm(name, SequentialRNNLM)
        ref = section(d, "w")
        sd = lm.state_dict()
        assert list(sd) == list(ref)
        for k, v in ref.items():
            assert tuple(sd[k].shape) == v.shape, k
    assert list(sd)[:1] == ["encoder.weight"] and list(sd)[-2:] == ["decoder.weight", "decoder.bias"]
    assert [k for k in sd if k.startswith("rnn.")][:4] == [f"rnn.{p}_l0" for p in
                                                            ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


@pytest.mark.parametrize("name", SIZED)
def test_sized_weights_regenerate(name):
    from espnet_amd.lm import SequentialRNNLM
    load_lm(name, SequentialRNNLM)  # asserts the layout and every per-tensor sum


def test_restatement_matches_reference_outputs():
    """The float64 CPU restatement the GPU tests use as their bf16 yardstick reproduces the
    fixture (the reference's f32 run) to f32 rounding."""
    cfg, d = load("rnn_lm_nhid")
    sd = {k: torch.from_numpy(v) for k, v in section(d, "w").items()}
    lg, (h, c) = restate_forward(sd, torch.from_numpy(d["in.ids"]))
    np.testing.assert_allclose(lg.numpy(), d["out.logits"], atol=1e-5, rtol=1e-5)
    np.testing.assert_allclose(h.numpy(), d["out.h"], atol=1e-5, rtol=1e-5)
    np.testing.assert_allclose(c.numpy(), d["out.c"], atol=1e-5, rtol=1e-5)


def test_refusals_name_the_option():
    from espnet_amd.lm import SequentialRNNLM
    for rt in ("gru", "rnn_tanh", "rnn_relu"):
        with pytest.raises(NotImplementedError, match="rnn_type"):
            SequentialRNNLM(30, unit=8, rnn_type=rt)
    with pytest.raises(NotImplementedError, match="tie_weights"):
        SequentialRNNLM(30, unit=8, tie_weights=True)
    with pytest.raises(ValueError, match="invalid option"):
        SequentialRNNLM(30, unit=8, rnn_type="rnn")
    lm = SequentialRNNLM(30, unit=8)
    with pytest.raises(RuntimeError, match="prepare"):
        lm(torch.zeros(1, 2, dtype=torch.long), None)
    with pytest.raises(RuntimeError, match="GPU only"):
        lm.prepare("cpu")


def test_zero_state():
    from espnet_amd.lm import SequentialRNNLM
    h, c = SequentialRNNLM(30, unit=8, nhid=12, nlayers=3).zero_state()
    for t in (h, c):
        assert t.shape == (3, 12) and t.dtype == torch.float32 and not t.any()


def test_build_lm_on_recipe_confs():
    from espnet_amd.lm import SequentialRNNLM, TransformerLM, build_lm
    cfg, d = load("rnn_lm_recipes")
    assert tuple(cfg["recipes"]) == RECIPES
    for key in RECIPES:
        y = recipe(key)
        with torch.device("meta"):
            lm = build_lm(y.get("lm"), y["lm_conf"], cfg["vocab_size"])
        assert type(lm) is SequentialRNNLM
        assert sum(p.numel() for p in lm.parameters()) == int(d["nparams." + key]), key
        assert len(lm.state_dict()) == int(d["nkeys." + key]), key
    assert recipe("librispeech_train_lm_adam")["lm_conf"] == dict(nlayers=4, unit=2048)
    assert type(build_lm("transformer", dict(att_unit=64, embed_unit=16, unit=32, layer=1), 20)) is TransformerLM
    with pytest.raises(ValueError, match="lm must be one of"):
        build_lm("rwkv", {}, 20)


def _packed_gemv(P, I, H, SL, x, h):
    """W_ih x + W_hh h read out of the flat packed operand, following include/espnet_amd.h:
    element (tile t, slice s, row r, j) at ((t * nks + s) * 16 + r) * SL + j."""
    Ip, Hp = (I + 31) // 32 * 32, (H + 31) // 32 * 32
    nks, nt = (Ip + Hp) // SL, (H + 3) // 4
    P = np.asarray(P, dtype=np.float64)
    assert P.size == nt * nks * 16 * SL
    xa = np.zeros(Ip + Hp)
    xa[:I], xa[Ip:Ip + H] = x, h
    out = np.zeros(4 * H)
    for t in range(nt):
        for r in range(16):
            u, gate = divmod(r, 4)
            acc = 0.0
            for s in range(nks):
                o = ((t * nks + s) * 16 + r) * SL
                acc += float(P[o:o + SL] @ xa[s * SL:(s + 1) * SL])
            if 4 * t + u < H:
                out[gate * H + 4 * t + u] = acc
            else:
                assert acc == 0.0
    return out


@pytest.mark.parametrize("I,H", [(1, 1), (5, 3), (26, 26), (24, 40), (650, 650)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pack_layout_against_numpy(I, H, dtype):
    from espnet_amd.lm.lstm_pack import pack_lstm_bias, pack_lstm_weights
    g = torch.Generator().manual_seed(I * 1000 + H)
    w_ih = torch.randint(-3, 4, (4 * H, I), generator=g).float()  # integers: exact in bf16 and in any sum order
    w_hh = torch.randint(-3, 4, (4 * H, H), generator=g).float()
    x = torch.randint(-3, 4, (I,), generator=g).float()
    h = torch.randint(-3, 4, (H,), generator=g).float()
    P = pack_lstm_weights(w_ih, w_hh, dtype)
    assert P.dtype == dtype and P.dim() == 1
    SL = 32 if dtype == torch.bfloat16 else 16
    got = torch.from_numpy(_packed_gemv(P.float().numpy(), I, H, SL, x.numpy(), h.numpy())).float()
    assert torch.equal(got, w_ih @ x + w_hh @ h)
    # every entry that holds no weight is zero: the all-ones pack marks the data positions
    ones = pack_lstm_weights(torch.ones(4 * H, I), torch.ones(4 * H, H), dtype).float()
    assert int(ones.sum()) == 4 * H * (I + H) and set(ones.unique().tolist()) <= {0.0, 1.0}
    Q = pack_lstm_weights(w_ih + 10, w_hh + 10, dtype).float()  # no zero among the data
    assert bool((Q[ones == 0] == 0).all()) and bool((Q[ones == 1] != 0).all())
    b_ih, b_hh = torch.arange(4 * H).float(), 100.0 * torch.arange(4 * H).float()
    pb = pack_lstm_bias(b_ih, b_hh)
    assert torch.equal(pb.view(H, 4).t().reshape(-1), b_ih + b_hh)


@pytest.mark.parametrize("I", [1, 40])
@pytest.mark.parametrize("H", [3, 26, 64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_step_pack_holds_the_hh_pack_and_refresh_leaves_nothing_stale(H, I, dtype):
    """The K slices [Ip / SL, (Ip + Hp) / SL) of every tile of the decoding step's pack are the
    training forward's pack bit for bit, and an HHPacks refreshed with other weights equals a
    fresh pack of those weights in both operands."""
    from espnet_amd.lm.lstm_pack import HHPacks, pack_lstm_hh, pack_lstm_hh_t, pack_lstm_weights
    g = torch.Generator().manual_seed(100 * H + I)
    w_ih, w_hh, w2 = torch.randn(4 * H, I, generator=g), torch.randn(4 * H, H, generator=g), torch.randn(4 * H, H, generator=g)
    SL = 32 if dtype == torch.bfloat16 else 16
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    Ip, Hp, nt = (I + 31) // 32 * 32, (H + 31) // 32 * 32, (H + 3) // 4
    full = pack_lstm_weights(w_ih, w_hh, dtype).view(nt, (Ip + Hp) // SL, 16 * SL)
    hh = pack_lstm_hh(w_hh, dtype).view(nt, Hp // SL, 16 * SL)
    assert torch.equal(full[:, Ip // SL:].view(bits), hh.view(bits))
    packs = HHPacks(w_hh, dtype).refresh(w_hh)
    assert torch.equal(packs.fwd.view(bits), hh.reshape(-1).view(bits))
    packs.refresh(w2)
    assert torch.equal(packs.fwd.view(bits), pack_lstm_hh(w2, dtype).view(bits))
    assert torch.equal(packs.bwd.view(bits), pack_lstm_hh_t(w2, dtype).view(bits))
