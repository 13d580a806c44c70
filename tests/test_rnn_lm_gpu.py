"""SequentialRNNLM (espnet2/lm/seq_rnn_lm.py) on the HIP path against the reference run on the
same weights (tests/golden/rnn_lm_*.npz, tests/capture_rnn_lm_goldens.py): forward logits and
final state, a chain of batch_score steps with the beam's reordering of states, score, and
BeamSearch / BatchBeamSearch with RNN-LM shallow fusion (decoder + CTC prefix + LM + length
bonus) reproducing the reference's n-best."""
import numpy as np
import pytest
import torch

from rnn_lm_goldens import SIZED, SMALL, load_lm, restate_forward

pytestmark = pytest.mark.gpu

TOL = dict(atol=1e-4, rtol=1e-4)  # what tests/test_lm_gpu.py holds TransformerLM to


def _lm(name, amp=False):
    from espnet_amd.lm import SequentialRNNLM
    cfg, d, lm = load_lm(name, SequentialRNNLM)
    lm.prepare("cuda", amp=amp)
    lm.eval()
    return cfg, d, lm


def _stacked(states):
    return (torch.stack([h for h, _ in states], dim=1).cpu().numpy(),
            torch.stack([c for _, c in states], dim=1).cpu().numpy())


@pytest.mark.parametrize("name", SMALL + SIZED)
def test_forward_logits_and_state_match_reference(name):
    cfg, d, lm = _lm(name)
    logits, (h, c) = lm(torch.from_numpy(d["in.ids"]), None)
    np.testing.assert_allclose(logits.cpu().numpy(), d["out.logits"], **TOL)
    np.testing.assert_allclose(h.cpu().numpy(), d["out.h"], **TOL)
    np.testing.assert_allclose(c.cpu().numpy(), d["out.c"], **TOL)
    # continuing from a returned hidden state == one pass over the whole sequence
    T = d["in.ids"].shape[1]
    if T > 1:
        ids = torch.from_numpy(d["in.ids"])
        _, hid = lm(ids[:, :T // 2], None)
        l2, (h2, c2) = lm(ids[:, T // 2:], hid)
        np.testing.assert_allclose(l2.cpu().numpy(), d["out.logits"][:, T // 2:], **TOL)
        np.testing.assert_allclose(h2.cpu().numpy(), d["out.h"], **TOL)


@pytest.mark.parametrize("name", SIZED)
def test_sized_batch_score_from_given_states(name):
    """n = 17 (two row tiles) from states that are not views of an earlier step (stack fallback)."""
    cfg, d, lm = _lm(name)
    bh, bc = torch.from_numpy(d["in.bs_h"]).cuda(), torch.from_numpy(d["in.bs_c"]).cuda()
    n = bh.shape[1]
    logp, st = lm.batch_score(torch.from_numpy(d["in.ys"]).cuda(), [(bh[:, i], bc[:, i]) for i in range(n)], None)
    np.testing.assert_allclose(logp.cpu().numpy(), d["out.bs_logp"], **TOL)
    h, c = _stacked(st)
    np.testing.assert_allclose(h, d["out.bs_h"], **TOL)
    np.testing.assert_allclose(c, d["out.bs_c"], **TOL)


@pytest.mark.parametrize("name", SMALL)
def test_batch_score_chain_matches_reference(name):
    cfg, d, lm = _lm(name)
    ys = torch.from_numpy(d["in.ys"]).cuda()
    states = [None] * ys.shape[0]
    k = 0
    while f"chain.{k}.logp" in d:
        logp, states = lm.batch_score(ys[:, :k + 1], states, None)
        assert logp.shape == d[f"chain.{k}.logp"].shape and len(states) == ys.shape[0]
        assert all(h.shape == (lm.nlayers, lm.nhid) and c.shape == h.shape for h, c in states)
        np.testing.assert_allclose(logp.cpu().numpy(), d[f"chain.{k}.logp"], **TOL)
        h, c = _stacked(states)
        np.testing.assert_allclose(h, d[f"chain.{k}.h"], **TOL)
        np.testing.assert_allclose(c, d[f"chain.{k}.c"], **TOL)
        k += 1
    assert k >= 2


def test_batch_score_reordered_repeated_and_mixed_states():
    """What a beam does with the states: a permutation, one parent twice, the old states again
    afterwards (they are immutable), and states of mixed origin (the stack fallback)."""
    cfg, d, lm = _lm("rnn_lm_tiny")
    ys = torch.from_numpy(d["in.ys"]).cuda()
    n = ys.shape[0]
    _, s0 = lm.batch_score(ys[:, :1], [None] * n, None)
    _, s1 = lm.batch_score(ys[:, :2], s0, None)
    ref2 = d["chain.2.logp"]
    keep = [(h.clone(), c.clone()) for h, c in s1]
    base, st2 = lm.batch_score(ys[:, :3], s1, None)
    np.testing.assert_allclose(base.cpu().numpy(), ref2, **TOL)
    h2, c2 = _stacked(st2)

    perm = [2, 0, 3, 1]
    got, stp = lm.batch_score(ys[perm][:, :3], [s1[i] for i in perm], None)
    assert torch.equal(got, base[perm])  # the same rows through the in-kernel gather: bit-identical
    hp, cp = _stacked(stp)
    assert np.array_equal(hp, h2[:, perm]) and np.array_equal(cp, c2[:, perm])

    twice = [1, 1, 3, 1]  # one parent several times, with different next tokens
    yt = ys[twice][:, :3].clone()
    yt[1, 2], yt[3, 2] = ys[0, 2], ys[2, 2]
    got, _ = lm.batch_score(yt, [s1[i] for i in twice], None)
    assert torch.equal(got[0], base[1]) and torch.equal(got[2], base[3])
    one, _ = lm.batch_score(yt[1:2], [s1[1]], None)
    torch.testing.assert_close(got[1], one[0], atol=1e-6, rtol=1e-6)

    # later steps have run; the old states are unchanged and give the same result again
    for (h, c), (hk, ck) in zip(s1, keep):
        assert torch.equal(h, hk) and torch.equal(c, ck)
    again, _ = lm.batch_score(ys[:, :3], s1, None)
    assert torch.equal(again, base)

    # mixed origin: None (zeros), a view of an earlier step, a clone, a CPU tensor pair
    mixed = [None, s1[1], (s1[2][0].clone(), s1[2][1].clone()), (s1[3][0].cpu(), s1[3][1].cpu())]
    got, _ = lm.batch_score(ys[:, :3], mixed, None)
    np.testing.assert_allclose(got[1:].cpu().numpy(), ref2[1:], **TOL)
    torch.testing.assert_close(got[1:], base[1:], atol=1e-6, rtol=1e-6)
    zero, _ = lm.batch_score(ys[:1, 2:3], [None], None)  # row 0 restarted from the zero state
    torch.testing.assert_close(got[0], zero[0], atol=1e-6, rtol=1e-6)
    zs, _ = lm.batch_score(ys[:1, 2:3], [tuple(t.cuda() for t in lm.zero_state())], None)
    torch.testing.assert_close(zs[0], zero[0], atol=1e-6, rtol=1e-6)


def test_score_equals_batch_score_row_and_takes_its_own_state_back():
    cfg, d, lm = _lm("rnn_lm_tiny")
    ys = torch.from_numpy(d["in.ys"]).cuda()
    state = None
    for k in range(3):
        logp, state = lm.score(ys[2, :k + 1], state, None)
        assert logp.shape == (lm.vocab_size,)
        np.testing.assert_allclose(logp.cpu().numpy(), d[f"chain.{k}.logp"][2], **TOL)
    # the (L, 1, H) state layout the reference's own score returns
    ref_style = (state[0].unsqueeze(1).clone(), state[1].unsqueeze(1).clone())
    a, _ = lm.score(ys[2, :4], state, None)
    b, _ = lm.score(ys[2, :4], ref_style, None)
    np.testing.assert_allclose(a.cpu().numpy(), d["chain.3.logp"][2], **TOL)
    torch.testing.assert_close(a, b, atol=1e-6, rtol=1e-6)


def test_training_mode_raises_and_reload_repacks():
    cfg, d, lm = _lm("rnn_lm_tiny")
    ids = torch.from_numpy(d["in.ids"])
    lm.train()
    with pytest.raises(NotImplementedError, match="no training"):
        lm(ids, None)
    lm.eval()
    sd = {k: v.clone() for k, v in lm.state_dict().items()}
    lm.load_state_dict({k: torch.zeros_like(v) for k, v in sd.items()})
    flat, _ = lm(ids, None)
    assert not flat.any()  # the post hook repacked the zero weights
    lm.load_state_dict(sd)
    logits, _ = lm(ids, None)
    np.testing.assert_allclose(logits.cpu().numpy(), d["out.logits"], **TOL)


@pytest.mark.parametrize("batch", [False, True])
def test_beam_search_with_rnn_lm_fusion_matches_reference(batch):
    from espnet_amd.asr.inference import attention_beam_search
    from test_inference_gpu import _setup
    m, _, inp = _setup()
    cfg, d, lm = _lm("rnn_lm_tiny")
    meta, tag = (cfg["nbest_batch"], "b") if batch else (cfg["nbest"], "c")
    for ci, (beam, lb, mlr, cw, lw) in enumerate(cfg["cases"]):
        got = attention_beam_search(m, inp["speech"], inp["speech_lengths"], beam, lb, mlr, ctc_weight=cw, lm=lm,
                                    lm_weight=lw, batch=batch)
        for u, nbest in enumerate(got):
            n = [e["n"] for e in meta if e["case"] == ci and e["utt"] == u][0]
            assert len(nbest) == n, (ci, u)
            for r, h in enumerate(nbest):
                k = f"{tag}{ci}.u{u}.h{r}"
                assert h.yseq.tolist() == d[k + ".yseq"].tolist(), (ci, u, r)
                np.testing.assert_allclose(float(h.score), float(d[k + ".score"]), rtol=1e-4, atol=1e-3)
                np.testing.assert_allclose(float(h.scores["lm"]), float(d[k + ".lm"]), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("lm_conf", [dict(nlayers=4, unit=2048), dict(unit=650, nlayers=2)], ids=["4x2048", "2x650"])
def test_recipe_sized_lm_loads_and_decodes(lm_conf):
    """A librispeech-sized lm_conf and the 2 x 650 default: a reference-layout state_dict loads
    into a prepared model and attention_beam_search decodes with it, batch or not."""
    from espnet_amd.asr.inference import attention_beam_search
    from espnet_amd.lm import build_lm
    from test_inference_gpu import _setup
    m, _, inp = _setup()
    V = m.vocab_size
    torch.manual_seed(1)
    with torch.device("cuda"):
        lm = build_lm(None, lm_conf, V)
        donor = build_lm("seq_rnn", lm_conf, V)
    assert list(donor.state_dict()) == ["encoder.weight"] + [
        f"rnn.{p}_l{k}" for k in range(lm_conf["nlayers"]) for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
    ] + ["decoder.weight", "decoder.bias"]
    lm.prepare("cuda")
    lm.eval()
    lm.load_state_dict(donor.state_dict())
    ids = torch.randint(1, V, (2, 3))
    want, _ = restate_forward({k: v.cpu() for k, v in donor.state_dict().items()}, ids, dtype=torch.float32)
    logits, _ = lm(ids, None)
    torch.testing.assert_close(logits.cpu(), want, **TOL)
    # (random weights leave near-ties, so the two search classes, whose arithmetic differs in
    # rounding, are not compared with each other: each must decode, and reproducibly)
    for batch in (False, True):
        runs = [attention_beam_search(m, inp["speech"][:1], inp["speech_lengths"][:1], 3, 0.0, 0.0, ctc_weight=0.3,
                                      lm=lm, lm_weight=0.3, batch=batch)[0] for _ in range(2)]
        assert len(runs[0]) >= 1
        for a, b in zip(*runs):
            assert a.yseq.tolist() == b.yseq.tolist() and float(a.score) == float(b.score)
            assert int(a.yseq[0]) == m.sos and int(a.yseq[-1]) == m.eos and len(a.yseq) > 2
            assert np.isfinite(float(a.score)) and float(a.scores["lm"]) < 0


@pytest.mark.parametrize("name", ["rnn_lm_tiny", "rnn_lm_650"])
def test_rnn_lm_bf16_close(name):
    """amp=True (bf16 packs): relative L2 error of the logits against the fixture within the
    project's AMP rule, max(2 x the error of a CPU restatement that rounds the weights and the
    product operands to bf16 as the HIP path does, 2e-2)."""
    cfg, d, lm = _lm(name, amp=True)
    ids = torch.from_numpy(d["in.ids"])
    ref = torch.from_numpy(d["out.logits"]).double()
    logits, _ = lm(ids, None)
    e = float((logits.cpu().double() - ref).norm() / ref.norm())
    sd = {k: v.detach().cpu() for k, v in lm.state_dict().items()}
    cpu, _ = restate_forward(sd, ids, bf16=True)
    e_cpu = float((cpu - ref).norm() / ref.norm())
    print(f"{name} bf16: rel L2 of logits {e:.3e} (CPU bf16 restatement {e_cpu:.3e})")
    assert e <= max(2 * e_cpu, 2e-2), (e, e_cpu)
