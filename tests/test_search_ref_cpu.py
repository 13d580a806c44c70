"""Pins tests/search_ref.py, the references the beam-search kernel tests compare against: the
prefix-score restatement against oracle.asr_oracle.OracleCTCPrefixScore (f32, pinned to the
reference beam-search goldens) — bit-equal in float32, within the f32 floor in float64 — on the
T=37 inputs of test_ctc_gpu.py's kernel test; its frame range, window and <eos> / blank rules;
the pre-beam against torch.topk; the selection against a scalar restatement."""
import numpy as np
import pytest
import torch

import search_ref as R
from oracle.asr_oracle import OracleCTCPrefixScore

F32, F64 = np.float32, np.float64
T, V, EOS = 37, 11, 10
PREFIXES = ([EOS], [EOS, 3], [EOS, 3, 5], [EOS, 3, 5, 5])
CS = np.array([0, 3, 5, 7, EOS], dtype=np.int64)


def _logp():
    g = torch.Generator().manual_seed(5)
    return torch.log_softmax(torch.randn(T, V, generator=g) * 2, -1).numpy()


def _oracle_chain(impl, y):
    r_prev = impl.initial_state()
    for k in range(1, len(y)):
        _, st = impl(np.array(y[:k]), np.array([y[k]]), r_prev)
        r_prev = st[0]
    return r_prev


@pytest.mark.parametrize("y", PREFIXES, ids=lambda y: f"ol{len(y) - 1}")
def test_prefix_score_f32_is_bit_equal_to_oracle(y):
    logp = _logp()
    impl = OracleCTCPrefixScore(logp, 0, EOS)
    r_prev = _oracle_chain(impl, y)
    assert np.array_equal(r_prev, R.chain_ref(logp, 0, EOS, y[1:], F32))
    psi_o, r_o = impl(np.array(y), CS, r_prev)
    psi, r = R.prefix_score_ref(logp, r_prev, len(y) - 1, y[-1], CS, 0, EOS, F32)
    assert psi.dtype == F32 and r.dtype == F32 and r.shape == (len(CS), T, 2)
    assert np.array_equal(psi, psi_o)
    assert np.array_equal(r, r_o)


@pytest.mark.parametrize("y", PREFIXES, ids=lambda y: f"ol{len(y) - 1}")
def test_prefix_score_f64_within_f32_floor_of_oracle(y):
    """Every frame of the f32 recursion rounds a logaddexp and a sum, each to 2^-24 of a value
    the metric divides by |v| + 1, and at worst the roundings of all T frames add up: the oracle
    is within 4 * T * 2^-24 = 8.8e-6 of float64 (measured: 2.8e-7)."""
    logp = _logp()
    impl = OracleCTCPrefixScore(logp, 0, EOS)
    r_prev = _oracle_chain(impl, y)
    psi_o, r_o = impl(np.array(y), CS, r_prev)
    psi, r = R.prefix_score_ref(logp, r_prev, len(y) - 1, y[-1], CS, 0, EOS, F64)
    assert psi.dtype == F64 and r.dtype == F64
    err = max(R.rel_err(psi_o, psi), R.rel_err(r_o, r))
    print(f"ol={len(y) - 1}: oracle (f32) vs float64 {err:.3g}")
    assert err <= 4 * T * 2.0 ** -24, err
    assert np.array_equal(impl.initial_state(), R.initial_state_ref(logp, 0, F32))
    assert R.rel_err(impl.initial_state(), R.initial_state_ref(logp, 0, F64)) <= T * 2.0 ** -24


@pytest.mark.parametrize("window", [(1, T), (5, 20), (30, 33), (T - 1, T), (3, T + 9)])
@pytest.mark.parametrize("y", PREFIXES[:3], ids=lambda y: f"ol{len(y) - 1}")
def test_prefix_score_window_is_bit_equal_to_oracle(y, window):
    logp = _logp()
    impl = OracleCTCPrefixScore(logp, 0, EOS)
    r_prev = _oracle_chain(impl, y)
    psi_o, r_o = impl(np.array(y), CS, r_prev, window=window)
    psi, r = R.prefix_score_ref(logp, r_prev, len(y) - 1, y[-1], CS, 0, EOS, F32, *window)
    assert np.array_equal(psi, psi_o)
    assert np.array_equal(r, r_o)


def test_prefix_score_frame_range_and_dead_rows():
    """start / end as the kernels compute them, rows outside them logzero but for the empty
    prefix's r[0], and a prefix as long as the utterance: nothing live but the <eos> psi."""
    assert R.frame_range(37, 0) == (1, 37) and R.frame_range(37, 4) == (4, 37)
    assert R.frame_range(37, 0, 5, 40) == (5, 37) and R.frame_range(37, 2, 60, 70) == (37, 37)
    assert R.frame_range(2, 5) == (2, 2) and R.frame_range(1, 0) == (1, 1)
    logp = _logp()
    r0 = R.initial_state_ref(logp, 0, F64)
    lz = R.LOGZERO
    psi, r = R.prefix_score_ref(logp, r0, 0, EOS, CS, 0, EOS, F64, 5, 20)
    assert np.array_equal(r[:, 0, 0], logp[0, CS].astype(F64)) and np.all(r[:, 0, 1] == lz)
    assert np.all(r[:, 1:5] == lz) and np.all(r[:, 20:] == lz) and np.all(r[:, 5:20, 0] > lz)
    assert psi[0] == lz and psi[-1] == np.logaddexp(r0[-1, 0], r0[-1, 1])
    psi, r = R.prefix_score_ref(logp[:2], r0[:2], 5, 3, CS, 0, EOS, F64)
    assert np.all(r == lz) and np.all(psi[:-1] == lz) and psi[-1] == np.logaddexp(r0[1, 0], r0[1, 1])
    ext = R.extend_state_ref(logp, 0, r0[:12], 30, F64)
    np.testing.assert_allclose(ext, r0[:30], rtol=1e-14)
    ext0 = R.extend_state_ref(logp, 0, r0[:0], 30, F64)
    assert np.all(ext0[:, 0] == lz) and ext0[0, 1] == lz
    np.testing.assert_allclose(ext0[1:, 1], lz + np.cumsum(logp[1:30, 0].astype(F64)), rtol=1e-14)
    impl = OracleCTCPrefixScore(logp[:30], 0, EOS)
    assert np.array_equal(impl.extend_state(r0[:12].astype(F32)),
                          R.extend_state_ref(logp, 0, r0[:12].astype(F32), 30, F32))


@pytest.mark.parametrize("V_,P", [(17, 15), (50, 30), (5000, 64)])
@pytest.mark.parametrize("use_lb", [0, 1])
def test_prebeam_ref_matches_topk(V_, P, use_lb):
    g = torch.Generator().manual_seed(V_ + P)
    logp = torch.log_softmax(torch.randn(3, V_, generator=g) * 3, -1)
    W = R.weighted_ref(logp.numpy(), 0.7, 0.3, use_lb)
    # tie-free where it matters: the P + 1 largest values of every row are distinct
    assert all(len(np.unique(np.sort(W[h])[-P - 1:])) == P + 1 for h in range(3))
    Wt = torch.tensor(0.7, dtype=torch.float32) * logp
    if use_lb:
        Wt = Wt + torch.tensor(0.3, dtype=torch.float32)
    assert np.array_equal(Wt.numpy(), W)
    got = R.prebeam_ref(logp.numpy(), 0.7, 0.3, use_lb, P, V_ - 1)
    assert got.dtype == np.int32 and got.shape == (3, P + 1)
    assert np.array_equal(got[:, :P], torch.topk(Wt, P, dim=1).indices.numpy())
    assert np.all(got[:, P] == V_ - 1)


def test_prebeam_ref_breaks_ties_toward_the_lower_token():
    logp = np.array([[1.0, 2.0, 2.0, 0.5, 2.0, 1.0, -np.inf, 1.0]], dtype=F32)
    assert R.prebeam_ref(logp, 0.5, 0.0, 0, 6, 7).tolist() == [[1, 2, 4, 0, 5, 7, 7]]


def _select_scalar(logp, cand, psi, prefix, score, w_dec, w_lb, use_lb, w_ctc, V_, beam):
    """select_ref's rule one slot at a time, with Python's sort."""
    n, P1 = cand.shape
    items = []
    for h in range(n):
        for k in range(P1):
            j = int(cand[h, k])
            if k == P1 - 1 and j in cand[h, :P1 - 1].tolist():
                continue
            W = F32(w_dec) * logp[h, j]
            if use_lb:
                W = W + F32(w_lb)
            W = (W + F32(w_ctc) * (psi[h, k] - prefix[h])) + score[h]
            items.append((-float(W), h * V_ + j, h, j, k))
    items.sort()
    return [(h, j, k, -w) for w, _, h, j, k in items[:beam]]


@pytest.mark.parametrize("weights", [(0.5, 1.0, 0.25), (0.7, 0.1, 0.3)], ids=["exact", "rounded"])
@pytest.mark.parametrize("use_lb", [0, 1])
def test_select_ref_matches_scalar_restatement(weights, use_lb):
    w_dec, w_lb, w_ctc = weights
    g = np.random.default_rng(3)
    n, P, V_, beam, T_ = 6, 7, 40, 20, 7
    logp = R.quantised((n, V_), g)
    logp[4], logp[0, V_ - 1] = logp[1], 50.0  # a cross-hypothesis tie; <eos> among row 0's P tokens
    cand = R.prebeam_ref(logp, w_dec, w_lb, use_lb, P, V_ - 1)
    assert V_ - 1 in cand[0, :P]
    psi, prefix, score = R.quantised((n, P + 1), g), R.quantised(n, g), R.quantised(n, g)
    psi[4], prefix[4], score[4] = psi[1], prefix[1], score[1]
    out = R.select_ref(logp, cand, psi, prefix, score, w_dec, w_lb, use_lb, w_ctc, V_, beam, T_)
    want = _select_scalar(logp, cand, psi, prefix, score, w_dec, w_lb, use_lb, w_ctc, V_, beam)
    assert [tuple(r[:3]) for r in out["rec_i"].tolist()] == [w[:3] for w in want]
    assert np.all(out["rec_i"][:, 3] == 0)
    assert out["rec_f"][:, 0].tolist() == [w[3] for w in want]
    assert len(np.unique(out["rec_f"][:, 0])) < beam  # the ties are there
    assert (0, V_ - 1, P) not in [w[:3] for w in want]
    for b, (h, j, k, _) in enumerate(want):
        assert out["rec_f"][b, 1] == logp[h, j] and out["rec_f"][b, 3] == psi[h, k]
        assert out["rec_f"][b, 2] == psi[h, k] - prefix[h]
        assert out["rptr_next"][b] == (h * (P + 1) + k) * T_ * 2 * 4
    assert np.array_equal(out["last_next"], out["rec_i"][:, 1])
    assert np.array_equal(out["prefix_next"], out["rec_f"][:, 3])
    assert np.array_equal(out["score_next"], out["rec_f"][:, 0])


def test_select_ref_marks_missing_candidates():
    logp = np.array([[0.0, -1.0, -2.0, -3.0, 5.0]], dtype=F32)
    cand = R.prebeam_ref(logp, 1.0, 0.0, 0, 3, 4)
    assert cand.tolist() == [[4, 0, 1, 4]]
    out = R.select_ref(logp, cand, np.zeros((1, 4), F32), np.zeros(1, F32), np.zeros(1, F32), 1.0, 0.0, 0, 0.5, 5, 4, 3)
    assert out["rec_i"][:3, :3].tolist() == [[0, 4, 0], [0, 0, 1], [0, 1, 2]]
    assert out["rec_i"][:, 3].tolist() == [0, 0, 0, 1] and out["rec_f"][3, 0] == -np.inf
