"""The beam-search selection kernels of csrc/beam.hip through the C ABI against the np.float32
references of tests/search_ref.py: integer outputs exactly, float outputs bit for bit.

  prebeam<8|16|32>  prebeam_kernel, 8 / 16 / 32 tokens per lane (V <= 8192 / 16384 / 32768), with
                    scores quantised to multiples of 0.25 (exact ties), a padded row stride, P up
                    to PB_PMAX = 64, and rows whose best tokens sit in one wave's slice, in the
                    last wave's ragged tail, or next to a block of -inf
  select            select_kernel from 4 to 4,096 candidate slots (its strided loops run once up to
                    64 slots), ties within and across hypotheses, the duplicate <eos> rule, the
                    `none` record, and the argument checks of both entry points
  chained step      prebeam -> ea_ctc_prefix_score_dev -> select twice at n = 20, V = 5000,
                    T = 300, beam = 20: step two's parents are what step one's select wrote

Chained step, measured on an MI355X (f32 floor, bound max(1e-6, 4 x floor), kernel worst of psi, r):
  step 1  floor 1.28e-6  bound 5.11e-6  kernel 1.28e-6
  step 2  floor 1.17e-6  bound 4.68e-6  kernel 1.17e-6

The "rounded" weights (0.7, 0.1, 0.3) are what found select's scores an ulp off the reference:
the compiler fused w_dec*logp + w_lb and W + w_ctc*inc into multiply-adds (fixed in beam.hip);
with the "exact" weights (0.5, 1.0, 0.25) every product is exact and the two agree either way.
"""
import numpy as np
import pytest
import torch

import search_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENT_I = -7
PB_V = [("prebeam<8>", v) for v in (2, 17, 50, 1024, 1025, 5000, 8192)] + \
       [("prebeam<16>", 8193), ("prebeam<16>", 16384), ("prebeam<32>", 16385), ("prebeam<32>", 32768)]
PB_P = [1, 15, 30, 64]
PB_CASES = [(t, v, p) for t, v in PB_V for p in PB_P if p < v]  # P < V is the contract
WEIGHTS = {"exact": (0.5, 1.0, 0.25), "rounded": (0.7, 0.1, 0.3)}  # w_dec, w_lb, w_ctc


def prebeam_template(V):
    """ea_beam_prebeam's dispatch: 16 waves split V, each lane holds ceil(ceil(V / 16) / 64) tokens."""
    per = ((V + 15) // 16 + 63) // 64
    return "prebeam<8>" if per <= 8 else "prebeam<16>" if per <= 16 else "prebeam<32>"


_ROWS = {}


def prebeam_rows(V):
    """(3, V + 3) quantised scores, shared and read-only; the padding columns would win if read."""
    if V not in _ROWS:
        x = np.full((3, V + 3), 1e30, dtype=F32)
        x[:, :V] = R.quantised((3, V), np.random.default_rng(V))
        _ROWS[V] = x
    return _ROWS[V]


def run_prebeam(x, V, n, P, eos, w_dec, w_lb, use_lb, xd=None):
    """cand (4, P + 1) from a buffer prefilled with a sentinel: rows >= n must stay untouched."""
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    xd = torch.from_numpy(x).cuda() if xd is None else xd
    cand = torch.full((4, P + 1), SENT_I, dtype=torch.int32, device="cuda")
    lib.ea_beam_prebeam(n, V, xd.data_ptr(), x.shape[1], w_dec, w_lb, use_lb, P, eos, cand.data_ptr(), ops.stream())
    torch.cuda.synchronize()
    out = cand.cpu().numpy()
    assert np.all(out[n:] == SENT_I), "slots of hypotheses >= n written"
    return out[:n]


@pytest.mark.parametrize("tmpl,V,P", PB_CASES, ids=[f"{t}-V{v}-P{p}" for t, v, p in PB_CASES])
def test_prebeam_matches_reference(tmpl, V, P):
    assert prebeam_template(V) == tmpl
    x = prebeam_rows(V)
    xd = torch.from_numpy(x).cuda()
    eos = V - 1
    w_dec, w_lb, _ = WEIGHTS["rounded"]
    for n in (1, 3):
        for use_lb in (0, 1):
            want = R.prebeam_ref(x[:n, :V], w_dec, w_lb, use_lb, P, eos)
            got = run_prebeam(x, V, n, P, eos, w_dec, w_lb, use_lb, xd)
            assert np.array_equal(got, want), (n, use_lb)
    W = R.weighted_ref(x[:, :V], w_dec, w_lb, 1)
    if V >= 1024:  # the ties are there: the P-th and (P+1)-th values coincide in some row
        assert any(np.sort(W[h])[-P] == np.sort(W[h])[-P - 1] for h in range(3)) or P == 1


@pytest.mark.parametrize("P", [15, 64])
def test_prebeam_special_rows(P):
    """V = 5000: 16 waves of 313 tokens (the last one 305), five tokens per lane.  Row 0: an
    ascending ramp inside wave 3's slice, so all P winners come from one wave's list, one per
    lane.  Row 1: the same slice ascending in lane-major order, so the winners are a few lanes'
    whole lists.  Row 2: the best tokens at the end of the last wave's ragged tail.  Row 3: -inf
    over waves 2..4 but a few entries, so those slices hold fewer than P finite values."""
    V, span = 5000, 313
    g = np.random.default_rng(P)
    x = np.full((4, V + 3), 1e30, dtype=F32)
    x[:, :V] = R.quantised((4, V), g)
    x[0, 3 * span:4 * span] = 100 + 0.25 * np.arange(span)
    k = np.arange(span)
    x[1, 3 * span:4 * span] = 100 + 0.25 * ((k % 64) * 5 + k // 64)
    x[2, V - 40:V] += 100
    x[3, 2 * span - 10:5 * span + 7] = -np.inf
    x[3, [2 * span, 3 * span + 5, 3 * span + 69, 4 * span + 100]] = 50.0
    w_dec, w_lb, _ = WEIGHTS["rounded"]
    for lo in (0, 1):  # rows 0..2, then 1..3: three rows a launch
        rows = np.ascontiguousarray(x[lo:lo + 3])
        want = R.prebeam_ref(rows[:, :V], w_dec, w_lb, 1, P, 7)
        got = run_prebeam(rows, V, 3, P, 7, w_dec, w_lb, 1)
        assert np.array_equal(got, want), lo
    want = R.prebeam_ref(x[:, :V], w_dec, w_lb, 1, P, 7)
    assert np.all((want[0, :P] >= 3 * span) & (want[0, :P] < 4 * span)) and len(set((want[0, :P] - 3 * span) % 64)) == P
    assert len(set((want[1, :P] - 3 * span) % 64)) <= P // 4 + 1
    assert np.all(want[2, :min(P, 40)] >= V - 40)
    assert want[3, :4].tolist() == [2 * span, 3 * span + 5, 3 * span + 69, 4 * span + 100]


def test_prebeam_rounds_product_and_sum_separately():
    """Two neighbouring f32 log-probs a < b whose products with w_dec round to one f32, so
    W = w_dec*logp + w_lb ties and the lower token comes first, while a fused multiply-add
    (one rounding, of a sum in a finer binade) would order b's token ahead."""
    w_dec, w_lb = F32(0.7), F32(0.1)
    fused = lambda v: F32(F64(w_dec) * F64(v) + F64(w_lb))
    a = F32(-0.2)
    for _ in range(64):
        b = np.nextafter(a, F32(0))
        if w_dec * a == w_dec * b and fused(a) != fused(b):
            break
        a = b
    assert w_dec * a + w_lb == w_dec * b + w_lb and fused(b) > fused(a)
    V = 50
    x = np.full((3, V + 3), 1e30, dtype=F32)
    x[:, :V] = -10
    x[:, 3], x[:, 7] = a, b
    assert R.prebeam_ref(x[:, :V], 0.7, 0.1, 1, 2, V - 1).tolist() == [[3, 7, V - 1]] * 3
    assert run_prebeam(x, V, 3, 2, V - 1, 0.7, 0.1, 1).tolist() == [[3, 7, V - 1]] * 3


@pytest.mark.parametrize("n,V,ld,P", [(1, 50, 53, 50), (1, 50, 53, 51), (1, 5000, 5003, 65), (1, 32769, 32772, 15),
                                      (1, 50, 49, 15)], ids=["P=V", "P>V", "P>64", "V>32768", "ld<V"])
def test_prebeam_refuses_out_of_contract(n, V, ld, P):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import HipError, lib
    xd = torch.zeros(max(ld, V) + 8, device="cuda")
    cand = torch.full((P + 1,), SENT_I, dtype=torch.int32, device="cuda")
    with pytest.raises(HipError, match="bad argument"):  # the binding raises on a non-zero return
        lib.ea_beam_prebeam(n, V, xd.data_ptr(), ld, 0.7, 0.1, 1, P, 0, cand.data_ptr(), ops.stream())
    torch.cuda.synchronize()
    assert bool((cand == SENT_I).all())  # nothing was launched


# ------------------------------------------------------------------------------ select
def select_buffers(beam):
    """select's outputs, one record longer than the beam, prefilled with sentinels."""
    dev = "cuda"
    return dict(rec_i=torch.full((beam + 1, 4), SENT_I, dtype=torch.int32, device=dev),
                rec_f=torch.full((beam + 1, 4), -7.25, device=dev),
                last_next=torch.full((beam + 1,), SENT_I, dtype=torch.int32, device=dev),
                rptr_next=torch.full((beam + 1,), SENT_I, dtype=torch.int64, device=dev),
                prefix_next=torch.full((beam + 1,), -7.25, device=dev),
                score_next=torch.full((beam + 1,), -7.25, device=dev))


def run_select(n, V, P, beam, T, logp_d, ld, cand_d, psi_d, prefix_d, score_d, w, use_lb, r_new_d, out=None):
    """One ea_beam_select launch (a refusal raises HipError); the records on the host, rptr_next
    as the byte offset from r_new, and under "device" the buffers the kernel wrote."""
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    out = select_buffers(beam) if out is None else out
    lib.ea_beam_select(n, V, P, beam, T, logp_d.data_ptr(), ld, cand_d.data_ptr(), psi_d.data_ptr(),
                       prefix_d.data_ptr(), score_d.data_ptr(), w[0], w[1], use_lb, w[2], r_new_d.data_ptr(),
                       out["rec_i"].data_ptr(), out["rec_f"].data_ptr(), out["last_next"].data_ptr(),
                       out["rptr_next"].data_ptr(), out["prefix_next"].data_ptr(),
                       out["score_next"].data_ptr(), ops.stream())
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    for k, v in host.items():  # one record past the beam: untouched
        assert np.all(v[beam] == (SENT_I if v.dtype.kind == "i" else F32(-7.25))), k
    host = {k: v[:beam] for k, v in host.items()}
    host["rptr_next"] = host["rptr_next"] - r_new_d.data_ptr()
    host["device"] = out  # the next step's inputs
    return host


def assert_select_equal(got, want, valid=None):
    """Every field of every record exactly (f32 fields bit for bit); `valid` limits the records
    whose fields are specified."""
    sel = slice(None) if valid is None else slice(0, valid)
    for k in ("rec_i", "rec_f", "last_next", "rptr_next", "prefix_next", "score_next"):
        g, w = got[k][sel], want[k][sel]
        if g.dtype.kind == "f":
            assert np.array_equal(g.view(np.int32), w.astype(F32).view(np.int32)), k
        else:
            assert np.array_equal(g, w), k


SELECT = [(1, 3, 2), (10, 15, 10), (20, 30, 20), (63, 64, 60), (64, 63, 64)]


@pytest.mark.parametrize("wname", list(WEIGHTS))
@pytest.mark.parametrize("n,P,beam", SELECT, ids=[f"select-n{n}-P{p}-beam{b}-slots{n * (p + 1)}" for n, p, b in SELECT])
def test_select_matches_reference(n, P, beam, wname):
    """V = 5000, T = 7 (r_new is an address base only).  Quantised logp, psi, prefix and score:
    with the "exact" weights every sum is exact, so equal inputs tie; every third hypothesis
    repeats an earlier one's row, psi, prefix and score (hypothesis 2 the leading hypothesis 0's),
    which ties across hypotheses (flat index order) under either weight set.  <eos> is among
    hypothesis 0's P tokens."""
    V, T, ld = 5000, 7, 5003
    eos = V - 1
    w = WEIGHTS[wname]
    g = np.random.default_rng(n * 100 + P)
    x = np.full((n, ld), 1e30, dtype=F32)
    x[:, :V] = R.quantised((n, V), g)
    psi = R.quantised((n, P + 1), g) - 20
    prefix, score = R.quantised(n, g) - 15, R.quantised(n, g) - 30
    # hypothesis 0 leads, <eos> is its best token, and its duplicate <eos> slot has the best psi of
    # all: the beam would open with that slot if the duplicate rule did not fire
    x[0, eos], score[0], psi[0, P] = x[0, :V].max() + 1, score.max() + 3, 0.0
    psi[0, 0] = -5.0  # <eos> itself (column 0, the best token) is chosen
    for h in range(2, n, 3):
        x[h], psi[h], prefix[h], score[h] = x[h - 2], psi[h - 2], prefix[h - 2], score[h - 2]
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    xd = torch.from_numpy(x).cuda()
    for use_lb in (0, 1):
        cand = torch.full((n, P + 1), SENT_I, dtype=torch.int32, device="cuda")
        lib.ea_beam_prebeam(n, V, xd.data_ptr(), ld, w[0], w[1], use_lb, P, eos, cand.data_ptr(), ops.stream())
        torch.cuda.synchronize()
        cand_h = cand.cpu().numpy()
        assert np.array_equal(cand_h, R.prebeam_ref(x[:, :V], w[0], w[1], use_lb, P, eos))
        assert eos in cand_h[0, :P]
        r_new = torch.empty(n * (P + 1) * T * 2, device="cuda")
        got = run_select(n, V, P, beam, T, xd, ld, cand, torch.from_numpy(psi).cuda(),
                         torch.from_numpy(prefix).cuda(), torch.from_numpy(score).cuda(), w, use_lb, r_new)
        want = R.select_ref(x, cand_h, psi, prefix, score, w[0], w[1], use_lb, w[2], V, beam, T)
        assert np.all(want["rec_i"][:, 3] == 0)
        assert_select_equal(got, want)
        pairs = {(int(r[0]), int(r[1])) for r in got["rec_i"]}
        assert len(pairs) == beam, "winners not distinct"
        recs = [tuple(r[:3]) for r in want["rec_i"].tolist()]
        assert (0, eos, cand_h[0].tolist().index(eos)) in recs and (0, eos, P) not in recs
        if beam >= 10:  # the case has the ties it is about
            sc = want["rec_f"][:, 0]
            assert len(np.unique(sc)) < beam
            if n >= 3:
                par = want["rec_i"][:, 0]
                assert any(sc[a] == sc[a + 1] and par[a] != par[a + 1] for a in range(beam - 1))


def test_select_fewer_candidates_than_beam():
    """n = 1, P = 3 with <eos> among the P tokens: three valid slots for beam = 4.  The fourth
    record says so: rec_i[3, 3] == 1 and its score is -inf (rec_f[3, 0] and score_next[3]); its
    other fields are unspecified and not looked at."""
    V, T, P, beam, ld = 50, 7, 3, 4, 53
    eos = V - 1
    w = WEIGHTS["rounded"]
    g = np.random.default_rng(1)
    x = np.full((1, ld), 1e30, dtype=F32)
    x[:, :V] = R.quantised((1, V), g)
    x[0, eos] = x[0, :V].max() + 1
    cand_h = R.prebeam_ref(x[:, :V], w[0], w[1], 1, P, eos)
    assert cand_h[0, 0] == eos
    psi, prefix, score = R.quantised((1, P + 1), g) - 20, R.quantised(1, g), R.quantised(1, g)
    r_new = torch.empty((P + 1) * T * 2, device="cuda")
    got = run_select(1, V, P, beam, T, torch.from_numpy(x).cuda(), ld, torch.from_numpy(cand_h).cuda(),
                     torch.from_numpy(psi).cuda(), torch.from_numpy(prefix).cuda(),
                     torch.from_numpy(score).cuda(), w, 1, r_new)
    want = R.select_ref(x, cand_h, psi, prefix, score, w[0], w[1], 1, w[2], V, beam, T)
    assert want["rec_i"][:, 3].tolist() == [0, 0, 0, 1]
    assert_select_equal(got, want, valid=3)
    assert got["rec_i"][3, 3] == 1 and got["rec_f"][3, 0] == -np.inf and got["score_next"][3] == -np.inf


@pytest.mark.parametrize("n,P,beam", [(64, 64, 10), (1, 3, 5)], ids=["slots>4096", "beam>slots"])
def test_select_refuses_out_of_contract(n, P, beam):
    from espnet_amd._lib import HipError
    V, T = 100, 7
    z = lambda *s: torch.zeros(*s, device="cuda")
    cand = torch.zeros(n * (P + 1), dtype=torch.int32, device="cuda")
    out = select_buffers(beam)
    with pytest.raises(HipError, match="bad argument"):
        run_select(n, V, P, beam, T, z(n, V), V, cand, z(n * (P + 1)), z(n), z(n), WEIGHTS["rounded"], 1,
                   z(n * (P + 1) * T * 2), out=out)
    torch.cuda.synchronize()
    assert bool((out["rec_i"] == SENT_I).all()) and bool((out["last_next"] == SENT_I).all())


# ------------------------------------------------------------------------------ chained step
def test_two_chained_beam_steps():
    """prebeam -> ea_ctc_prefix_score_dev -> select, twice, at n = 20, V = 5000, T = 300, beam = 20
    (31 candidates a hypothesis: ctc_prefix_score2_kernel<64>).  Step one's parents are 20
    one-label prefixes; step two's are exactly what step one's select wrote (last_next,
    rptr_next into step one's r_new, prefix_next, score_next).  Selection is checked exactly
    given the device's own psi, so a near-tie cannot flip it; psi and r of both steps against
    the float64 restatement chained along the chosen tokens, under max(1e-6, 4 x floor) with the
    floor of the float32 restatement chained the same way."""
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    n, V, T, beam, P, blank = 20, 5000, 300, 20, 30, 0
    eos, nc, ld = V - 1, 31, 5000
    w = WEIGHTS["rounded"]
    g = np.random.default_rng(20)
    xd = torch.from_numpy(R.ctc_logits(T, V, blank, seed=5)).cuda()
    logp_d = torch.empty(T, V, device="cuda")
    r0_d = torch.empty(T, 2, device="cuda")
    assert lib.ea_ctc_prefix_init(T, V, xd.data_ptr(), V, blank, logp_d.data_ptr(), r0_d.data_ptr(), ops.stream()) == 0
    torch.cuda.synchronize()
    logp = logp_d.cpu().numpy()
    dec = [torch.log_softmax(torch.from_numpy(g.standard_normal((n, V)).astype(F32) * 3), -1).numpy() for _ in range(2)]
    # step one's parents: prefixes of one label
    labels = g.integers(1, V - 1, size=n)
    par = [R.chain_ref(logp, blank, eos, [int(y)], F64).astype(F32) for y in labels]
    par_d = [torch.from_numpy(p).cuda() for p in par]
    st = dict(last=torch.from_numpy(labels.astype(np.int32)).cuda(),
              rptr=torch.tensor([p.data_ptr() for p in par_d], dtype=torch.int64, device="cuda"),
              prefix=torch.from_numpy((R.quantised(n, g) - 12).astype(F32)).cuda(),
              score=torch.from_numpy((g.standard_normal(n) * 2 - 20).astype(F32)).cuda())
    # host mirrors of the chain: per current hypothesis (last label, r in f64 / f32 arithmetic)
    lasts, r64, r32 = labels.tolist(), par, par
    alive = []  # step one's r_new stays allocated: step two reads it through rptr_next
    for step in range(2):
        dd = torch.from_numpy(dec[step]).cuda()
        cand = torch.empty(n, nc, dtype=torch.int32, device="cuda")
        psi = torch.empty(n, nc, device="cuda")
        r_new = torch.empty(n, nc, T, 2, device="cuda")
        assert lib.ea_beam_prebeam(n, V, dd.data_ptr(), ld, w[0], w[1], 1, P, eos, cand.data_ptr(), ops.stream()) == 0
        assert lib.ea_ctc_prefix_score_dev(T, V, blank, eos, n, nc, logp_d.data_ptr(), st["rptr"].data_ptr(), step + 1,
                                           st["last"].data_ptr(), cand.data_ptr(), psi.data_ptr(), r_new.data_ptr(),
                                           ops.stream()) == 0
        got = run_select(n, V, P, beam, T, dd, ld, cand, psi, st["prefix"], st["score"], w, 1, r_new)
        cand_h, psi_h, r_h = cand.cpu().numpy(), psi.cpu().numpy(), r_new.cpu().numpy()
        assert np.array_equal(cand_h, R.prebeam_ref(dec[step], w[0], w[1], 1, P, eos))
        want = R.select_ref(dec[step], cand_h, psi_h, st["prefix"].cpu().numpy(), st["score"].cpu().numpy(),
                            w[0], w[1], 1, w[2], V, beam, T)
        assert_select_equal(got, want)
        assert len({(int(r[0]), int(r[1])) for r in got["rec_i"]}) == beam
        # the recursion of this step in f64 and f32, each from its own chain
        ref = [R.prefix_score_ref(logp, r64[h], step + 1, lasts[h], cand_h[h], blank, eos, F64) for h in range(n)]
        f32 = [R.prefix_score_ref(logp, r32[h], step + 1, lasts[h], cand_h[h], blank, eos, F32) for h in range(n)]
        psi64, rr64 = np.stack([p for p, _ in ref]), np.stack([r for _, r in ref])
        floor = max(R.rel_err(np.stack([p for p, _ in f32]), psi64), R.rel_err(np.stack([r for _, r in f32]), rr64))
        err = max(R.rel_err(psi_h, psi64), R.rel_err(r_h, rr64))
        print(f"chained step {step + 1}: floor {floor:.3g} bound {R.bound(floor):.3g} kernel {err:.3g}")
        assert err <= R.bound(floor), (step, err, floor)
        # the hand-over: the next parents are select's outputs, on the device and on the host
        hs, ks = got["rec_i"][:, 0], got["rec_i"][:, 2]
        lasts = got["rec_i"][:, 1].tolist()
        r64 = [ref[h][1][k] for h, k in zip(hs, ks)]
        r32 = [f32[h][1][k] for h, k in zip(hs, ks)]
        alive.append(r_new)
        d = got["device"]
        st = dict(last=d["last_next"][:beam], rptr=d["rptr_next"][:beam], prefix=d["prefix_next"][:beam],
                  score=d["score_next"][:beam])  # views: the very buffers select wrote
