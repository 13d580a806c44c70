"""The CTC prefix-score kernels of csrc/ctc_prefix.hip through the C ABI against the float64
restatement of tests/search_ref.py, on every path of the dispatch in launch_prefix2 /
prefix_score_meta:

  score2<256>   ctc_prefix_score2_kernel<256>, n_cand <= 20: one chunk (T <= 257 frames from
                start = 1) and several (the chunk loop's second iteration, the nf < CH tail, the
                write-back at 2*t0); n_cand = 20 is its largest LDS footprint, 65,696 B
  score2<64>    ctc_prefix_score2_kernel<64>, 21 <= n_cand <= 83 (66,200 B of LDS at 83)
  per-pair      ctc_prefix_score_kernel, 16-frame register chunks: through launch_prefix2
                (84 <= n_cand <= 256) and directly (n_cand > 256)

each through ea_ctc_prefix_score (per-hypothesis output lengths 1, 3, 7), ea_ctc_prefix_score_dev
(uniform 0 and 4) and ea_ctc_prefix_score_win, plus ea_ctc_prefix_init and ea_ctc_prefix_extend.

Logits are randn * 2 with the blank column raised by 2; logp is what ea_ctc_prefix_init wrote;
the parents are the float64 recursion chained along a random prefix, rounded to f32, one
allocation each; the reference reads the same f32 logp and parents as the kernel.  log_psi and
all T*2 rows of every candidate are compared: rows outside [start, end) bit for bit (logzero, the
empty prefix's r[0] = (logp[0, c], logzero)), the rest by |got - ref64| / (|ref64| + 1) against
max(1e-6, 4 x floor), floor being the same metric for the float32 np.logaddexp restatement (the
reference implementation's arithmetic) on the case's own inputs.  Guard regions around log_psi and
r_new must come back untouched, logp and the parents unchanged.

Measured on an MI355X, the case of each family where the kernel comes closest to its bound
(f32 floor of that case, its bound, the kernel's worst of log_psi and r):
  score2<256> one chunk    n_cand=5   T=37   floor 3.17e-7  bound 1.27e-6  kernel 3.17e-7
  score2<256> chunks       n_cand=20  T=258  floor 1.06e-6  bound 4.23e-6  kernel 1.06e-6
  score2<64>               n_cand=21  T=530  floor 9.43e-7  bound 3.77e-6  kernel 9.71e-7
  per-pair via prefix2     n_cand=256 T=300  floor 1.24e-6  bound 4.95e-6  kernel 1.24e-6
  per-pair direct          n_cand=257 T=300  floor 1.14e-6  bound 4.55e-6  kernel 1.14e-6
  windows (all families)                     floor 1.18e-6  bound 4.71e-6  kernel 1.18e-6
  init  logp 1.12e-7 of LOGSM_BOUND 8.1e-7;  r0 floor 2.93e-7  bound 1.17e-6  kernel 2.93e-7
  extend                                     floor 4.87e-8  bound 1e-6     kernel 4.87e-8
lae_fast (hardware exp2 / log2, no log1p) stays within 1.03x the float32 np.logaddexp floor over
530 serial frames: the worst elements are sums where one path dominates, which both round alike.
Both LDS footprints above 64 KiB (65,696 B at n_cand=20, 66,200 B at n_cand=83) launch.
"""
import numpy as np
import pytest
import torch

import search_ref as R
from test_decoder_ops_gpu import LOGSM_BOUND

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
BLANK = 0
SENT = -7.25
LZ = F32(R.LOGZERO)

ROWS = [
    ("score2<256>-one-chunk", 1, 1), ("score2<256>-one-chunk", 1, 37),
    ("score2<256>-one-chunk", 5, 2), ("score2<256>-one-chunk", 5, 37),
    ("score2<256>-chunks", 16, 256), ("score2<256>-chunks", 16, 258), ("score2<256>-chunks", 16, 530),
    ("score2<256>-chunks", 20, 257), ("score2<256>-chunks", 20, 258), ("score2<256>-chunks", 20, 530),
    ("score2<64>", 21, 64), ("score2<64>", 21, 530), ("score2<64>", 31, 65), ("score2<64>", 31, 130),
    ("score2<64>", 83, 66), ("score2<64>", 83, 530),
    ("per-pair-via-prefix2", 84, 16), ("per-pair-via-prefix2", 84, 300), ("per-pair-via-prefix2", 256, 17),
    ("per-pair-via-prefix2", 256, 18), ("per-pair-via-prefix2", 256, 300),
    ("per-pair-direct", 257, 17), ("per-pair-direct", 257, 300), ("per-pair-direct", 300, 17),
    ("per-pair-direct", 300, 300),
]
ENTRIES = {"meta-ol1.3.7": ("meta", (1, 3, 7)), "dev-ol0": ("dev", (0, 0, 0)), "dev-ol4": ("dev", (4, 4, 4))}
WIN_ROWS = [("score2<256>-chunks", 20, 530), ("score2<64>", 31, 530), ("per-pair-via-prefix2", 84, 300),
            ("per-pair-direct", 257, 300)]
WINDOWS = {"1:T": lambda T: (1, T), "5:40": lambda T: (5, 40), "60:70": lambda T: (60, 70),
           "T-1:T": lambda T: (T - 1, T), "3:T+9": lambda T: (3, T + 9)}


def family(n_cand):
    """The dispatch of launch_prefix2 / prefix_score_meta restated: dynamic LDS of the CH-frame
    instance is (3*CH + n_cand*(CH + 1) + n_cand*(2*CH + 1)) * 4 bytes, at most 64 KiB."""
    lds = lambda ch: (3 * ch + n_cand * (ch + 1) + n_cand * (2 * ch + 1)) * 4
    if n_cand > 256:
        return "per-pair-direct"
    return "score2<256>" if lds(256) <= 65536 else "score2<64>" if lds(64) <= 65536 else "per-pair-via-prefix2"


def vocab(n_cand):
    return 40 if n_cand <= 40 else 320


_LOGP = {}


def device_logp(T, V):
    """(device, host) log-posteriors of the (T, V) case, from ea_ctc_prefix_init; shared, read-only."""
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    if (T, V) not in _LOGP:
        x = torch.from_numpy(R.ctc_logits(T, V, BLANK, seed=T * 1000 + V)).cuda()
        logp = torch.empty(T, V, device="cuda")
        r0 = torch.empty(T, 2, device="cuda")
        assert lib.ea_ctc_prefix_init(T, V, x.data_ptr(), V, BLANK, logp.data_ptr(), r0.data_ptr(), ops.stream()) == 0
        torch.cuda.synchronize()
        _LOGP[(T, V)] = (logp, logp.cpu().numpy())
    return _LOGP[(T, V)]


def guarded(n, guard, dtype=torch.float32):
    """n elements with `guard` sentinel elements on each side: (whole buffer, the inner view)."""
    buf = torch.full((n + 2 * guard,), SENT, dtype=dtype, device="cuda")
    return buf, buf[guard:guard + n]


def launch(case, entry, logp_d):
    """One launch of `entry` on the case; returns (log_psi (n_hyp, n_cand), r (n_hyp, n_cand, T, 2))
    after checking the guard regions and that logp and the parents were not written."""
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    T, V, nh, nc = case.T, case.V, case.n_hyp, case.n_cand
    eos = case.eos
    parents_d = [torch.from_numpy(p).cuda() for p in reversed(case.parents)][::-1]  # one allocation each
    ptrs = torch.tensor([p.data_ptr() for p in parents_d], dtype=torch.int64, device="cuda")
    last_d = torch.from_numpy(case.lasts).cuda()
    cand_d = torch.from_numpy(case.cands.reshape(-1)).cuda()
    meta = torch.cat([torch.tensor(case.ols, dtype=torch.int32, device="cuda"), last_d, cand_d])
    psi_buf, psi = guarded(nh * nc, nc)
    r_buf, r = guarded(nh * nc * T * 2, T * 2)
    logp_before = logp_d.clone()
    if entry == "meta":
        rc = lib.ea_ctc_prefix_score(T, V, BLANK, eos, nh, nc, logp_d.data_ptr(), ptrs.data_ptr(), meta.data_ptr(),
                                     psi.data_ptr(), r.data_ptr(), ops.stream())
    elif entry == "win":
        rc = lib.ea_ctc_prefix_score_win(T, V, BLANK, eos, nh, nc, logp_d.data_ptr(), ptrs.data_ptr(),
                                         meta.data_ptr(), case.wstart, case.wend, psi.data_ptr(), r.data_ptr(),
                                         ops.stream())
    else:
        assert len(set(case.ols)) == 1
        rc = lib.ea_ctc_prefix_score_dev(T, V, BLANK, eos, nh, nc, logp_d.data_ptr(), ptrs.data_ptr(), case.ols[0],
                                         last_d.data_ptr(), cand_d.data_ptr(), psi.data_ptr(), r.data_ptr(),
                                         ops.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    psi_all, r_all = psi_buf.cpu().numpy(), r_buf.cpu().numpy()
    for name, a, g in (("log_psi", psi_all, nc), ("r_new", r_all, T * 2)):
        assert np.all(a[:g] == SENT) and np.all(a[-g:] == SENT), f"{name}: guard region written"
    assert torch.equal(logp_d, logp_before), "logp written"
    for p_d, p in zip(parents_d, case.parents):
        assert np.array_equal(p_d.cpu().numpy(), p), "parent written"
    return psi_all[nc:-nc].reshape(nh, nc), r_all[T * 2:-T * 2].reshape(nh, nc, T, 2)


def check(case, psi, r, what):
    """Dead rows bit for bit, everything by the metric under max(1e-6, 4 x floor)."""
    assert not np.isnan(psi).any() and not np.isnan(r).any()
    for h in range(case.n_hyp):
        dead = case.dead_rows(h)
        want = case.r64[h][:, dead].astype(F32)  # logzero, or logp[0, c]: both exact in f32
        assert np.array_equal(want.astype(F64), case.r64[h][:, dead])
        assert np.array_equal(r[h][:, dead], want), f"{what}: hypothesis {h}: rows outside [start, end)"
    err_psi, err_r = R.rel_err(psi, case.psi64), R.rel_err(r, case.r64)
    b = R.bound(case.floor)
    print(f"{what}: floor {case.floor:.3g} bound {b:.3g} kernel psi {err_psi:.3g} r {err_r:.3g}")
    assert max(err_psi, err_r) <= b, (err_psi, err_r, b)


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("fam,n_cand,T", ROWS, ids=[f"{f}-n{n}-T{t}" for f, n, t in ROWS])
def test_prefix_score_matches_f64(fam, n_cand, T, entry):
    assert fam.startswith(family(n_cand))
    V = vocab(n_cand)
    logp_d, logp = device_logp(T, V)
    kind, ols = ENTRIES[entry]
    case = R.PrefixCase(logp, BLANK, V - 1, ols, n_cand, seed=n_cand * 1000 + T)
    assert (case.cands == V - 1).any() and (case.cands == BLANK).any()
    assert any(case.lasts[h] in case.cands[h] for h in range(3))
    psi, r = launch(case, kind, logp_d)
    check(case, psi, r, f"{fam} n_cand={n_cand} T={T} {entry}")


@pytest.mark.parametrize("entry,ols", [("meta", (5, 2, 9)), ("dev", (5, 5, 5))], ids=["meta-ol5.2.9", "dev-ol5"])
def test_prefix_as_long_as_the_utterance(entry, ols):
    """ol >= T: no live frame, everything logzero but the <eos> psi."""
    T, V, n_cand = 2, 40, 5
    logp_d, logp = device_logp(T, V)
    case = R.PrefixCase(logp, BLANK, V - 1, ols, n_cand, seed=7)
    psi, r = launch(case, entry, logp_d)
    assert np.all(r == LZ)
    is_eos = case.cands == V - 1
    assert is_eos.sum() == 3 and np.all(psi[~is_eos] == LZ)
    check(case, psi, r, f"score2<256> ol>=T {entry}")


@pytest.mark.parametrize("ol", [0, 2])
@pytest.mark.parametrize("win", list(WINDOWS))
@pytest.mark.parametrize("fam,n_cand,T", WIN_ROWS, ids=[f"{f}-n{n}-T{t}" for f, n, t in WIN_ROWS])
def test_prefix_score_window_matches_f64(fam, n_cand, T, win, ol):
    """ea_ctc_prefix_score_win; a window starting past frame 1 with ol = 0 keeps r[0] = (logp[0, c],
    logzero) below a logzero gap."""
    assert fam.startswith(family(n_cand))
    V = vocab(n_cand)
    logp_d, logp = device_logp(T, V)
    ws, we = WINDOWS[win](T)
    case = R.PrefixCase(logp, BLANK, V - 1, (ol,) * 3, n_cand, seed=n_cand + T + ol, wstart=ws, wend=we)
    psi, r = launch(case, "win", logp_d)
    if ol == 0:
        assert np.array_equal(r[:, :, 0, 0], np.stack([logp[0, case.cands[h]] for h in range(3)]))
    check(case, psi, r, f"{fam} n_cand={n_cand} T={T} window {win} ol={ol}")


def test_prefix_init_matches_f64():
    """ea_ctc_prefix_init at T=530, V=320 with a padded logits row and blank != 0: logp by the
    log-softmax rule of test_decoder_ops_gpu.py, r0 = (logzero, cumulative blank log-prob)
    against the float64 sum of the kernel's own logp."""
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    T, V, blank = 530, 320, 5
    x = R.ctc_logits(T, V, blank, seed=11, ld=V + 3)
    xd = torch.from_numpy(x).cuda()
    logp_buf, logp_d = guarded(T * V, V)
    r0_buf, r0_d = guarded(T * 2, 2)
    assert lib.ea_ctc_prefix_init(T, V, xd.data_ptr(), V + 3, blank, logp_d.data_ptr(), r0_d.data_ptr(),
                                  ops.stream()) == 0
    torch.cuda.synchronize()
    la, ra = logp_buf.cpu().numpy(), r0_buf.cpu().numpy()
    assert np.all(la[:V] == SENT) and np.all(la[-V:] == SENT) and np.all(ra[:2] == SENT) and np.all(ra[-2:] == SENT)
    logp, r0 = la[V:-V].reshape(T, V), ra[2:-2].reshape(T, 2)
    ref = torch.log_softmax(torch.from_numpy(x[:, :V]).double(), -1).numpy()
    err = float((np.abs(logp - ref) / (np.abs(ref) + 1)).max())
    assert np.all(r0[:, 0] == LZ)
    r64, r32 = R.initial_state_ref(logp, blank, F64), R.initial_state_ref(logp, blank, F32)
    floor, err_r = R.rel_err(r32, r64), R.rel_err(r0, r64)
    print(f"init: logp err {err:.3g} of {LOGSM_BOUND:.3g}; r0 floor {floor:.3g} bound {R.bound(floor):.3g} "
          f"kernel {err_r:.3g}")
    assert err <= LOGSM_BOUND, err
    assert err_r <= R.bound(floor), (err_r, floor)


@pytest.mark.parametrize("T_old", [0, 1, 12])
def test_prefix_extend_matches_f64(T_old):
    """ea_ctc_prefix_extend from T_old frames to 30: the copied rows bit for bit, r^n logzero and
    r^b the blank sum from the last copied row (from logzero for T_old = 0)."""
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    T, V = 30, 40
    logp_d, logp = device_logp(T, V)
    r_old = R.chain_ref(logp, BLANK, V - 1, [3, 9], F64).astype(F32)[:T_old]  # real r^n and r^b values
    old_d = torch.from_numpy(np.ascontiguousarray(r_old)).cuda() if T_old else torch.empty(0, 2, device="cuda")
    buf, r_d = guarded(T * 2, T * 2)
    assert lib.ea_ctc_prefix_extend(T_old, T, V, BLANK, logp_d.data_ptr(), old_d.data_ptr(), r_d.data_ptr(),
                                    ops.stream()) == 0
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert np.all(a[:T * 2] == SENT) and np.all(a[-T * 2:] == SENT)
    r = a[T * 2:-T * 2].reshape(T, 2)
    assert np.array_equal(r[:T_old], r_old)
    assert np.all(r[max(T_old, 1):, 0] == LZ)
    if T_old == 0:
        assert np.all(r[0] == LZ)
    r64, r32 = R.extend_state_ref(logp, BLANK, r_old, T, F64), R.extend_state_ref(logp, BLANK, r_old, T, F32)
    floor, err = R.rel_err(r32, r64), R.rel_err(r, r64)
    print(f"extend T_old={T_old}: floor {floor:.3g} bound {R.bound(floor):.3g} kernel {err:.3g}")
    assert err <= R.bound(floor), (err, floor)
