"""The unfused attention softmax (ea_attn_softmax_fwd / ea_attn_softmax_bwd, csrc/attention.hip:
masked softmax + dropout + the rel-shift band gather / scatter of every fp32 run and every head
dim != 64) through the C-ABI against a float64 torch restatement on the CPU.

Forward reference: scores = scale * (S + BD_raw[i, T1-1-i+j]), masked where j >= min(klen[b], T2)
or (causal and j > i), softmax with masked entries and fully-masked rows exactly 0.
Backward reference: dS = scale * P * (dP - rowsum(P * dP)), dP = dPd * mask / (1 - p), on a P that
comes from the f64 forward (rounded to f32), so the backward is tested without the forward kernel.

Shapes cross every register-array instantiation (T2 <= 64, 128, 256, 512, 1024, 2048) and the
refusal above 2048.  Dropout masks are recovered from the kernel's own output (the hash is not
restated).

Tolerances (f32 noise floor = the same formula in f32 torch against f64 on these inputs, measured
with f32_floors() below; the kernel is allowed 8x):
  forward  P : |got - ref| <= FWD_BOUND * (ref + 1e-4 / T2)
               floor 5.7e-7, bound 4.5e-6, kernel worst 9.1e-7
  backward dS: |got - ref| <= BWD_BOUND * scale * P * (|dP| + rowsum(P * |dP|))   (the condition
               of p * (d - dot): d - dot cancels, so the error is relative to its operands)
               floor 1.5e-7, bound 1.2e-6, kernel worst 1.2e-7
  bf16 outputs add 2^-8 * |ref|.
"""
import numpy as np
import pytest
import torch

from test_attention_gpu import rel_shift

SENT = -7.25  # exact in bf16
FWD_BOUND = 4.5e-6
BWD_BOUND = 1.2e-6
BF16 = 2.0 ** -8
CROSS_T2 = [1, 63, 64, 65, 128, 129, 257, 513, 1025, 2048]
REL_T = [5, 64, 65, 130]
FWD_CASES = ([("cross", t) for t in CROSS_T2] + [("rel", t) for t in REL_T] +
             [("causal", 7), ("causal", 65), ("causal_rel", 7), ("causal_rel", 65)])
BWD_T2 = [63, 64, 65, 129, 513, 2048]


def rup(n, m=8):
    return (n + m - 1) // m * m


def band_index(T):
    """rel_shift as an index law: shifted[i, j] = raw[i, T-1-i+j]."""
    return T - 1 - torch.arange(T)[:, None] + torch.arange(T)[None, :]


def gather_band(bd):
    """bd (B, H, T, 2T-1) -> (B, H, T, T)."""
    T = bd.shape[2]
    return torch.gather(bd, -1, band_index(T).expand(*bd.shape[:2], T, T))


def causal_keep(T1, T2):
    return torch.arange(T2)[None, :] <= torch.arange(T1)[:, None]


def keep_mask(B, T1, T2, klen, causal):
    """(B, 1, T1, T2) bool, True = key j takes part in row i."""
    kl = torch.full((B,), T2) if klen is None else torch.tensor(klen).clamp(max=T2)
    keep = (torch.arange(T2)[None, :] < kl[:, None])[:, None, None, :].expand(B, 1, T1, T2)
    if causal:
        keep = keep & causal_keep(T1, T2)[None, None]
    return keep


def softmax_ref(S, bd, keep, scale, shift=None):
    """In S's dtype (f64: the reference; f32: the noise floor).  Differentiable."""
    sc = S if bd is None else S + (shift or gather_band)(bd)
    sc = (sc * scale).masked_fill(~keep, float("-inf"))
    mx = sc.amax(-1, keepdim=True)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    e = torch.exp(sc - mx)
    s = e.sum(-1, keepdim=True)
    return e / torch.where(s > 0, s, torch.ones_like(s))


def softmax_bwd_ref(P, dP, scale):
    return scale * P * (dP - (P * dP).sum(-1, keepdim=True))


def bwd_scale(P, dP, scale):
    """The operands' size of p * (d - dot): what an f32 error of dS is relative to."""
    return scale * P * (dP.abs() + (P * dP.abs()).sum(-1, keepdim=True))


class Case:
    def __init__(self, kind, T, B=2, H=2):
        g = torch.Generator().manual_seed(7919 * len(kind) + T)
        self.kind, self.B, self.H = kind, B, H
        self.T1, self.T2 = (3, T) if kind == "cross" else (T, T)
        self.causal = kind.startswith("causal")
        rel = kind in ("rel", "causal_rel")
        # scale * (S [+ BD]) is about N(0, 1)
        self.scale = 0.35 if rel else 0.5
        self.S = torch.randn(B, H, self.T1, self.T2, generator=g) * 2
        self.bd = torch.randn(B, H, T, 2 * T - 1, generator=g) * 2 if rel else None
        T2 = self.T2
        # all keys / clamped + empty / one key + ragged / full + ragged
        self.klens = [None, [T2 + 3, 0], [1, max(T2 - 2, 1)], [T2, T2 // 2 + 1]]

    def keep(self, klen):
        return keep_mask(self.B, self.T1, self.T2, klen, self.causal)

    def ref(self, klen, dtype=torch.float64):
        bd = None if self.bd is None else self.bd.to(dtype)
        return softmax_ref(self.S.to(dtype), bd, self.keep(klen), self.scale)


def fwd_err(got, ref, T2):
    return ((got.double() - ref).abs() / (ref + 1e-4 / T2)).max().item()


def bwd_err(got, ref, den):
    return ((got.double() - ref).abs() / (den + 1e-300)).max().item()


def bwd_inputs(T1, T2, klen, causal, rel, seed):
    g = torch.Generator().manual_seed(seed)
    B = H = 2
    S = torch.randn(B, H, T1, T2, generator=g, dtype=torch.float64)
    bd = torch.randn(B, H, T1, 2 * T1 - 1, generator=g, dtype=torch.float64) if rel else None
    keep = keep_mask(B, T1, T2, klen, causal)
    scale = 0.7
    P = softmax_ref(S, bd, keep, scale).float()
    dPd = torch.randn(B, H, T1, T2, generator=g)
    return S, bd, keep, scale, P, dPd


def f32_floors():
    """Worst error of the f32 torch evaluation of the same formulas on the tests' own inputs."""
    fwd = bwd = 0.0
    for kind, T in FWD_CASES:
        c = Case(kind, T)
        for klen in c.klens:
            fwd = max(fwd, fwd_err(c.ref(klen, torch.float32), c.ref(klen), c.T2))
    for T2 in BWD_T2 + REL_T:
        rel = T2 in REL_T
        _, _, _, scale, P, dPd = bwd_inputs(T2 if rel else 3, T2, [T2 + 3, T2 // 2 + 1], False, rel, T2)
        ref = softmax_bwd_ref(P.double(), dPd.double(), scale)
        bwd = max(bwd, bwd_err(softmax_bwd_ref(P, dPd, scale), ref, bwd_scale(P.double(), dPd.double(), scale)))
    return {"fwd": fwd, "bwd": bwd}


# ------------------------------------------------------------------ reference self-checks (CPU)
def test_reference_matches_oracle_mha_core():
    """softmax_ref's weights are mha_core's (masked_fill(min) -> softmax -> masked_fill(0)):
    with v = I the oracle returns the attention matrix itself."""
    from oracle.asr_oracle import mha_core
    g = torch.Generator().manual_seed(3)
    B, H, T1, T2, dk = 2, 2, 6, 9, 4
    q = torch.randn(B, H, T1, dk, generator=g, dtype=torch.float64)
    k = torch.randn(B, H, T2, dk, generator=g, dtype=torch.float64)
    extra = torch.randn(B, H, T1, T2, generator=g, dtype=torch.float64)
    keep = keep_mask(B, T1, T2, [T2 + 1, 0], False)
    eye = torch.eye(T2, dtype=torch.float64).expand(B, H, T2, T2)
    w = mha_core(q, k, eye, extra, keep[:, 0], 0.0, False, dk)
    S = torch.matmul(q, k.transpose(-2, -1)) + extra
    ours = softmax_ref(S, None, keep, 1.0 / dk ** 0.5)
    torch.testing.assert_close(ours, w, rtol=1e-13, atol=1e-15)
    assert torch.equal(ours[1], torch.zeros_like(ours[1]))  # klen = 0: exactly 0, not NaN
    keep = keep_mask(B, T2, T2, [T2, 4], True)
    S = torch.randn(B, H, T2, T2, generator=g, dtype=torch.float64)
    w = mha_core(torch.eye(T2, dtype=torch.float64).expand(B, H, T2, T2), eye, eye, S - eye, keep[:, 0], 0.0, False, 1)
    torch.testing.assert_close(softmax_ref(S, None, keep, 1.0), w, rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("T", [1, 2, 5, 64, 65])
def test_gather_law_matches_view_rel_shift(T):
    bd = torch.randn(2, 3, T, 2 * T - 1, generator=torch.Generator().manual_seed(T), dtype=torch.float64)
    assert torch.equal(gather_band(bd), rel_shift(bd))


# ------------------------------------------------------------------ GPU runners
def _pad(x, ld, fill, dtype=None):
    out = torch.full((*x.shape[:-1], ld), fill, dtype=dtype or x.dtype)
    out[..., : x.shape[-1]] = x
    return out


def _bd_dev(bd):
    """(B, H, T, 2T-1) -> the kernel's [h][b][i][ldBD], NaN in the padding columns."""
    if bd is None:
        return None, 0
    ld = rup(bd.shape[-1])
    return _pad(bd.permute(1, 0, 2, 3).float(), ld, float("nan")).cuda(), ld


def run_fwd(S, bd, klen, causal, scale, p=0.0, seed=0, pd_dtype=torch.float32, alias=False):
    """-> P, Pd on the CPU, (B, H, T1, ld) with the padding columns in."""
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import dt, lib
    B, H, T1, T2 = S.shape
    ld = rup(T2)
    Sd = _pad(S, ld, SENT).cuda()
    P = Sd if alias else torch.full_like(Sd, SENT)
    Pd = torch.full((B, H, T1, ld), SENT, dtype=pd_dtype, device="cuda")
    bdd, ldbd = _bd_dev(bd)
    kd = None if klen is None else torch.tensor(klen, dtype=torch.int64).cuda()
    lib.ea_attn_softmax_fwd(B, H, T1, T2, scale, Sd.data_ptr(), ld, 0 if bdd is None else bdd.data_ptr(), ldbd,
                            0 if kd is None else kd.data_ptr(), int(causal), float(p), seed, P.data_ptr(), ld,
                            Pd.data_ptr(), dt(Pd), ld, ops.stream())
    torch.cuda.synchronize()
    return P.cpu(), Pd.cpu()


def run_bwd(P, dPd, scale, p=0.0, seed=0, ds_dtype=torch.float32, dbd=False):
    """-> dS (B, H, T1, ld), dBD (H, B, T1, ldBD) or None, on the CPU with their padding in.
    The inputs' padding columns are NaN: a read past T2 would poison the row sum."""
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import dt, lib
    B, H, T1, T2 = P.shape
    ld = rup(T2)
    Pp, dp = _pad(P, ld, float("nan")).cuda(), _pad(dPd, ld, float("nan")).cuda()
    dS = torch.full((B, H, T1, ld), SENT, dtype=ds_dtype, device="cuda")
    ldbd = rup(2 * T1 - 1)
    dB = torch.full((H, B, T1, ldbd), float("nan"), dtype=ds_dtype, device="cuda") if dbd else None
    lib.ea_attn_softmax_bwd(B, H, T1, T2, scale, dp.data_ptr(), ld, Pp.data_ptr(), ld, float(p), seed, dS.data_ptr(),
                            dt(dS), ld, 0 if dB is None else dB.data_ptr(), ldbd, ops.stream())
    torch.cuda.synchronize()
    return dS.cpu(), None if dB is None else dB.cpu()


# ------------------------------------------------------------------ forward
@pytest.mark.gpu
@pytest.mark.parametrize("kind,T", FWD_CASES)
def test_fwd_matches_f64(kind, T):
    """Every klen pattern (none, clamped + empty, one key + ragged, full + ragged) x Pd dtype x
    P aliasing S or not.  Kernel worst error over all cases: 9.1e-7 of FWD_BOUND = 4.5e-6."""
    c = Case(kind, T)
    T2 = c.T2
    worst = 0.0
    for klen in c.klens:
        keep = c.keep(klen).expand(c.B, c.H, c.T1, T2)
        ref = c.ref(klen)
        P0, Pd0 = run_fwd(c.S, c.bd, klen, c.causal, c.scale)
        got = P0[..., :T2]
        err = fwd_err(got, ref, T2)
        worst = max(worst, err)
        assert err <= FWD_BOUND, (klen, err)
        assert torch.equal(got[~keep], torch.zeros(int((~keep).sum())))  # masked: exactly 0, never NaN
        if klen is not None and 0 in klen:
            b = klen.index(0)
            assert torch.equal(P0[b, ..., :T2], torch.zeros(c.H, c.T1, T2))
            assert torch.equal(Pd0[b, ..., :T2], torch.zeros(c.H, c.T1, T2))
        assert torch.equal(Pd0[..., :T2], got)  # p = 0: Pd is P
        for t in (P0, Pd0):
            assert torch.equal(t[..., T2:], torch.full_like(t[..., T2:], SENT))
        P1, Pd1 = run_fwd(c.S, c.bd, klen, c.causal, c.scale, alias=True)  # in place, as attn_fwd
        assert torch.equal(P1, P0) and torch.equal(Pd1, Pd0)
        for alias in (False, True):
            P2, Pd2 = run_fwd(c.S, c.bd, klen, c.causal, c.scale, pd_dtype=torch.bfloat16, alias=alias)
            assert torch.equal(P2, P0)
            assert torch.equal(Pd2[..., :T2], got.to(torch.bfloat16))
            assert torch.equal(Pd2[..., T2:], torch.full_like(Pd2[..., T2:], SENT))
    print(f"attn_softmax_fwd {kind} T={T}: worst err {worst:.3g}")


@pytest.mark.gpu
def test_refuses_long_rows_and_band_with_cross_attention():
    """T2 = 2049 has no instantiation: bad argument, and nothing is written.  The rel term needs
    T1 == T2."""
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import F32, HipError, lib
    T2 = 2049
    ld = rup(T2)
    Sd = _pad(torch.randn(1, 1, 3, T2), ld, SENT).cuda()
    P, Pd, dS = (torch.full_like(Sd, SENT) for _ in range(3))
    with pytest.raises(HipError, match="bad argument"):
        lib.ea_attn_softmax_fwd(1, 1, 3, T2, 1.0, Sd.data_ptr(), ld, 0, 0, 0, 0, 0.0, 0, P.data_ptr(), ld,
                                Pd.data_ptr(), F32, ld, ops.stream())
    with pytest.raises(HipError, match="bad argument"):
        lib.ea_attn_softmax_bwd(1, 1, 3, T2, 1.0, Sd.data_ptr(), ld, Sd.data_ptr(), ld, 0.0, 0, dS.data_ptr(), F32,
                                ld, 0, 0, ops.stream())
    torch.cuda.synchronize()
    for t in (P, Pd, dS):
        assert torch.equal(t.cpu(), torch.full(t.shape, SENT))
    with pytest.raises(HipError, match="bad argument"):
        run_fwd(torch.randn(1, 1, 5, 6), torch.randn(1, 1, 5, 9), None, False, 1.0)
    with pytest.raises(HipError, match="bad argument"):
        run_bwd(torch.rand(1, 1, 5, 6), torch.randn(1, 1, 5, 6), 1.0, dbd=True)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,T", [("cross", 129), ("rel", 130), ("causal", 65), ("cross", 2048)])
def test_fwd_dropout_mask(kind, T):
    c = Case(kind, T)
    T2, p = c.T2, 0.1
    klen = [T2 + 3, T2 // 2 + 1]
    keep = c.keep(klen).expand(c.B, c.H, c.T1, T2)
    P, Pd = (t[..., :T2] for t in run_fwd(c.S, c.bd, klen, c.causal, c.scale, p=p, seed=1234))
    assert bool((P[keep] > 0).all())  # so no unmasked entry is left out below
    assert torch.equal(Pd[~keep], torch.zeros(int((~keep).sum())))
    kept = Pd != 0
    np.testing.assert_allclose(Pd[kept].numpy(), (P[kept].double() / (1 - p)).numpy(), rtol=1e-6, atol=0)
    n = int(keep.sum())
    q = 1 - round(p * 65536) / 65536
    assert abs(int(kept.sum()) - n * q) <= 6 * (n * q * (1 - q)) ** 0.5, (int(kept.sum()), n * q)
    P16, Pd16 = (t[..., :T2] for t in run_fwd(c.S, c.bd, klen, c.causal, c.scale, p=p, seed=1234,
                                              pd_dtype=torch.bfloat16, alias=True))
    assert torch.equal(P16, P)
    assert torch.equal(Pd16 != 0, kept)
    assert torch.equal(Pd16, Pd.to(torch.bfloat16))
    _, again = run_fwd(c.S, c.bd, klen, c.causal, c.scale, p=p, seed=1234)
    assert torch.equal(again[..., :T2], Pd)
    _, other = run_fwd(c.S, c.bd, klen, c.causal, c.scale, p=p, seed=1235)
    assert not torch.equal(other[..., :T2] != 0, kept)


# ------------------------------------------------------------------ backward
def _check_ds(dS, ref, den, dtype, T2):
    got = dS[..., :T2].double()
    tol = BWD_BOUND * den + (BF16 * ref.abs() if dtype == torch.bfloat16 else 0)
    assert bool(((got - ref).abs() <= tol).all()), ((got - ref).abs() / (den + 1e-300)).max().item()
    assert torch.equal(got[den == 0], torch.zeros(int((den == 0).sum()), dtype=torch.float64))
    assert torch.equal(dS[..., T2:], torch.full_like(dS[..., T2:], SENT))


@pytest.mark.gpu
@pytest.mark.parametrize("T2", BWD_T2)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bwd_matches_f64(T2, dtype):
    """Cross-attention rows (T1 = 3), clamped + ragged klen.  Kernel worst error (f32 dS) 1.2e-7 of
    BWD_BOUND = 1.2e-6."""
    _, _, _, scale, P, dPd = bwd_inputs(3, T2, [T2 + 3, T2 // 2 + 1], False, False, T2)
    ref = softmax_bwd_ref(P.double(), dPd.double(), scale)
    den = bwd_scale(P.double(), dPd.double(), scale)
    dS, _ = run_bwd(P, dPd, scale, ds_dtype=dtype)
    if dtype == torch.float32:
        print(f"attn_softmax_bwd T2={T2}: err {bwd_err(dS[..., :T2], ref, den):.3g}")
    _check_ds(dS, ref, den, dtype, T2)


@pytest.mark.gpu
@pytest.mark.parametrize("T", REL_T)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("causal", [False, True])
def test_bwd_band_gradient(T, dtype, causal):
    """dBD is the kernel's own dS on the band and exact zeros off it, columns >= 2T-1 untouched;
    and it equals autograd through the f64 forward built on the view-based rel_shift."""
    klen = [T + 3, T // 2 + 1]
    S, bd, keep, scale, P, dPd = bwd_inputs(T, T, klen, causal, True, 31 * T + causal)
    ref = softmax_bwd_ref(P.double(), dPd.double(), scale)
    den = bwd_scale(P.double(), dPd.double(), scale)
    dS, dB = run_bwd(P, dPd, scale, ds_dtype=dtype, dbd=True)
    _check_ds(dS, ref, den, dtype, T)
    n = 2 * T - 1
    assert bool(dB[..., n:].isnan().all())  # untouched
    band = dB[..., :n].permute(1, 0, 2, 3)  # (B, H, T, 2T-1)
    assert not bool(band.isnan().any())  # every entry written
    expect = torch.zeros_like(band)
    expect.scatter_(-1, band_index(T).expand(2, 2, T, T), dS[..., :T])
    assert torch.equal(band, expect)
    bd_ = bd.clone().requires_grad_(True)
    Pa = softmax_ref(S, bd_, keep, scale, shift=rel_shift)
    torch.testing.assert_close(Pa.detach().float(), P, rtol=0, atol=0)
    (Pa * dPd.double()).sum().backward()
    tol = BWD_BOUND * den.max() + (BWD_BOUND + (BF16 if dtype == torch.bfloat16 else 0)) * bd_.grad.abs()
    assert bool(((band.double() - bd_.grad).abs() <= tol).all())


@pytest.mark.gpu
@pytest.mark.parametrize("kind,T", [("cross", 129), ("rel", 65), ("causal_rel", 65)])
def test_bwd_regenerates_the_forward_dropout_mask(kind, T):
    c = Case(kind, T)
    T2, p, seed = c.T2, 0.1, 77
    klen = [T2 + 3, T2 // 2 + 1]
    keep = c.keep(klen).expand(c.B, c.H, c.T1, T2)
    Pk, Pd = (t[..., :T2] for t in run_fwd(c.S, c.bd, klen, c.causal, c.scale, p=p, seed=seed))
    assert bool((Pk[keep] > 0).all())
    mask = (Pd != 0).double()  # where P == 0 the mask is unknown and multiplies 0
    P = c.ref(klen).float()
    dPd = torch.randn(c.S.shape, generator=torch.Generator().manual_seed(T))
    dP = dPd.double() * mask / (1 - p)
    ref = softmax_bwd_ref(P.double(), dP, c.scale)
    den = bwd_scale(P.double(), dP, c.scale)
    dS, dB = run_bwd(P, dPd, c.scale, p=p, seed=seed, dbd=c.bd is not None)
    _check_ds(dS, ref, den, torch.float32, T2)
    wrong = softmax_bwd_ref(P.double(), dPd.double(), c.scale)  # no mask: must be far away
    assert float((dS[..., :T2].double() - wrong).abs().max()) > 1e-2 * float(ref.abs().max())


if __name__ == "__main__":
    print(f32_floors())
