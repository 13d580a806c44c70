"""The legacy rel-pos law in the unfused attention kernels (ea_attn_softmax_fwd_mode /
ea_attn_softmax_bwd_mode with EA_REL_LEGACY) and the table kernels (ea_legacy_pext /
ea_legacy_pext_fold), through the C ABI against a float64 restatement on the CPU.

Inputs come from head-dim-16 operands: S = (q+u)·k^T and the band BD[r, k] = (q_r+v)·Pext[k] over
2T-1 columns, both handed to the kernel rounded to f32.  The f64 reference is
softmax(scale * (S + legacy rel_shift)) with the shift written from the index law
(tests/legacy_relpos_goldens.py, equal bit-for-bit to the reference's view-based rel_shift:
tests/test_legacy_relpos_cpu.py); its band read is checked here against legacy_shift((q+v)·p^T).

Shapes (B, H, T): (2, 4, 5), (2, 4, 33), (1, 2, 65): one and two 64-lane row chunks, ragged
klen.  Tolerances are those of tests/test_attn_softmax_gpu.py (FWD_BOUND on P, BWD_BOUND on dS,
2^-8 relative for bf16 outputs); the band gradient must be the kernel's own dS placed by the row
law, exact zeros elsewhere (column T included), every row written in full."""
import numpy as np
import pytest
import torch

from legacy_relpos_goldens import legacy_shift, pext, pext_fold
from test_attn_softmax_gpu import (BF16, BWD_BOUND, FWD_BOUND, SENT, _pad, bwd_err, bwd_scale, fwd_err, keep_mask, rup,
                                   softmax_bwd_ref, softmax_ref)

pytestmark = pytest.mark.gpu

SHAPES = [(2, 4, 5), (2, 4, 33), (1, 2, 65)]
DK = 16


def legacy_gather(bd):
    """bd (B, H, T, 2T-1) -> (B, H, T, T): bd[i + (j > i), T-1-i+j]."""
    T = bd.shape[2]
    i = torch.arange(T).view(T, 1).expand(T, T)
    j = torch.arange(T).view(1, T).expand(T, T)
    row = (i + (j > i).long()).clamp(max=T - 1)
    return bd[..., row, T - 1 - i + j]


def legacy_scatter(ds):
    """dS (B, H, T, T) -> dBD (B, H, T, 2T-1) by the row law: the adjoint of legacy_gather, but
    for column T.  That column multiplies Pext's constant zero row (score entries j == i+1), so
    nothing downstream reads its gradient and the kernels write it as zero."""
    B, H, T, _ = ds.shape
    out = torch.zeros(B, H, T, 2 * T - 1, dtype=ds.dtype)
    for i in range(T):
        for j in range(T):
            if j != i + 1:
                out[:, :, i + (j > i), T - 1 - i + j] += ds[:, :, i, j]
    return out


def make(B, H, T, seed):
    g = torch.Generator().manual_seed(seed)
    q, k = (torch.randn(B, H, T, DK, generator=g, dtype=torch.float64) for _ in range(2))
    u, v = (torch.randn(1, H, 1, DK, generator=g, dtype=torch.float64) * 0.5 for _ in range(2))
    p = torch.randn(H, T, DK, generator=g, dtype=torch.float64)
    S = (q + u) @ k.transpose(-1, -2)
    px = torch.stack([pext(p[h]) for h in range(H)])  # (H, 2T-1, dk)
    bd = (q + v) @ px.transpose(-1, -2)  # (B, H, T, 2T-1)
    full = (q + v) @ p.transpose(-1, -2)  # (B, H, T, T): what the reference shifts
    torch.testing.assert_close(legacy_gather(bd), legacy_shift(full), rtol=1e-13, atol=1e-13)
    klen = [T, max(T * 3 // 5, 1)][:B]
    return S.float(), bd.float(), klen, 1.0 / DK ** 0.5


def _bd_dev(bd, dtype=torch.float32):
    ld = rup(bd.shape[-1])
    return _pad(bd.permute(1, 0, 2, 3).to(dtype), ld, float("nan")).cuda(), ld


def run_fwd(S, bd, klen, scale, mode, causal=False, p=0.0, seed=0):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import dt, lib
    B, H, T1, T2 = S.shape
    ld = rup(T2)
    Sd = _pad(S, ld, SENT).cuda()
    P = torch.full_like(Sd, SENT)
    Pd = torch.full_like(Sd, SENT)
    bdd, ldbd = _bd_dev(bd) if bd is not None else (None, 0)
    kd = torch.tensor(klen, dtype=torch.int64).cuda()
    lib.ea_attn_softmax_fwd_mode(B, H, T1, T2, scale, Sd.data_ptr(), ld, 0 if bdd is None else bdd.data_ptr(), ldbd,
                                 kd.data_ptr(), int(causal), float(p), seed, P.data_ptr(), ld, Pd.data_ptr(), dt(Pd), ld,
                                 mode, ops.stream())
    torch.cuda.synchronize()
    return P.cpu(), Pd.cpu()


def run_bwd(P, dPd, scale, mode, ds_dtype=torch.float32, p=0.0, seed=0, dbd=True):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import dt, lib
    B, H, T1, T2 = P.shape
    ld = rup(T2)
    Pp, dp = _pad(P, ld, float("nan")).cuda(), _pad(dPd, ld, float("nan")).cuda()
    dS = torch.full((B, H, T1, ld), SENT, dtype=ds_dtype, device="cuda")
    ldbd = rup(2 * T1 - 1)
    dB = torch.full((H, B, T1, ldbd), float("nan"), dtype=ds_dtype, device="cuda") if dbd else None
    lib.ea_attn_softmax_bwd_mode(B, H, T1, T2, scale, dp.data_ptr(), ld, Pp.data_ptr(), ld, float(p), seed,
                                 dS.data_ptr(), dt(dS), ld, 0 if dB is None else dB.data_ptr(), ldbd, mode, ops.stream())
    torch.cuda.synchronize()
    return dS.cpu(), None if dB is None else dB.cpu()


@pytest.mark.parametrize("B,H,T", SHAPES)
def test_legacy_fwd_matches_f64(B, H, T):
    from espnet_amd._lib import REL_LATEST, REL_LEGACY
    S, bd, klen, scale = make(B, H, T, 100 + T)
    keep = keep_mask(B, T, T, klen, False)
    ref = softmax_ref(S.double(), bd.double(), keep, scale, shift=legacy_gather)
    P, Pd = run_fwd(S, bd, klen, scale, REL_LEGACY)
    err = fwd_err(P[..., :T], ref, T)
    print(f"legacy softmax fwd {(B, H, T)}: err {err:.3g} of {FWD_BOUND}")
    assert err <= FWD_BOUND
    keep4 = keep.expand(B, H, T, T)
    assert torch.equal(P[..., :T][~keep4], torch.zeros(int((~keep4).sum())))
    assert torch.equal(Pd, P)
    assert torch.equal(P[..., T:], torch.full_like(P[..., T:], SENT))
    if T > 2:  # and it is not the latest law
        latest, _ = run_fwd(S, bd, klen, scale, REL_LATEST)
        assert float((latest[..., :T] - P[..., :T]).abs().max()) > 1e-3


@pytest.mark.parametrize("B,H,T", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_legacy_bwd_matches_f64_and_row_law(B, H, T, dtype):
    from espnet_amd._lib import REL_LEGACY
    S, bd, klen, scale = make(B, H, T, 200 + T)
    keep = keep_mask(B, T, T, klen, False)
    bd64 = bd.double().requires_grad_(True)
    P64 = softmax_ref(S.double(), bd64, keep, scale, shift=legacy_gather)
    P = P64.detach().float()
    dPd = torch.randn(B, H, T, T, generator=torch.Generator().manual_seed(T))
    ref = softmax_bwd_ref(P.double(), dPd.double(), scale)
    den = bwd_scale(P.double(), dPd.double(), scale)
    dS, dB = run_bwd(P, dPd, scale, REL_LEGACY, ds_dtype=dtype)
    got = dS[..., :T].double()
    if dtype == torch.float32:
        print(f"legacy softmax bwd {(B, H, T)}: err {bwd_err(got, ref, den):.3g} of {BWD_BOUND}")
    tol = BWD_BOUND * den + (BF16 * ref.abs() if dtype == torch.bfloat16 else 0)
    assert bool(((got - ref).abs() <= tol).all()), bwd_err(got, ref, den)
    assert torch.equal(dS[..., T:], torch.full_like(dS[..., T:], SENT))
    n = 2 * T - 1
    assert bool(dB[..., n:].isnan().all())  # the row padding is untouched
    band = dB[..., :n].permute(1, 0, 2, 3)  # (B, H, T, 2T-1)
    assert not bool(band.isnan().any())  # every band row written in full
    assert torch.equal(band, legacy_scatter(dS[..., :T]))  # the kernel's own dS, placed by the row law
    if T >= 2:
        assert torch.equal(band[..., T], torch.zeros_like(band[..., T]))  # the forced zero's column
    for r in range(T):  # columns outside [T-1-r, T-1] and [T+1, 2T-1-r]
        assert torch.equal(band[:, :, r, :T - 1 - r], torch.zeros_like(band[:, :, r, :T - 1 - r]))
        assert torch.equal(band[:, :, r, 2 * T - r:], torch.zeros_like(band[:, :, r, 2 * T - r:]))
    # and autograd through the f64 forward (but for the constant-zero column T)
    (P64 * dPd.double()).sum().backward()
    want = bd64.grad.clone()
    if T >= 2:
        want[..., T] = 0
    tol = BWD_BOUND * den.max() + (BWD_BOUND + (BF16 if dtype == torch.bfloat16 else 0)) * want.abs()
    assert bool(((band.double() - want).abs() <= tol).all())


def test_legacy_dropout_mask_is_regenerated():
    from espnet_amd._lib import REL_LEGACY
    B, H, T = 2, 4, 33
    S, bd, klen, scale = make(B, H, T, 333)
    keep = keep_mask(B, T, T, klen, False).expand(B, H, T, T)
    p, seed = 0.1, 77
    P, Pd = (t[..., :T] for t in run_fwd(S, bd, klen, scale, REL_LEGACY, p=p, seed=seed))
    assert bool((P[keep] > 0).all())
    mask = (Pd != 0).double()
    np.testing.assert_allclose(Pd[Pd != 0].numpy(), (P[Pd != 0].double() / (1 - p)).numpy(), rtol=1e-6, atol=0)
    dPd = torch.randn(B, H, T, T, generator=torch.Generator().manual_seed(5))
    dP = dPd.double() * mask / (1 - p)
    ref = softmax_bwd_ref(P.double(), dP, scale)
    den = bwd_scale(P.double(), dP, scale)
    dS, dB = run_bwd(P, dPd, scale, REL_LEGACY, p=p, seed=seed)
    assert bool(((dS[..., :T].double() - ref).abs() <= BWD_BOUND * den).all())
    assert torch.equal(dB[..., :2 * T - 1].permute(1, 0, 2, 3), legacy_scatter(dS[..., :T]))


def test_latest_mode_is_the_old_entry_point_and_bad_modes_are_refused():
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import F32, REL_LATEST, REL_LEGACY, HipError, lib
    import test_attn_softmax_gpu as A
    B, H, T = 2, 4, 33
    S, bd, klen, scale = make(B, H, T, 9)
    P0, Pd0 = A.run_fwd(S, bd, klen, False, scale, p=0.1, seed=3)
    P1, Pd1 = run_fwd(S, bd, klen, scale, REL_LATEST, p=0.1, seed=3)
    assert torch.equal(P0, P1) and torch.equal(Pd0, Pd1)
    dPd = torch.randn(B, H, T, T, generator=torch.Generator().manual_seed(1))
    dS0, dB0 = A.run_bwd(P0[..., :T], dPd, scale, p=0.1, seed=3, dbd=True)
    dS1, dB1 = run_bwd(P0[..., :T], dPd, scale, REL_LATEST, p=0.1, seed=3)
    assert torch.equal(dS0, dS1) and torch.equal(dB0[..., :2 * T - 1], dB1[..., :2 * T - 1])
    with pytest.raises(HipError, match="bad argument"):
        run_fwd(S, bd, klen, scale, 2)
    with pytest.raises(HipError, match="bad argument"):
        run_bwd(P0[..., :T], dPd, scale, 2)
    with pytest.raises(HipError, match="bad argument"):  # legacy has no causal form
        run_fwd(S, bd, klen, scale, REL_LEGACY, causal=True)
    with pytest.raises(HipError, match="bad argument"):  # nor one without the band
        run_fwd(S, None, klen, scale, REL_LEGACY)
    with pytest.raises(HipError, match="bad argument"):
        run_bwd(P0[..., :T], dPd, scale, REL_LEGACY, dbd=False)
    x = torch.zeros(8, 8, device="cuda")
    with pytest.raises(HipError, match="bad argument"):
        lib.ea_legacy_pext(3, 8, x.data_ptr(), 4, x.data_ptr(), 8, F32, ops.stream())


@pytest.mark.parametrize("T", [1, 2, 3, 5, 70])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pext_and_fold_kernels(T, dtype):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import dt, lib
    d, ldp, ldx = 24, 32, 40
    g = torch.Generator().manual_seed(T)
    p = torch.randn(T, d, generator=g).to(dtype)
    pd = torch.full((T, ldp), float("nan"), dtype=dtype)
    pd[:, :d] = p
    out = torch.full((2 * T - 1, ldx), SENT, dtype=dtype, device="cuda")
    pdd = pd.cuda()
    lib.ea_legacy_pext(T, d, pdd.data_ptr(), ldp, out.data_ptr(), ldx, dt(out), ops.stream())
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.equal(out[:, :d], pext(p))
    assert torch.equal(out[:, d:], torch.full_like(out[:, d:], SENT))
    w = torch.randn(2 * T - 1, d, generator=g).to(dtype)
    wd = torch.full((2 * T - 1, ldx), float("nan"), dtype=dtype)
    wd[:, :d] = w
    wdd = wd.cuda()
    dp = torch.full((T, ldp), SENT, dtype=dtype, device="cuda")
    lib.ea_legacy_pext_fold(T, d, wdd.data_ptr(), ldx, dp.data_ptr(), ldp, dt(dp), ops.stream())
    torch.cuda.synchronize()
    dp = dp.cpu()
    assert torch.equal(dp[:, :d], pext_fold(w.float()).to(dtype))  # one f32 add, rounded once
    assert torch.equal(dp[:, d:], torch.full_like(dp[:, d:], SENT))
