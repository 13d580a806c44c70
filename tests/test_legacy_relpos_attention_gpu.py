"""The legacy rel-pos attention core in bf16 with head dim 64 against an f32 torch restatement
written from the index law (tests/legacy_relpos_goldens.py legacy_shift, equal bit-for-bit to the
reference's view-based rel_shift) on the bf16-rounded inputs:

  * the fused kernels' legacy variant (ea_attn_fused_fwd2_mode, ea_attn_fused_bwd2_mode with the
    flags layers/conformer.py passes, ea_attn_legacy_band): O, dK, dV, total dq, dp folded back to
    T rows, the band's zero pattern, NaN-prefilled outputs fully overwritten;
  * the unfused kernels at this head dim (q + bias, the band GEMM against ea_legacy_pext's table,
    ea_attn_softmax_fwd_mode / _bwd_mode, the P·V and gradient GEMMs; EA_FUSED_ATTN=0): the same.

Shapes (B, H, T, klens): T = 1 (no upper triangle), 2 (the single forced zero), 3, 64 (one tile),
65 (row i+1 of the first tile's last row lives in the next tile), 130 and 137 (three tiles, both
off-diagonal kinds).  Bounds are those tests/test_attention_gpu.py applies to the latest variant:
rel-L2 < 1e-2 on O, < 2e-2 on gradients."""
import math

import pytest
import torch

from legacy_relpos_goldens import legacy_shift, pext, pext_fold
from test_attention_gpu import _rel

pytestmark = pytest.mark.gpu

DEV = "cuda"
bf = torch.bfloat16
SHAPES = [(1, 1, 1, [1]), (1, 1, 2, [2]), (2, 1, 3, [3, 2]), (2, 2, 64, [64, 1]), (2, 2, 65, [65, 40]),
          (1, 2, 130, [130]), (2, 3, 137, [137, 100])]


def reference(q, k, v, u, vb, p, klen, H):
    """f32 torch on the CPU: q/k/v (B, T, H*64), p (T, H*64) = linear_pos(pos_emb)."""
    B, T, d = q.shape
    dk = d // H
    qh = q.view(B, T, H, dk).transpose(1, 2)
    kh = k.view(B, T, H, dk).transpose(1, 2)
    vh = v.view(B, T, H, dk).transpose(1, 2)
    ac = torch.matmul(qh + u.view(1, H, 1, dk), kh.transpose(-2, -1))
    ph = p.view(1, T, H, dk).transpose(1, 2)
    bd = legacy_shift(torch.matmul(qh + vb.view(1, H, 1, dk), ph.transpose(-2, -1)))
    scores = (ac + bd) / math.sqrt(dk)
    mask = (torch.arange(T)[None, :] < klen[:, None])[:, None, None, :].expand(B, 1, T, T)
    scores = scores.masked_fill(~mask, torch.finfo(scores.dtype).min)
    attn = torch.softmax(scores, dim=-1).masked_fill(~mask, 0.0)
    return torch.matmul(attn, vh).transpose(1, 2).reshape(B, T, d)


def inputs(B, H, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    d = H * 64
    r = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(bf)  # noqa: E731
    q, k, v, p, dO = r(B, T, d), r(B, T, d), r(B, T, d), r(T, d), r(B, T, d)
    u, vb = (torch.randn(d, generator=g) * 0.1 for _ in range(2))
    return q, k, v, u, vb, p, dO


def pext_dev(p):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import dt, lib
    T, d = p.shape
    px = torch.empty(2 * T - 1, d, dtype=p.dtype, device=DEV)
    lib.ea_legacy_pext(T, d, p.data_ptr(), d, px.data_ptr(), d, dt(px), ops.stream())
    return px


def fused_fwd(q, k, v, u, vb, px, klen, H, p=0.0, seed=0, mask=False, mode=None, causal=False):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import REL_LEGACY, lib
    B, T, d = q.shape
    O = torch.full((B, T, d), float("nan"), dtype=bf, device=DEV)
    lse = torch.full((B * H * T,), float("nan"), device=DEV)
    ldm = 2 * ((T + 63) // 64)
    dm = torch.zeros(B * H * T * ldm, dtype=torch.int32, device=DEV) if mask else None
    lib.ea_attn_fused_fwd2_mode(B, H, T, T, 64, q.data_ptr(), d, k.data_ptr(), d, v.data_ptr(), d, u.data_ptr(),
                                vb.data_ptr(), 0 if px is None else px.data_ptr(), d, klen.data_ptr(), int(causal),
                                1 / 8, float(p), seed, O.data_ptr(), d, lse.data_ptr(),
                                0 if dm is None else dm.data_ptr(), ldm if mask else 0,
                                REL_LEGACY if mode is None else mode, ops.stream())
    torch.cuda.synchronize()
    return O, lse, dm


def fused_bwd(q, k, v, u, vb, px, klen, H, O, lse, dO, p=0.0, seed=0, dm=None, flags=2, mode=None):
    """-> dq (the q+u path), dk, dv, the legacy band (H, B, T, 2T-1) and what lies outside it, q+v."""
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import REL_LEGACY, lib
    from espnet_amd.layers.common import attn_fused_bwd, dbd_layout
    B, T, d = q.shape
    shift, ldbd = dbd_layout(T)
    nan = lambda *s: torch.full(s, float("nan"), dtype=bf, device=DEV)  # noqa: E731
    dq, dk, dv, qv = nan(B, T, d), nan(B, T, d), nan(B, T, d), nan(B, T, d)
    raw, band = nan(H * B * T * ldbd), nan(H * B * T * ldbd)
    nqb = (T + 63) // 64
    part = torch.full((2 * B * nqb * d,), float("nan"), device=DEV)
    attn_fused_bwd(B=B, H=H, T1=T, T2=T, q=q, ldq=d, k=k, ldk=d, v=v, ldv=d, bu=u, bv=vb, pp=px, ldp=d, klen=klen,
                   causal=False, scale=1 / 8, p=p, seed=seed, O=O, ldo=d, lse=lse, dO=dO, lddo=d, dq=dq, lddq=d,
                   dk=dk, lddk=d, dv=dv, lddv=d, dbd=raw, ldbd=ldbd, part=part, ldpart=d, qv_out=qv, ldqv=d,
                   dmask=dm, ldm=0 if dm is None else 2 * ((T + 63) // 64), flags=flags,
                   rel_mode=REL_LEGACY if mode is None else mode)
    lib.ea_attn_legacy_band(H * B, T, raw.data_ptr(), band.data_ptr(), ldbd, ops.stream())
    torch.cuda.synchronize()
    full = band.view(H, B, T, ldbd)
    outside = torch.cat([full[..., :shift], full[..., shift + 2 * T - 1:]], -1)
    return dq, dk, dv, full[..., shift: shift + 2 * T - 1], outside, qv, part


def unfused(q, k, v, u, vb, px, klen, H, dO=None, p=0.0, seed=0):
    """The legacy training path at head dim 64 in bf16 -> O (and dq, dk, dv, dbd (H, B, T, 2T-1), qv)."""
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import REL_LEGACY, lib
    from espnet_amd.layers.common import attn_bwd, attn_fwd
    B, T, d = q.shape
    N, P2 = B * T, 2 * T - 1
    ldbd = (P2 + 7) // 8 * 8
    qu = torch.empty(N, d, dtype=bf, device=DEV)
    qv = torch.empty(N, d, dtype=bf, device=DEV)
    lib.ea_add_pos_bias(N, H, 64, q.data_ptr(), d, u.data_ptr(), vb.data_ptr(), qu.data_ptr(), qv.data_ptr(),
                        ops.dt(qu), ops.stream())
    bd = torch.empty(H * B * T * ldbd, device=DEV)
    ops.gemm(qv, px, bd, M=T, N=P2, K=64, a_kmajor=1, b_kmajor=1, lda=d, ldb=d, ldc=ldbd, batch=B, nh=H,
             sA=(T * d, 64), sB=(0, 64), sC=(T * ldbd, B * T * ldbd), splitk=False)
    kw = dict(B=B, H=H, T1=T, T2=T, dk=64, ldq=d, ldk=d, ldv=d, scale=1 / 8, p=p, seed=seed, cd=bf)
    O, P, Pd, ldT = attn_fwd(qu, k.view(N, d), v.view(N, d), klen=klen, causal=False, bd=bd, ldbd=ldbd,
                             rel_mode=REL_LEGACY, **kw)
    if dO is None:
        torch.cuda.synchronize()
        return O.view(B, T, d)
    dq, dk, dv = (torch.empty(N, d, dtype=bf, device=DEV) for _ in range(3))
    dbd = torch.full((H * B * T * ldbd,), float("nan"), dtype=bf, device=DEV)
    attn_bwd(dO.view(N, d), qu, k.view(N, d), v.view(N, d), P, Pd, ldT, dq=dq, lddq=d, dk_=dk, lddk=d, dv=dv, lddv=d,
             dbd=dbd, ldbd=ldbd, rel_mode=REL_LEGACY, **kw)
    torch.cuda.synchronize()
    return O.view(B, T, d), dq.view(B, T, d), dk.view(B, T, d), dv.view(B, T, d), dbd.view(H, B, T, ldbd)[..., :P2], qv


@pytest.mark.parametrize("B,H,T,klens", SHAPES)
def test_legacy_attention_matches_f32_restatement(B, H, T, klens):
    q, k, v, u, vb, p, dO = inputs(B, H, T, seed=T)
    klen = torch.tensor(klens, dtype=torch.long)
    qf, kf, vf, pf = (t.float().requires_grad_(True) for t in (q, k, v, p))
    ref = reference(qf, kf, vf, u, vb, pf, klen, H)
    ref.backward(dO.float())
    qd, kd, vd, pd, dOd, ud, vbd, kld = (t.to(DEV) for t in (q, k, v, p, dO, u, vb, klen))
    px = pext_dev(pd)
    assert torch.equal(px.cpu(), pext(p))
    # the fused forward's legacy variant
    O, lse, _ = fused_fwd(qd, kd, vd, ud, vbd, px, kld, H)
    assert not bool(O.isnan().any()) and not bool(lse.isnan().any())  # fully overwritten
    e = _rel(O.cpu(), ref.detach())
    print(f"fused legacy fwd {(B, H, T)}: O rel-L2 {e:.3g}")
    assert e < 1e-2
    d = H * 64

    def _rel0(a, b):
        """_rel, or for an exactly zero reference (T = 1: a one-key softmax has dS = P (dP - D) = 0,
        so dK, dq and dp vanish) the absolute size: dP - D is the difference of two 64-term f32 dot
        products of O(1) terms in different orders, |.| <= 64 * 2^-24 * O(1) ~ 4e-6; bound 1e-5,
        returned scaled so that the callers' 2e-2 applies."""
        if float(b.norm()) == 0.0:
            return float(a.float().abs().max()) / 1e-5 * 2e-2 * 0.999
        return _rel(a, b)

    def check(tag, O_, dq, dk, dv, dbd, qv):
        assert _rel(O_.cpu(), ref.detach()) < 1e-2, tag
        e = (_rel0(dk.cpu(), kf.grad), _rel(dv.cpu(), vf.grad))
        assert max(e) < 2e-2, (tag, e)
        dbd4 = dbd.float().cpu()
        assert not bool(dbd4.isnan().any()), tag  # every band row written in full
        pxh = px.float().cpu().view(2 * T - 1, H, 64).permute(1, 0, 2)  # (H, R, 64)
        dq_v = torch.einsum("hbir,hrc->bihc", dbd4, pxh).reshape(B, T, d)
        eq = _rel0(dq.float().cpu() + dq_v, qf.grad)
        assert eq < 2e-2, (tag, eq)
        dpx = torch.einsum("hbir,bihc->rhc", dbd4, qv.float().cpu().view(B, T, H, 64)).reshape(2 * T - 1, d)
        ep = _rel0(pext_fold(dpx), pf.grad)
        assert ep < 2e-2, (tag, ep)
        # zero pattern: row r holds columns [T-1-r, T-1] and [T+1, 2T-1-r]
        r = torch.arange(T)[:, None]
        c = torch.arange(2 * T - 1)[None, :]
        outside = ~(((c >= T - 1 - r) & (c <= T - 1)) | ((c >= T + 1) & (c <= 2 * T - 1 - r)))
        if bool(outside.any()):
            assert float(dbd4[:, :, outside].abs().max()) == 0.0, tag
        print(f"{tag} legacy bwd {(B, H, T)}: dK {e[0]:.3g} dV {e[1]:.3g} dq {eq:.3g} dp {ep:.3g}")

    # the fused backward passes + the band fix-up
    dq, dk, dv, band, off_band, qv, part = fused_bwd(qd, kd, vd, ud, vbd, px, kld, H, O, lse, dOd)
    for t in (dq, dk, dv, qv):
        assert not bool(t.isnan().any())
    assert float(off_band.float().abs().max()) == 0.0  # zeros, no NaN left
    check("fused", O, dq, dk, dv, band, qv)
    # the unfused kernels
    O2, dq2, dk2, dv2, dbd2, qv2 = unfused(qd, kd, vd, ud, vbd, px, kld, H, dO=dOd)
    assert _rel(O.cpu(), O2.cpu()) < 1e-2
    check("unfused", O2, dq2, dk2, dv2, dbd2, qv2)
    assert _rel(qv, qv2.view(B, T, d)) < 1e-2


def test_fused_legacy_forward_matches_unfused_with_dropout():
    """Same dropout masks (counter hash, index (z*T + i)*T + j) in the fused legacy forward and the
    unfused legacy path; the keep bits are written."""
    B, H, T, klens = 2, 2, 65, [65, 40]
    q, k, v, u, vb, p, dO = (t.to(DEV) for t in inputs(B, H, T, seed=3))
    klen = torch.tensor(klens, dtype=torch.long, device=DEV)
    px = pext_dev(p)
    O, lse, dm = fused_fwd(q, k, v, u, vb, px, klen, H, p=0.1, seed=12345, mask=True)
    O2, dq2, dk2, dv2, dbd2, _ = unfused(q, k, v, u, vb, px, klen, H, dO=dO, p=0.1, seed=12345)
    assert _rel(O, O2) < 1e-2
    assert int((dm != 0).sum()) > 0
    O0, _, _ = fused_fwd(q, k, v, u, vb, px, klen, H)
    assert _rel(O, O0) > 5e-2  # the dropout did something
    for mask in (dm, None):  # the forward's keep bits, and the counter hash
        dq, dk, dv, band, _, _, _ = fused_bwd(q, k, v, u, vb, px, klen, H, O, lse, dO, p=0.1, seed=12345, dm=mask)
        assert _rel(dq, dq2) < 2e-2
        assert _rel(dk, dk2) < 2e-2
        assert _rel(dv, dv2) < 2e-2
        assert _rel(band, dbd2) < 2e-2
    again = fused_bwd(q, k, v, u, vb, px, klen, H, O, lse, dO, p=0.1, seed=12345, dm=dm)
    for x, y in zip((dq, dk, dv, band), again):
        assert torch.equal(x, y)  # bit-reproducible run to run


def test_fused_forward_refuses_what_has_no_legacy_form(monkeypatch):
    from espnet_amd._lib import HipError, REL_LATEST
    B, H, T = 1, 1, 5
    q, k, v, u, vb, p, dO = (t.to(DEV) for t in inputs(B, H, T))
    klen = torch.tensor([5], dtype=torch.long, device=DEV)
    px = pext_dev(p)
    fused_fwd(q, k, v, u, vb, px, klen, H)
    with pytest.raises(HipError, match="bad argument"):
        fused_fwd(q, k, v, u, vb, px, klen, H, mode=2)
    with pytest.raises(HipError, match="bad argument"):
        fused_fwd(q, k, v, u, vb, px, klen, H, causal=True)
    with pytest.raises(HipError, match="bad argument"):
        fused_fwd(q, k, v, u, vb, None, klen, H)
    monkeypatch.setenv("EA_ATTN_FWD_V1", "1")  # the original forward kernel: an error, not a latest-law result
    with pytest.raises(HipError, match="bad argument"):
        fused_fwd(q, k, v, u, vb, px, klen, H)
    O, lse, _ = fused_fwd(q, k, v, u, vb, px, klen, H, mode=REL_LATEST)  # latest still runs there
    assert not bool(O.isnan().any())
    monkeypatch.delenv("EA_ATTN_FWD_V1")
    # backward: no in-kernel d(q+v) term, no original passes
    with pytest.raises(HipError, match="bad argument"):
        fused_bwd(q, k, v, u, vb, px, klen, H, O, lse, dO, flags=3)
    with pytest.raises(HipError, match="bad argument"):
        fused_bwd(q, k, v, u, vb, px, klen, H, O, lse, dO, flags=4)
    with pytest.raises(HipError, match="bad argument"):
        fused_bwd(q, k, v, u, vb, px, klen, H, O, lse, dO, mode=2)
    monkeypatch.setenv("EA_ATTN_BWDKV_V1", "1")
    with pytest.raises(HipError, match="bad argument"):
        fused_bwd(q, k, v, u, vb, px, klen, H, O, lse, dO)
