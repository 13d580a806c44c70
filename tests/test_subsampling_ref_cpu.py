"""Pins tests/subsampling_ref.py, the float64 references the subsampling kernel tests compare
against: the per-mode index restatements against torch.nn.functional.conv2d under float64
autograd, the phase-split helpers against layers.subsampling.phase_geo's plane offsets, the
layer restatement with a dropout mask and a PE table against autograd, and the |v| < 2**24
condition of the integer grid on every geometry of test_conv_sub_kernels_gpu.py."""
import math

import pytest
import torch
import torch.nn.functional as F

import subsampling_ref as R

F64 = torch.float64
GRIDS = [(3, 3), (4, 4), (30, 9), (9, 40)]


@pytest.mark.parametrize("T1,F1", GRIDS)
def test_conv2_refs_match_autograd(T1, F1):
    g = torch.Generator().manual_seed(T1 * 100 + F1)
    B, C = 2, 5
    x1 = torch.randn(B, T1, F1, C, generator=g, dtype=F64)           # ~half negative: a real mask
    W2 = torch.randn(C + 1, C, 3, 3, generator=g, dtype=F64)
    xin = torch.relu(x1).permute(0, 3, 1, 2).clone().requires_grad_(True)
    w = W2.clone().requires_grad_(True)
    y = F.conv2d(xin, w, stride=2)                                    # (B, Co, T2, F2)
    assert y.shape[2:] == (R.down(T1), R.down(F1))
    dY = torch.randn(y.shape, generator=g, dtype=F64)
    y.backward(dY)
    x1r = torch.relu(x1)
    torch.testing.assert_close(R.conv2_fwd_ref(x1r, W2), y.detach().permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    dYn = dY.permute(0, 2, 3, 1).contiguous()
    want_dx = xin.grad.permute(0, 2, 3, 1) * (x1r > 0)
    torch.testing.assert_close(R.conv2_dgrad_ref(x1r, W2, dYn), want_dx, rtol=1e-12, atol=1e-12)
    want_dw = w.grad.reshape(C + 1, C, 9).permute(0, 2, 1)            # (Co, 9, Ci)
    torch.testing.assert_close(R.conv2_wgrad_ref(x1r, dYn), want_dw, rtol=1e-12, atol=1e-12)
    if T1 % 2 == 0:  # the last x1 row is read by no conv2 output
        assert not bool(R.conv2_dgrad_ref(x1r, W2, dYn)[:, -1].any())
    if F1 % 2 == 0:
        assert not bool(R.conv2_dgrad_ref(x1r, W2, dYn)[:, :, -1].any())
    # the im2col restatements are the same convolution
    col = R.im2col_conv2_ref(x1r)
    wk = W2.reshape(C + 1, C, 9).permute(0, 2, 1).reshape(C + 1, 9 * C)
    torch.testing.assert_close((col @ wk.t()).reshape(y.shape[0], y.shape[2], y.shape[3], -1),
                               y.detach().permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    dcol = dYn.reshape(-1, C + 1) @ wk
    torch.testing.assert_close(R.col2im_conv2_ref(dcol, x1r), want_dx, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("T1,F1", GRIDS)
def test_conv1_refs_match_autograd(T1, F1):
    g = torch.Generator().manual_seed(T1 * 100 + F1 + 7)
    B, C = 2, 8
    T, Fin = 2 * T1 + 1 + (T1 % 2 == 0), 2 * F1 + 2
    x = torch.randn(B, T, Fin, generator=g, dtype=F64)
    w1 = torch.randn(C, 9, generator=g, dtype=F64).requires_grad_(True)
    b1 = torch.randn(C, generator=g, dtype=F64).requires_grad_(True)
    pre = F.conv2d(x.unsqueeze(1), w1.reshape(C, 1, 3, 3), b1, stride=2)
    assert pre.shape[2:] == (T1, F1)
    gh = torch.randn(pre.shape, generator=g, dtype=F64)
    pre.backward(gh)
    torch.testing.assert_close(R.conv1_fwd_ref(x, w1.detach(), b1.detach()),
                               torch.relu(pre.detach()).permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    dw, db = R.conv1_wgrad_ref(x, gh.permute(0, 2, 3, 1))
    torch.testing.assert_close(dw, w1.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(db, b1.grad, rtol=1e-12, atol=1e-12)
    col = R.im2col_conv1_ref(x)
    assert not bool(col[:, 9:].any())
    torch.testing.assert_close((col[:, :9] @ w1.detach().t() + b1.detach()).reshape(B, T1, F1, C),
                               pre.detach().permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("B,T1,F1,C", [(1, 3, 3, 8), (2, 4, 4, 8), (3, 30, 9, 16), (2, 9, 40, 8), (2, 5, 6, 64)])
def test_phase_split_is_phase_geo_order(B, T1, F1, C):
    from espnet_amd._lib import CONV_FWD
    from espnet_amd.layers.subsampling import phase_geo
    geo, nI, nJ, rows = phase_geo(B, T1, F1, R.down(T1), R.down(F1), C, CONV_FWD)
    assert rows == R.plane_rows(B, T1, F1) and sum(rows) == B * T1 * F1
    # every element names its own pixel: value = ((b*T1 + t1)*F1 + f1)*C + c
    x1 = torch.arange(B * T1 * F1 * C, dtype=F64).reshape(B, T1, F1, C)
    x1p = R.phase_split(x1, B, T1, F1, C)
    assert x1p.shape == (B * T1 * F1, C)
    flat = x1p.reshape(-1)
    for b in range(B):
        for t1 in (0, 1, T1 - 2, T1 - 1):
            for f1 in (0, 1, F1 - 2, F1 - 1):
                a, e = t1 & 1, f1 & 1
                off = geo.plane[a * 2 + e] + ((b * nI[a] + t1 // 2) * nJ[e] + f1 // 2) * C  # ea_conv_geo
                assert torch.equal(flat[off:off + C], x1[b, t1, f1]), (b, t1, f1)
    assert torch.equal(R.phase_unsplit(x1p, B, T1, F1, C), x1)
    assert torch.equal(R.phase_split(R.phase_unsplit(x1p, B, T1, F1, C), B, T1, F1, C), x1p)
    # the support bits: byte row*(C/8) + c/8, bit c & 7
    m = torch.rand(B, T1, F1, C, generator=torch.Generator().manual_seed(1)) < 0.4
    pos = R.pos_split(m, B, T1, F1, C)
    assert pos.dtype == torch.uint8 and pos.numel() == B * T1 * F1 * C // 8
    mp = R.phase_split(m, B, T1, F1, C)
    for row, c in ((0, 0), (0, 7), (B * T1 * F1 - 1, C - 1), (rows[0], 9 % C)):
        assert bool((int(pos[row * (C // 8) + c // 8]) >> (c & 7)) & 1) == bool(mp[row, c])
    assert torch.equal(R.pos_unsplit(pos, B, T1, F1, C), m)


def _layer_autograd(P, feats, gy, mask, pe):
    P = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    C = P["conv.0.weight"].shape[0]
    x = torch.relu(F.conv2d(feats.unsqueeze(1), P["conv.0.weight"], P["conv.0.bias"], stride=2))
    x = torch.relu(F.conv2d(x, P["conv.2.weight"], P["conv.2.bias"], stride=2))
    b, c, t, f = x.shape
    y = F.linear(x.transpose(1, 2).contiguous().view(b, t, c * f), P["out.0.weight"], P["out.0.bias"]) * math.sqrt(C)
    if pe is not None:
        y = y + pe[:t]
    if mask is not None:
        y = y * mask
    y.backward(gy)
    return y.detach(), {k: v.grad for k, v in P.items()}


@pytest.mark.parametrize("use_mask,use_pe", [(False, False), (True, False), (True, True), (False, True)])
def test_layer_restatement_with_mask_and_pe_matches_autograd(use_mask, use_pe):
    g = torch.Generator().manual_seed(3)
    idim, C, B, T = 11, 6, 2, 14
    F2 = R.down(R.down(idim))
    T2 = R.down(R.down(T))
    P = {"conv.0.weight": torch.randn(C, 1, 3, 3, generator=g, dtype=F64),
         "conv.0.bias": torch.randn(C, generator=g, dtype=F64),
         "conv.2.weight": torch.randn(C, C, 3, 3, generator=g, dtype=F64) / 3,
         "conv.2.bias": torch.randn(C, generator=g, dtype=F64),
         "out.0.weight": torch.randn(C, C * F2, generator=g, dtype=F64) / 3,
         "out.0.bias": torch.randn(C, generator=g, dtype=F64)}
    feats = torch.randn(B, T, idim, generator=g, dtype=F64)
    gy = torch.randn(B, T2, C, generator=g, dtype=F64)
    mask = (torch.rand(B, T2, C, generator=g) >= 0.3).to(F64) / 0.7 if use_mask else None
    pe = torch.randn(T2 + 3, C, generator=g, dtype=F64) if use_pe else None
    y, gr = R.subsampling_f64(P, feats, gy, False, mask=mask, pe=pe)
    y0, g0 = _layer_autograd(P, feats, gy, mask, pe)
    torch.testing.assert_close(y, y0, rtol=1e-12, atol=1e-12)
    for k in g0:
        torch.testing.assert_close(gr[k], g0[k], rtol=1e-11, atol=1e-11, msg=k)


@pytest.mark.parametrize("gid", sorted(R.GEOMETRIES))
def test_integer_grid_is_f32_exact(gid):
    """|v| < 2**24 for every input, exact intermediate and result of the geometry — and for the
    same sums over the inputs' magnitudes, which bound every partial sum in any order — with
    the integer prefill (|v| <= 3) the accumulating outputs start from."""
    c = R.conv_case(gid)
    c.check_exact(prefill=3)
    mags = c.magnitudes()
    print(gid, "max magnitude sums:", [float(m.max()) for m in mags])
    # the grid is not degenerate: results take many distinct values
    assert c.dw2.unique().numel() > 2 and c.dx1.unique().numel() > 2 and c.y2.unique().numel() > 2


def test_lo_half_case_needs_sixteen_bits():
    """The lo-half inputs k/16, |k| <= 4095: exact in f32, not in bf16, and exact as bf16 hi +
    bf16 lo."""
    x = R.lo_half_input((3, 7, 9), torch.Generator().manual_seed(0))
    assert bool(((x * 16) == (x * 16).round()).all()) and float(x.abs().max()) <= 4095 / 16
    hi = R.bf(x)
    lo = R.bf(x - hi)
    assert not torch.equal(hi, x)
    assert torch.equal(hi + lo, x)
    assert torch.equal(x.float().double(), x)
