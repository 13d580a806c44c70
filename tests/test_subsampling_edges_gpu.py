"""Conv2dSubsampling, forward + backward, at the geometry edges, against float64.

The layer is driven as test_subsampling_gpu._run drives it (seeded randn input, every parameter
gradient), at shapes (idim, C, B, T) chosen for the index arithmetic they reach: T2 = F2 = 1,
even T1 and even F1 (an x1 row / column no conv2 output reads), F2 = 20, 19 with F1 even, 63
(idim 257: the weight-gradient gather's F2 > 32 branch), C = 128, 1024 and 2048 on the implicit
route, and C = 96, which falls to the im2col route in bf16.

bf16 runs (the implicit route where _implicit_ok allows it, and the im2col route, forced on the
implicit-capable shapes) are compared with the float64 restatement that rounds to bf16 where
that route stores bf16 (subsampling_ref.subsampling_f64); fp32 runs with plain float64.  Every
(b, t2) output row and every gradient tensor is checked in relative L2.

Bounds.  bf16: the project's values for this comparison (test_benched_shapes_gpu.py), 1e-3 on
the output and the Linear's gradients, 3e-3 on the conv gradients; fp32: 2e-5, the project's
fp32 value.  Small shapes average over fewer pixels, so each is max(that value, 4 x the floor
of the reference itself): the distance between the restatement in float64 and the same
restatement evaluated in f32 torch CPU arithmetic at this input (4 x is the margin
test_benched_shapes_gpu.py gives an fp32 floor).  The bound is computed in the test from the
references alone and printed with the HIP deviation; a HIP deviation never sets a bound.

Further cases: output gradients confined to the first and last t2 of the last utterance (conv
gradients from edge pixels alone), 3e4 in every input frame / bin that only an unread x1 row /
column or no conv1 window sees (a leaked edge gradient would be scaled by 3e4), and dropout
p = 0.1 through the layer on both routes and with the absolute PositionalEncoding: the mask
recovered from the output's exact zeros must be the one the backward undoes.

Measured on MI355X
  (columns: HIP deviation / reference floor / bound, for the worst output row and for the gradient
  tensor closest to its bound; the floor in the gradient column is the largest over the tensors)
  i80_c64_b2_t7    bf16                 y 2.4e-04 / 2.3e-06 / 1e-03;  grad 2.1e-04 (out.0.weight) / 1.7e-06 / 1e-03
  i80_c64_b2_t7    bf16_im2col          y 7.7e-08 / 9.5e-08 / 1e-03;  grad 6.4e-08 (conv.0.weight) / 5.5e-08 / 3e-03
  i80_c64_b2_t7    fp32                 y 3.8e-07 / 2.9e-07 / 2e-05;  grad 3.3e-07 (out.0.weight) / 2.4e-07 / 2e-05
  i83_c64_b3_t62   bf16                 y 4.7e-04 / 4.7e-04 / 2e-03;  grad 7.1e-05 (out.0.weight) / 7.1e-05 / 1e-03
  i83_c64_b3_t62   bf16_im2col          y 3.2e-04 / 8.3e-05 / 1e-03;  grad 5.1e-05 (out.0.weight) / 1.2e-05 / 1e-03
  i83_c64_b3_t62   fp32                 y 4.8e-07 / 4.1e-07 / 2e-05;  grad 3.5e-07 (conv.2.weight) / 4.9e-07 / 2e-05
  i81_c128_b2_t33  bf16                 y 1.4e-05 / 1.4e-05 / 1e-03;  grad 1.4e-05 (conv.0.weight) / 1.3e-05 / 3e-03
  i81_c128_b2_t33  bf16_im2col          y 1.5e-06 / 7.6e-07 / 1e-03;  grad 1.2e-05 (conv.0.bias) / 1.5e-05 / 3e-03
  i81_c128_b2_t33  fp32                 y 2.8e-07 / 3.3e-07 / 2e-05;  grad 3.2e-07 (conv.0.weight) / 4.3e-07 / 2e-05
  i257_c64_b1_t23  bf16                 y 3.5e-07 / 3.5e-07 / 1e-03;  grad 2.6e-06 (conv.0.weight) / 1.1e-06 / 3e-03
  i257_c64_b1_t23  bf16_im2col          y 1.3e-07 / 1.4e-07 / 1e-03;  grad 7.9e-08 (conv.0.weight) / 8.7e-08 / 3e-03
  i257_c64_b1_t23  fp32                 y 3.9e-07 / 4.2e-07 / 2e-05;  grad 3.3e-07 (out.0.weight) / 3.1e-07 / 2e-05
  i7_c64_b2_t9     bf16                 y 3.8e-08 / 3.7e-08 / 1e-03;  grad 2.8e-06 (conv.0.weight) / 5.1e-08 / 3e-03
  i7_c64_b2_t9     bf16_im2col          y 3.3e-08 / 3.7e-08 / 1e-03;  grad 1.9e-08 (conv.0.weight) / 2.0e-08 / 3e-03
  i7_c64_b2_t9     fp32                 y 2.4e-07 / 1.3e-07 / 2e-05;  grad 2.3e-07 (out.0.weight) / 2.0e-07 / 2e-05
  i23_c1024_b2_t15 bf16                 y 3.2e-04 / 2.8e-04 / 1e-03;  grad 1.8e-04 (out.0.weight) / 1.2e-04 / 1e-03
  i23_c1024_b2_t15 bf16_im2col          y 3.3e-05 / 9.8e-06 / 1e-03;  grad 1.6e-05 (out.0.weight) / 1.8e-05 / 1e-03
  i23_c1024_b2_t15 fp32                 y 4.0e-07 / 5.0e-07 / 2e-05;  grad 3.2e-07 (conv.0.weight) / 6.6e-07 / 2e-05
  i23_c2048_b1_t11 bf16                 y 1.8e-07 / 2.6e-07 / 1e-03;  grad 5.5e-05 (conv.0.bias) / 3.7e-05 / 3e-03
  i23_c2048_b1_t11 bf16_im2col          y 9.1e-05 / 9.1e-05 / 1e-03;  grad 6.8e-05 (out.0.weight) / 6.8e-05 / 1e-03
  i23_c2048_b1_t11 fp32                 y 5.6e-07 / 6.8e-07 / 2e-05;  grad 6.9e-07 (conv.0.bias) / 1.2e-06 / 2e-05
  i80_c96_b2_t31   bf16                 y 1.0e-07 / 7.3e-05 / 1e-03;  grad 8.3e-08 (conv.0.weight) / 1.7e-05 / 3e-03
  i80_c96_b2_t31   fp32                 y 4.8e-07 / 3.3e-07 / 2e-05;  grad 3.8e-07 (out.0.weight) / 4.1e-07 / 2e-05
  i83_c64_b3_t62   bf16 edge-gy         y 4.7e-04 / 4.7e-04 / 2e-03;  grad 2.2e-06 (conv.0.weight) / 1.4e-07 / 3e-03
  i83_c64_b3_t62   bf16_im2col edge-gy  y 3.2e-04 / 8.3e-05 / 1e-03;  grad 4.9e-08 (conv.0.weight) / 5.4e-08 / 3e-03
  i83_c64_b3_t62   fp32 edge-gy         y 4.8e-07 / 4.1e-07 / 2e-05;  grad 2.9e-07 (out.0.weight) / 2.5e-07 / 2e-05
  i81_c128_b2_t33  bf16 edge-gy         y 1.4e-05 / 1.4e-05 / 1e-03;  grad 2.4e-06 (conv.0.weight) / 9.9e-06 / 3e-03
  i81_c128_b2_t33  bf16_im2col edge-gy  y 1.5e-06 / 7.6e-07 / 1e-03;  grad 5.0e-08 (conv.0.weight) / 6.6e-08 / 3e-03
  i81_c128_b2_t33  fp32 edge-gy         y 2.8e-07 / 3.3e-07 / 2e-05;  grad 3.0e-07 (conv.0.weight) / 3.3e-07 / 2e-05
  i80_c64_b2_t7    bf16 unread          y 2.4e-04 / 2.3e-06 / 1e-03;  grad 2.1e-04 (out.0.weight) / 1.7e-06 / 1e-03
  i80_c64_b2_t7    fp32 unread          y 3.8e-07 / 2.9e-07 / 2e-05;  grad 3.3e-07 (out.0.weight) / 2.4e-07 / 2e-05
  i83_c64_b3_t62   bf16 unread          y 4.7e-04 / 4.7e-04 / 2e-03;  grad 7.1e-05 (out.0.weight) / 7.1e-05 / 1e-03
  i83_c64_b3_t62   fp32 unread          y 4.8e-07 / 4.1e-07 / 2e-05;  grad 3.5e-07 (conv.2.weight) / 4.9e-07 / 2e-05
  i81_c128_b2_t33  bf16 unread          y 1.4e-05 / 1.4e-05 / 1e-03;  grad 1.4e-05 (conv.0.weight) / 1.3e-05 / 3e-03
  i81_c128_b2_t33  fp32 unread          y 2.8e-07 / 3.3e-07 / 2e-05;  grad 3.2e-07 (conv.0.weight) / 4.3e-07 / 2e-05
  i257_c64_b1_t23  bf16 unread          y 3.5e-07 / 3.5e-07 / 1e-03;  grad 2.6e-06 (conv.0.weight) / 1.1e-06 / 3e-03
  i257_c64_b1_t23  fp32 unread          y 3.9e-07 / 4.2e-07 / 2e-05;  grad 3.3e-07 (out.0.weight) / 3.1e-07 / 2e-05
  i7_c64_b2_t9     bf16 unread          y 3.8e-08 / 3.7e-08 / 1e-03;  grad 2.8e-06 (conv.0.weight) / 5.1e-08 / 3e-03
  i7_c64_b2_t9     fp32 unread          y 2.4e-07 / 1.3e-07 / 2e-05;  grad 2.3e-07 (out.0.weight) / 2.0e-07 / 2e-05
  i80_c96_b2_t31   bf16 unread          y 1.0e-07 / 7.3e-05 / 1e-03;  grad 8.3e-08 (conv.0.weight) / 1.7e-05 / 3e-03
  i80_c96_b2_t31   fp32 unread          y 4.8e-07 / 3.3e-07 / 2e-05;  grad 3.8e-07 (out.0.weight) / 4.1e-07 / 2e-05
  i83_c64_b3_t62   bf16 p=0.1           y 4.7e-04 / 4.7e-04 / 2e-03;  grad 7.1e-05 (out.0.weight) / 7.1e-05 / 1e-03
  i83_c64_b3_t62   bf16_im2col p=0.1    y 3.2e-04 / 8.3e-05 / 1e-03;  grad 4.8e-05 (out.0.weight) / 1.8e-05 / 1e-03
  i83_c64_b3_t62   fp32 p=0.1           y 5.0e-07 / 4.4e-07 / 2e-05;  grad 3.5e-07 (conv.2.weight) / 4.6e-07 / 2e-05
  i83_c64_b3_t62   fp32 p=0.1 abs-PE    y 3.7e-07 / 2.5e-07 / 2e-05;  grad 3.5e-07 (conv.2.weight) / 4.6e-07 / 2e-05
  dropout: 294 of 2,688 entries dropped on every route (expected 269 +- 15.6)
"""
import math

import pytest
import torch

import subsampling_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF, F32T, F64 = torch.bfloat16, torch.float32, torch.float64

# (idim, C, B, T)
SHAPES = [(80, 64, 2, 7), (83, 64, 3, 62), (81, 128, 2, 33), (257, 64, 1, 23), (7, 64, 2, 9), (23, 1024, 2, 15),
          (23, 2048, 1, 11), (80, 96, 2, 31)]
P_DROP = 0.1


def _sid(s):
    return "i%d_c%d_b%d_t%d" % s


def _implicit_capable(C):
    return C % 64 == 0 and 256 % (C // 8) == 0


VARIANTS = [(s, v) for s in SHAPES for v in ("bf16", "bf16_im2col", "fp32")
            if v != "bf16_im2col" or _implicit_capable(s[1])]


def _rel(a, b):
    a, b = a.double(), b.double()
    den = float(b.norm())
    return float((a - b).norm()) / den if den > 0 else float((a - b).norm())


def _row_rel(a, b):
    """max over (b, t2) rows of the relative L2 deviation."""
    a, b = a.double().reshape(-1, a.shape[-1]), b.double().reshape(-1, b.shape[-1])
    den = b.norm(dim=1)
    num = (a - b).norm(dim=1)
    return float(torch.where(den > 0, num / den.clamp_min(1e-300), num).max())


def _geom(shape):
    idim, C, B, T = shape
    T1, F1 = R.down(T), R.down(idim)
    return T1, F1, R.down(T1), R.down(F1)


def _inputs(shape, kind="plain"):
    """Seeded input and output gradient.  kind: plain / edge (gy only at the first and last t2 of
    the last utterance) / unread (3e4 where no read conv1 output looks)."""
    idim, C, B, T = shape
    T1, F1, T2, F2 = _geom(shape)
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(B, T, idim, generator=g)
    gy = torch.randn(B, T2, C, generator=g)
    if kind == "edge":
        keep = torch.zeros(B, T2, 1)
        keep[B - 1, 0] = keep[B - 1, T2 - 1] = 1.0
        gy = gy * keep
    if kind == "unread":
        # x1 row T1-1 (unread when T1 is even) alone sees frames 2*T1-1 and 2*T1; frames from
        # 2*T1+1 on are under no conv1 window; bins likewise
        feats[:, (2 * T1 - 1 if T1 % 2 == 0 else 2 * T1 + 1):] = 3e4
        feats[:, :, (2 * F1 - 1 if F1 % 2 == 0 else 2 * F1 + 1):] = 3e4
    return feats, gy


def _has_unread(shape):
    idim, C, B, T = shape
    T1, F1, _, _ = _geom(shape)
    return T1 % 2 == 0 or F1 % 2 == 0 or T > 2 * T1 + 1 or idim > 2 * F1 + 1


def _hip(shape, variant, feats, gy, p=0.0, seed=0, absolute=False):
    """One forward + backward of the layer.  -> (y, {param: grad}, {param: value}) on the host."""
    from espnet_amd.arena import ParamArena
    from espnet_amd.layers import subsampling as S
    from espnet_amd.layers.decoder import PositionalEncoding
    idim, C, B, T = shape
    cd = F32T if variant == "fp32" else BF
    torch.manual_seed(0)
    sub = S.Conv2dSubsampling(idim, C, p, PositionalEncoding(C, p) if absolute else None)
    P = {k: v.detach().double().clone() for k, v in sub.named_parameters()}
    arena = ParamArena(sub, DEV, [], shadow_dtype=cd)
    sub.bind(arena, "", cd)
    sub._anchor = torch.zeros(1, device=DEV, requires_grad=True)
    sub.train()
    old = S._implicit_ok
    if variant == "bf16_im2col":
        S._implicit_ok = lambda cd_, C_: False
    try:
        assert S._implicit_ok(cd, C) == (variant == "bf16" and _implicit_capable(C))
        y = sub(feats.to(DEV), seed)
        y.backward(gy.to(DEV))
    finally:
        S._implicit_ok = old
    torch.cuda.synchronize()
    grads = {k: v.grad.detach().double().cpu() for k, v in sub.named_parameters()}
    return y.detach().double().cpu(), grads, P


def _route(shape, variant):
    return "implicit" if variant == "bf16" and _implicit_capable(shape[1]) else "im2col"


def _refs(P, feats, gy, shape, variant, mask=None, pe=None):
    """The restatement in float64 and, for the floor, in f32."""
    torch.set_num_threads(16)
    em = variant != "fp32"
    with torch.no_grad():
        r64 = R.subsampling_f64(P, feats.double(), gy.double(), em, mask=mask, pe=pe, route=_route(shape, variant))
        r32 = R.subsampling_f64(P, feats.double(), gy.double(), em, mask=mask, pe=pe, route=_route(shape, variant),
                                dt=F32T)
    return r64, r32


def _project_bound(variant, k):
    if variant == "fp32":
        return 2e-5
    return 3e-3 if k.startswith("conv.") else 1e-3


def _check(tag, variant, y, grads, r64, r32):
    y64, g64 = r64
    y32, g32 = r32
    rows = [("y rows", _row_rel(y, y64), _row_rel(y32, y64), _project_bound(variant, "y"))]
    for k in g64:
        rows.append((k, _rel(grads[k], g64[k]), _rel(g32[k], g64[k]), _project_bound(variant, k)))
    bad = []
    for k, e, floor, proj in rows:
        bound = max(proj, 4.0 * floor)
        print(f"EDGE {tag} {k}: hip {e:.2e} floor {floor:.2e} bound {bound:.2e}")
        if not e <= bound:
            bad.append((k, e, bound))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("shape,variant", VARIANTS, ids=[f"{_sid(s)}-{v}" for s, v in VARIANTS])
def test_layer_vs_float64(shape, variant):
    feats, gy = _inputs(shape)
    y, grads, P = _hip(shape, variant, feats, gy)
    _check(f"{_sid(shape)} {variant}", variant, y, grads, *_refs(P, feats, gy, shape, variant))


@pytest.mark.parametrize("variant", ["bf16", "bf16_im2col", "fp32"])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]], ids=_sid)
def test_edge_only_gradients(shape, variant):
    feats, gy = _inputs(shape, "edge")
    y, grads, P = _hip(shape, variant, feats, gy)
    _check(f"{_sid(shape)} {variant} edge-gy", variant, y, grads, *_refs(P, feats, gy, shape, variant))


@pytest.mark.parametrize("variant", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", [s for s in SHAPES if _has_unread(s)], ids=_sid)
def test_unread_input_does_not_leak(shape, variant):
    feats, gy = _inputs(shape, "unread")
    assert float(feats.max()) == 3e4
    y, grads, P = _hip(shape, variant, feats, gy)
    # the reference's read pixels do not see the 3e4 either: same output as on the plain input
    _check(f"{_sid(shape)} {variant} unread-3e4", variant, y, grads, *_refs(P, feats, gy, shape, variant))


# ------------------------------------------------------------------------------ dropout
DROP_SHAPE = SHAPES[1]
DROP_CASES = [("bf16", False), ("bf16_im2col", False), ("fp32", False), ("fp32", True)]


@pytest.mark.parametrize("variant,absolute", DROP_CASES, ids=["bf16", "bf16_im2col", "fp32", "fp32_abs_pe"])
def test_dropout_mask_through_the_layer(variant, absolute):
    from espnet_amd.layers.decoder import sinusoid_table
    shape = DROP_SHAPE
    idim, C, B, T = shape
    T2 = _geom(shape)[2]
    feats, gy = _inputs(shape)
    y, grads, P = _hip(shape, variant, feats, gy, p=P_DROP, seed=1234, absolute=absolute)
    keep = y != 0
    n = keep.numel()
    dropped = n - int(keep.sum())
    sd = math.sqrt(n * P_DROP * (1 - P_DROP))
    print(f"EDGE dropout {variant} abs={absolute}: dropped {dropped} of {n} (expected {n * P_DROP:.0f} +- {sd:.1f})")
    assert abs(dropped - n * P_DROP) <= 5 * sd
    mask = keep.double() / (1.0 - P_DROP)
    pe = sinusoid_table(T2, C).double() if absolute else None
    # kept entries = reference / (1 - p), and every gradient = the restatement run with that mask
    _check(f"{_sid(shape)} {variant} dropout abs={absolute}", variant, y, grads,
           *_refs(P, feats, gy, shape, variant, mask=mask, pe=pe))
    y_same, _, _ = _hip(shape, variant, feats, gy, p=P_DROP, seed=1234, absolute=absolute)
    assert torch.equal(y_same != 0, keep)
    y_other, _, _ = _hip(shape, variant, feats, gy, p=P_DROP, seed=1235, absolute=absolute)
    assert not torch.equal(y_other != 0, keep)


@pytest.mark.parametrize("rows,d,L", [(1, 8, 1), (1, 8, 3), (37, 256, 37), (37, 256, 5)])
def test_add_pe_dropout_alone(rows, d, L):
    from espnet_amd._lib import F32
    from espnet_amd.layers.common import lib, ops
    g = torch.Generator().manual_seed(rows + L)
    y0 = torch.randn(rows, d, generator=g)
    pe = torch.randn(L, d, generator=g)
    idx = torch.arange(rows) % L
    ped = pe.to(DEV)
    y = y0.to(DEV)
    lib.ea_add_pe_dropout(rows, d, L, ped.data_ptr(), 0.0, 7, y.data_ptr(), ops.stream())
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), (y0.double() + pe[idx].double()).float())  # one f32 add, rounded once
    # p > 0: the zero set is ea_scale_dropout's at the same seed and shape (index r*d + c)
    y = (y0.abs() + 1.0).to(DEV)            # y + pe != 0 wherever kept
    pe1 = torch.ones(L, d, device=DEV)
    lib.ea_add_pe_dropout(rows, d, L, pe1.data_ptr(), 0.5, 99, y.data_ptr(), ops.stream())
    ones = torch.ones(rows, d, device=DEV)
    z = torch.empty(rows, d, device=DEV)
    lib.ea_scale_dropout(rows, d, ones.data_ptr(), F32, d, z.data_ptr(), F32, d, 1.0, 0.5, 99, ops.stream())
    torch.cuda.synchronize()
    assert torch.equal(y.cpu() == 0, z.cpu() == 0)
    kept = z.cpu() != 0
    assert torch.equal(y.cpu()[kept], (((y0.abs() + 1.0) + 1.0) * 2.0)[kept])  # (y + pe) / (1 - p), in f32
    if rows * d >= 1024:
        assert 0.4 < float((z == 0).float().mean()) < 0.6
