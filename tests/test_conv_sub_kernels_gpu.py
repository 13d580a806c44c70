"""Conv2dSubsampling's kernels through the C ABI, bit-exact against float64.

Every entry point of the subsampling layer (the three gather modes of ea_gemm_conv, the fused
conv1 weight gradient ea_gemm_conv_w1 / _w1b / _w1b_all + ea_conv1_wgrad_reduce, ea_conv1_fwd2,
ea_conv1_wgrad, the im2col route's ea_im2col_conv1 / ea_im2col_conv2 / ea_col2im_conv2, and
ea_permute3) on integer-grid inputs (tests/subsampling_ref.py): every product and partial sum is
an integer below 2**24, so f32 accumulation is exact in any order and under any split-K, the
only rounding is the final bf16 store, and the comparison with the float64 restatement is
torch.equal.  An error confined to one edge row, one tap or one tile cannot hide in a norm.

The geometries (subsampling_ref.GEOMETRIES) are the smallest that reach each branch: T2 = F2 = 1,
even T1 / F1 (unequal parity planes, an x1 row / column no conv2 output reads), F2 = 4, 19, 33
and 63 (the weight-gradient gather's pixel cursor: dF = 0, the idim-80 value, and the dT = 0
branch above 32), class planes and P2 with partial row tiles, and C = 128, 512, 1024 (N inside
one 256-wide tile, two and four N tiles).  The gather GEMMs run under the default dispatch, with
the ping-pong kernel off (ea_gemm_set_pipe(0)) and, forward and input gradient, pinned to the
256 x 256 tiles the benched shapes take (on either kernel).
"""
import contextlib
import ctypes

import pytest
import torch

import subsampling_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF, F32T = torch.bfloat16, torch.float32
SENT = 768.0  # sentinel (bf16-exact)
GIDS = list(R.GEOMETRIES)
UNREAD = ("g_even", "g_f4", "g_f19e")


def _api():
    from espnet_amd._lib import BF16, CONV_DGRAD, CONV_FWD, CONV_WGRAD, F32, GEMM_PIPE, HipError
    from espnet_amd.layers.common import ACT_RELU, EPI_ACT, EPI_DACT, lib, ops
    from espnet_amd.layers.subsampling import phase_geo
    return dict(BF16=BF16, F32=F32, FWD=CONV_FWD, DGRAD=CONV_DGRAD, WGRAD=CONV_WGRAD, GEMM_PIPE=GEMM_PIPE,
                HipError=HipError, ACT_RELU=ACT_RELU, EPI_ACT=EPI_ACT, EPI_DACT=EPI_DACT, lib=lib, ops=ops,
                phase_geo=phase_geo)


@contextlib.contextmanager
def _dispatch(mode):
    """default / pipe0 (ping-pong kernel off) / tile256 (256 x 256 tiles pinned) / tile256_pipe0."""
    A = _api()
    try:
        if mode.endswith("pipe0"):
            A["lib"].ea_gemm_set_pipe(0)
        if mode.startswith("tile256"):
            A["lib"].ea_gemm_set_tile(256, 256)
        yield
        torch.cuda.synchronize()
    finally:
        A["lib"].ea_gemm_set_tile(0, 0)
        A["lib"].ea_gemm_set_pipe(A["GEMM_PIPE"])


def _dt(t):
    A = _api()
    return A["BF16"] if t.dtype == BF else A["F32"]


def _d(t, dtype):
    return t.to(dtype).contiguous().to(DEV)


def _filled(shape, dtype, value=SENT):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def _eq(got, want):
    """Bit-exact: the device result against the float64 reference cast to the result's type."""
    got = got.detach().cpu()
    return torch.equal(got, want.to(got.dtype))


class _Ops:
    """Device operands of one geometry, laid out as layers.subsampling lays them out."""

    def __init__(self, c):
        B, T1, F1, C = c.B, c.T1, c.F1, c.C
        self.c = c
        x1p = torch.zeros(c.P1 + 64, C, dtype=torch.float64)     # + 64 zero rows (wgrad gather padding)
        x1p[:c.P1] = R.phase_split(c.x1, B, T1, F1, C)
        self.x1p = _d(x1p, BF)
        self.pos = R.pos_split(c.x1 > 0, B, T1, F1, C).to(DEV)
        dx2 = torch.zeros(c.P2 + 128, C, dtype=torch.float64)    # + zero rows (K padding, off-grid taps)
        dx2[:c.P2] = c.dY2.reshape(c.P2, C)
        self.dx2 = _d(dx2, BF)
        w = c.W2.reshape(C, C, 9)
        self.w2p = _d(w.reshape(C, C // 64, 64, 9).permute(0, 1, 3, 2), BF)   # [Co][C/64][9][64]
        self.w2t = _d(w.permute(2, 0, 1), BF)                                  # [9][co][ci]
        self.w2k = _d(w.permute(1, 2, 0), BF)                                  # [ci][9][co]
        self.b2 = _d(c.b2, F32T)
        self.feats = _d(c.x, F32T)
        self.rows = R.plane_rows(B, T1, F1)
        self.tiles = sum((r + 255) // 256 for r in self.rows)


_OPS = {}


def _ops(gid):
    if gid not in _OPS:
        c = R.conv_case(gid)
        c.check_exact(prefill=3)  # the condition that makes torch.equal the right comparison
        _OPS[gid] = _Ops(c)
    return _OPS[gid]


def _unread_mask(c):
    """NHWC bool: pixels of an x1 row / column that no conv2 output reads."""
    m = torch.zeros(c.B, c.T1, c.F1, 1, dtype=torch.bool)
    if c.T1 % 2 == 0:
        m[:, -1] = True
    if c.F1 % 2 == 0:
        m[:, :, -1] = True
    return m.expand(c.B, c.T1, c.F1, c.C)


# ------------------------------------------------------------------------------ ea_gemm_conv
@pytest.mark.parametrize("mode", ["default", "pipe0", "tile256", "tile256_pipe0"])
@pytest.mark.parametrize("gid", GIDS)
def test_gemm_conv_fwd(gid, mode):
    A = _api()
    o = _ops(gid)
    c = o.c
    C = c.C
    geo, _, _, _ = A["phase_geo"](c.B, c.T1, c.F1, c.T2, c.F2, C, A["FWD"])
    out = _filled((c.P2 + 8, C), BF)
    epi = A["ops"].make_epi(A["EPI_ACT"], bias=o.b2, act=A["ACT_RELU"])
    ws = A["ops"].splitk_ws(DEV)
    with _dispatch(mode):
        A["lib"].ea_gemm_conv(ctypes.byref(geo), 1, 1, c.P2, C, 9 * C, o.x1p.data_ptr(), C, o.w2p.data_ptr(), 9 * C,
                              out.data_ptr(), A["BF16"], C, ctypes.byref(epi), ws.data_ptr(), ws.numel(),
                              A["ops"].stream())
    assert _eq(out[:c.P2], c.y2.reshape(c.P2, C))
    assert bool((out[c.P2:] == SENT).all())


@pytest.mark.parametrize("mode", ["default", "pipe0", "tile256", "tile256_pipe0"])
@pytest.mark.parametrize("gid", GIDS)
def test_gemm_conv_dgrad_classes(gid, mode):
    A = _api()
    o = _ops(gid)
    c = o.c
    C = c.C
    ws = A["ops"].splitk_ws(DEV)
    got = torch.zeros(c.P1, C, dtype=BF)
    with _dispatch(mode):
        for a in (0, 1):
            for e in (0, 1):
                geo, _, _, rows = A["phase_geo"](c.B, c.T1, c.F1, c.T2, c.F2, C, A["DGRAD"], a=a, e=e, zero=c.P2 * C)
                Mc = rows[a * 2 + e]
                ntaps = (1 if a else 2) * (1 if e else 2)
                r0 = geo.plane[a * 2 + e] // C
                aux = o.x1p[r0:r0 + Mc]
                out = _filled((Mc + 8, C), BF)
                epi = A["ops"].make_epi(A["EPI_DACT"], act=A["ACT_RELU"], aux=aux)
                A["lib"].ea_gemm_conv(ctypes.byref(geo), 1, 0, Mc, C, ntaps * C, o.dx2.data_ptr(), C,
                                      o.w2t.data_ptr(), C, out.data_ptr(), A["BF16"], C, ctypes.byref(epi),
                                      ws.data_ptr(), ws.numel(), A["ops"].stream())
                torch.cuda.synchronize()
                assert bool((out[Mc:] == SENT).all()), (a, e)
                got[r0:r0 + Mc] = out[:Mc].cpu()
    want = R.phase_split(R.bf(c.dx1), c.B, c.T1, c.F1, C)
    for k, (r0, n) in enumerate(zip([0, o.rows[0], o.rows[0] + o.rows[1], sum(o.rows[:3])], o.rows)):
        assert _eq(got[r0:r0 + n], want[r0:r0 + n]), ("class", k)
    if gid in UNREAD:
        m = R.phase_split(_unread_mask(c), c.B, c.T1, c.F1, C)
        assert bool(m.any()) and bool((got[m] == 0).all())
        assert bool((c.x1[_unread_mask(c)] > 0).any())  # zero by geometry, not by the ReLU mask


@pytest.mark.parametrize("ws_on", [True, False], ids=["splitk_ws", "no_ws"])
@pytest.mark.parametrize("mode", ["default", "pipe0"])
@pytest.mark.parametrize("gid", GIDS)
def test_gemm_conv_wgrad(gid, mode, ws_on):
    A = _api()
    o = _ops(gid)
    c = o.c
    C = c.C
    K2 = (c.P2 + 63) // 64 * 64
    geo, _, _, _ = A["phase_geo"](c.B, c.T1, c.F1, c.T2, c.F2, C, A["WGRAD"], zero=c.P1 * C)
    out = _filled((C + 1, 9 * C), F32T)
    epi = A["ops"].make_epi()
    ws = A["ops"].splitk_ws(DEV)
    with _dispatch(mode):
        A["lib"].ea_gemm_conv(ctypes.byref(geo), 0, 0, C, 9 * C, K2, o.dx2.data_ptr(), C, o.x1p.data_ptr(), C,
                              out.data_ptr(), A["F32"], 9 * C, ctypes.byref(epi), ws.data_ptr() if ws_on else 0,
                              ws.numel() if ws_on else 0, A["ops"].stream())
    assert _eq(out[:C], c.dw2.reshape(C, 9 * C))
    assert bool((out[C:] == SENT).all())


# ------------------------------------------------------------------------------ fused conv1 wgrad
def _prefill(C):
    g = torch.Generator().manual_seed(C)
    return R.int_grid((C, 9), (-3, -2, -1, 1, 2, 3), g), R.int_grid((C,), (-3, -2, -1, 1, 2, 3), g)


def _run_fused(o, variant, feats=None, kmajor=False):
    """The conv2 input gradient with the fused conv1 weight gradient (per class with the bf16
    mask rows, per class with the support bits, or the merged launch), then the reduce into
    prefilled dw / dbias.  -> (dw, dbias, part) on the host."""
    A = _api()
    c = o.c
    C = c.C
    lib, ops = A["lib"], A["ops"]
    feats = o.feats if feats is None else feats
    part = _filled(((o.tiles + 1) * 10 * C,), F32T)
    pw, pb = _prefill(C)
    dw, db = _d(pw, F32T), _d(pb, F32T)
    if variant == "all":
        geo, _, _, _ = A["phase_geo"](c.B, c.T1, c.F1, c.T2, c.F2, C, A["DGRAD"], zero=c.P2 * C)
        epi = ops.make_epi(A["EPI_DACT"], act=A["ACT_RELU"])
        w = o.w2k if kmajor else o.w2t
        lib.ea_gemm_conv_w1b_all(ctypes.byref(geo), C, o.dx2.data_ptr(), C, w.data_ptr(), 9 * C if kmajor else C,
                                 ctypes.byref(epi), feats.data_ptr(), c.T, c.Fin, part.data_ptr(), o.pos.data_ptr(),
                                 ops.stream())
    else:
        tile0 = 0
        for a in (0, 1):
            for e in (0, 1):
                geo, _, _, rows = A["phase_geo"](c.B, c.T1, c.F1, c.T2, c.F2, C, A["DGRAD"], a=a, e=e, zero=c.P2 * C)
                Mc = rows[a * 2 + e]
                ntaps = (1 if a else 2) * (1 if e else 2)
                r0 = geo.plane[a * 2 + e] // C
                pp = part.data_ptr() + 4 * tile0 * 10 * C
                if variant == "w1":
                    epi = ops.make_epi(A["EPI_DACT"], act=A["ACT_RELU"], aux=o.x1p[r0:r0 + Mc])
                    lib.ea_gemm_conv_w1(ctypes.byref(geo), Mc, C, ntaps * C, o.dx2.data_ptr(), C, o.w2t.data_ptr(), C,
                                        ctypes.byref(epi), feats.data_ptr(), c.T, c.Fin, pp, ops.stream())
                else:
                    epi = ops.make_epi(A["EPI_DACT"], act=A["ACT_RELU"])
                    lib.ea_gemm_conv_w1b(ctypes.byref(geo), Mc, C, ntaps * C, o.dx2.data_ptr(), C, o.w2t.data_ptr(),
                                         C, ctypes.byref(epi), feats.data_ptr(), c.T, c.Fin, pp,
                                         o.pos.data_ptr() + r0 * (C // 8), ops.stream())
                tile0 += (Mc + 255) // 256
        assert tile0 == o.tiles
    lib.ea_conv1_wgrad_reduce(o.tiles, C, part.data_ptr(), dw.data_ptr(), db.data_ptr(), ops.stream())
    torch.cuda.synchronize()
    return dw.cpu(), db.cpu(), part.cpu()


FUSED = [("w1", False), ("w1b", False), ("all", False), ("all", True)]
FUSED_IDS = ["w1", "w1b", "w1b_all_w2t", "w1b_all_w2k"]


@pytest.mark.parametrize("variant,kmajor", FUSED, ids=FUSED_IDS)
@pytest.mark.parametrize("gid", GIDS)
def test_fused_conv1_wgrad_exact(gid, variant, kmajor):
    o = _ops(gid)
    c = o.c
    dw, db, part = _run_fused(o, variant, kmajor=kmajor)
    pw, pb = _prefill(c.C)
    assert torch.equal(dw.double(), pw + c.dw1)       # the prefill survives as an addend
    assert torch.equal(db.double(), pb + c.db1)
    assert bool((part[o.tiles * 10 * c.C:] == SENT).all())


@pytest.mark.parametrize("variant,kmajor", FUSED[:3], ids=FUSED_IDS[:3])
def test_fused_conv1_wgrad_refused_without_pipe_kernel(variant, kmajor):
    """The fused epilogue lives in the ping-pong kernel: with it off every fused entry returns
    an error before any launch (no quiet fall-back)."""
    A = _api()
    o = _ops("g_even")
    with _dispatch("pipe0"):
        with pytest.raises(A["HipError"]):
            _run_fused(o, variant, kmajor=kmajor)


def test_fused_conv1_wgrad_lo_half():
    """The f32 conv1 input patches enter the MFMA as bf16 hi + lo: inputs k/16, |k| <= 4095 need
    both halves.  Bound 1e-4 relative L2 against float64: the f32 accumulation of at most 390
    terms (the largest class plane of g_rows, 330 rows, in tiles of 256) is bounded by 390 * 2**-24
    ~ 2.3e-5; a missing lo half costs ~2**-9 ~ 2e-3."""
    B, T1, F1, C = R.GEOMETRIES["g_rows"]
    c = R.ConvCase(B, T1, F1, C, seed=101, lo_half=True)
    o = _Ops(c)
    dw, db, _ = _run_fused(o, "all")
    pw, pb = _prefill(C)
    e_w = float(((dw.double() - pw) - c.dw1).norm() / c.dw1.norm())
    hi_only = R.conv1_wgrad_ref(R.bf(c.x), c.g)[0]
    print(f"lo half: dw rel L2 {e_w:.2e} (hi half alone would be {float((hi_only - c.dw1).norm() / c.dw1.norm()):.2e})")
    assert e_w <= 1e-4, e_w
    assert torch.equal(db.double(), pb + c.db1)  # the bias column multiplies by 1: still exact


# ------------------------------------------------------------------------------ ea_conv1_fwd2
def _conv1_inputs(B, T1, F1, C, seed):
    g = torch.Generator().manual_seed(seed)
    T = 2 * T1 + 1 + (T1 % 2 == 0)      # even T1: one more input frame, seen by no window
    Fin = 2 * F1 + 1 + (F1 % 2 == 1)    # odd F1: one more input bin, seen by no window
    x = R.int_grid((B, T, Fin), range(-2, 3), g)
    w1 = R.int_grid((C, 9), (-1, 0, 1), g)
    b1 = R.int_grid((C,), (-1, 0, 1), g)
    return x, w1, b1


@pytest.mark.parametrize("B,T1,F1", [(1, 3, 3), (2, 4, 6), (3, 5, 7), (2, 3, 2)])
@pytest.mark.parametrize("C", [8, 64, 128, 512, 1024, 2048])
def test_conv1_fwd2(C, B, T1, F1):
    A = _api()
    x, w1, b1 = _conv1_inputs(B, T1, F1, C, C + T1)
    assert R.down(x.shape[1]) == T1 and R.down(x.shape[2]) == F1
    want = R.conv1_fwd_ref(x, w1, b1)
    R.assert_f32_exact(x, w1, b1, want, R.conv1_fwd_ref(x.abs(), w1.abs(), b1.abs()))
    P1 = B * T1 * F1
    xd, wd, bd = _d(x, F32T), _d(w1, F32T), _d(b1, F32T)
    for dtype in (BF, F32T):
        x1p = _filled((P1 + 64, C), dtype)
        pos = _filled((P1 * C // 8 + 16,), torch.uint8, 0xAA)
        A["lib"].ea_conv1_fwd2(B, x.shape[1], x.shape[2], C, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                               x1p.data_ptr(), _dt(x1p), pos.data_ptr(), A["ops"].stream())
        x1q = _filled((P1 + 64, C), dtype)
        A["lib"].ea_conv1_fwd2(B, x.shape[1], x.shape[2], C, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                               x1q.data_ptr(), _dt(x1q), 0, A["ops"].stream())
        torch.cuda.synchronize()
        got = x1p.cpu()
        assert _eq(R.phase_unsplit(got[:P1], B, T1, F1, C), want), dtype
        assert bool((got[P1:] == SENT).all()), dtype            # the 64 guard rows
        assert torch.equal(x1q.cpu(), got), dtype               # pos = NULL: the same x1p
        assert torch.equal(pos[:P1 * C // 8].cpu(), R.pack_bits(got[:P1].float() > 0)), dtype
        assert bool((pos[P1 * C // 8:] == 0xAA).all()), dtype


# ------------------------------------------------------------------------------ ea_conv1_wgrad
@pytest.mark.parametrize("dh_dtype", [BF, F32T], ids=["bf16", "f32"])
@pytest.mark.parametrize("C", [8, 64, 512])
def test_conv1_wgrad(C, dh_dtype):
    A = _api()
    B, T1, F1 = 4, 20, 27       # 2,160 pixels: 1, 5 and 34 blocks at C = 8, 64, 512
    x, _, _ = _conv1_inputs(B, T1, F1, C, 5)
    g = torch.Generator().manual_seed(C)
    dh = R.int_grid((B, T1, F1, C), range(-2, 3), g)
    dw_ref, db_ref = R.conv1_wgrad_ref(x, dh)
    R.assert_f32_exact(dw_ref, db_ref, *[3 + 2 * v for v in R.conv1_wgrad_ref(x.abs(), dh.abs())])
    xd = _d(x, F32T)
    dhp = _d(R.phase_split(dh, B, T1, F1, C), dh_dtype)
    ws = torch.zeros(1024 * 10 * C, dtype=F32T, device=DEV)
    pw, pb = _prefill(C)
    for ws_elems in (10 * C, ws.numel()):   # one block; every block the grid wants
        dw, db = _d(pw, F32T), _d(pb, F32T)
        for n in (1, 2):                    # accumulating
            A["lib"].ea_conv1_wgrad(B, x.shape[1], x.shape[2], C, xd.data_ptr(), dhp.data_ptr(), _dt(dhp),
                                    dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws_elems, A["ops"].stream())
            torch.cuda.synchronize()
            assert torch.equal(dw.cpu().double(), pw + n * dw_ref), (ws_elems, n)
            assert torch.equal(db.cpu().double(), pb + n * db_ref), (ws_elems, n)
    dw, db = _d(pw, F32T), _d(pb, F32T)
    with pytest.raises(A["HipError"]):      # no room for one block's partials
        A["lib"].ea_conv1_wgrad(B, x.shape[1], x.shape[2], C, xd.data_ptr(), dhp.data_ptr(), _dt(dhp),
                                dw.data_ptr(), db.data_ptr(), ws.data_ptr(), 10 * C - 1, A["ops"].stream())
    torch.cuda.synchronize()
    assert torch.equal(dw.cpu().double(), pw) and torch.equal(db.cpu().double(), pb)


# ------------------------------------------------------------------------------ im2col route
@pytest.mark.parametrize("dtype", [BF, F32T], ids=["bf16", "f32"])
@pytest.mark.parametrize("gid", ["g_even", "g_f19e"])
def test_im2col_conv1(gid, dtype):
    A = _api()
    c = R.conv_case(gid)
    col = _filled((c.P1, 16), dtype)
    xd = _d(c.x, F32T)
    A["lib"].ea_im2col_conv1(c.B, c.T, c.Fin, xd.data_ptr(), col.data_ptr(), _dt(col), A["ops"].stream())
    torch.cuda.synchronize()
    assert _eq(col, R.im2col_conv1_ref(c.x))
    assert bool((col[:, 9:] == 0).all())


@pytest.mark.parametrize("dtype", [BF, F32T], ids=["bf16", "f32"])
@pytest.mark.parametrize("gid", ["g_even", "g_f19e"])
def test_im2col_conv2(gid, dtype):
    A = _api()
    c = R.conv_case(gid)
    x1 = _d(c.x1, dtype)
    col = _filled((c.P2 + 1, 9 * c.C), dtype)
    A["lib"].ea_im2col_conv2(c.B, c.T1, c.F1, c.C, x1.data_ptr(), col.data_ptr(), _dt(col), A["ops"].stream())
    torch.cuda.synchronize()
    assert _eq(col[:c.P2], R.im2col_conv2_ref(c.x1))
    assert bool((col[c.P2:] == SENT).all())


@pytest.mark.parametrize("C,dcol_dtype,dtype", [(64, BF, BF), (64, BF, F32T), (64, F32T, BF), (64, F32T, F32T),
                                                (4, F32T, F32T), (4, BF, BF)],
                         ids=["c64_bf16x8", "c64_bf16_f32", "c64_f32_bf16", "c64_f32_f32", "c4_f32", "c4_bf16"])
@pytest.mark.parametrize("gid", ["g_even", "g_f19e"])
def test_col2im_conv2(gid, C, dcol_dtype, dtype):
    A = _api()
    c = R.conv_case(gid)
    g = torch.Generator().manual_seed(C)
    x1 = c.x1[..., :C].contiguous()
    dcol = R.int_grid((c.P2, 9 * C), (-1, 0, 1), g)
    want = R.col2im_conv2_ref(dcol, x1)
    x1d, dcd = _d(x1, dtype), _d(dcol, dcol_dtype)
    dx1 = _filled((c.P1 + 1, C), dtype)
    A["lib"].ea_col2im_conv2(c.B, c.T1, c.F1, C, dcd.data_ptr(), _dt(dcd), x1d.data_ptr(), dx1.data_ptr(), _dt(dx1),
                             A["ops"].stream())
    torch.cuda.synchronize()
    got = dx1[:c.P1].cpu().reshape(c.B, c.T1, c.F1, C)
    assert _eq(got, want)
    assert bool((dx1[c.P1:] == SENT).all())
    m = _unread_mask(c)[..., :C]
    assert bool(m.any()) and bool((got[m] == 0).all()) and bool((x1[m] > 0).any())
    assert bool((want[:, :c.T1 - 1 - (c.T1 % 2 == 0)] != 0).any())


# ------------------------------------------------------------------------------ ea_permute3
@pytest.mark.parametrize("src_dtype,dst_dtype", [(F32T, BF), (BF, F32T), (F32T, F32T)],
                         ids=["f32_bf16", "bf16_f32", "f32_f32"])
@pytest.mark.parametrize("A_,Bd,Cd", [(1, 3, 5), (7, 9, 64), (64, 64, 9)])
def test_permute3(A_, Bd, Cd, src_dtype, dst_dtype):
    A = _api()
    g = torch.Generator().manual_seed(A_ * 100 + Bd)
    src = R.int_grid((A_, Bd, Cd), range(-8, 9), g)
    pre = R.int_grid((A_, Cd, Bd), range(-8, 9), g)
    want = src.permute(0, 2, 1)
    sd = _d(src, src_dtype)
    n = A_ * Bd * Cd
    for acc in (0, 1):
        dst = _filled((n + 8,), dst_dtype)
        dst[:n] = _d(pre.reshape(-1), dst_dtype)
        A["lib"].ea_permute3(A_, Bd, Cd, sd.data_ptr(), _dt(sd), dst.data_ptr(), _dt(dst), acc, A["ops"].stream())
        torch.cuda.synchronize()
        assert _eq(dst[:n].reshape(A_, Cd, Bd), want + pre if acc else want), acc
        assert bool((dst[n:] == SENT).all())
