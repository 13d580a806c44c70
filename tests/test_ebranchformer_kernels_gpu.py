"""E-Branchformer kernels on the C-ABI (csrc/ebranchformer.hip): the CSGU row statistics, the
CSGU forward and backward (exact GELU + gate LayerNorm + depthwise conv + gating + dropout) and
the merge convolution forward and backward, each against float64 torch evaluated here from the
same bf16-rounded inputs, in both compute dtypes.

Tolerances are those of tests/test_conv_module_gpu.py for the same kinds of quantity (f32 tap
sums over bf16-valued inputs): outputs atol 1e-4 / rtol 1e-4 in f32 and rtol 8e-3 in bf16 (one
bf16 rounding of the stored value), input gradients atol 3e-2 / rtol 1e-2, tap-weight gradients
atol 2e-2 / rtol 1e-3, bias / gamma / beta gradients atol 2e-3 / rtol 1e-4."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (B, T, C = U/2, K): T < K with a ragged channel tile, K = 3, two channel tiles, and the recipe
# width with more than one 64-frame tile
CASES = [(3, 37, 64, 31), (2, 20, 72, 31), (4, 20, 64, 3), (2, 70, 128, 15), (2, 130, 512, 31)]
MERGE_C2 = {64: 128, 72: 144, 128: 128, 512: 512}  # 2d of the merge case with the same (B, T, K)
DTYPES = [torch.float32, torch.bfloat16]


def _bf(t):
    return t.to(torch.bfloat16).float()


def _ws(fn, *args, n=1):
    vals = [ctypes.c_long(0) for _ in range(n)]
    assert fn(*args, *[ctypes.addressof(v) for v in vals]) == 0
    return [v.value for v in vals]


@functools.lru_cache(maxsize=None)
def csgu_case(B, T, C, K):
    """bf16-valued inputs and the float64 reference (forward, every gradient), computed once."""
    g = torch.Generator().manual_seed(1000 * B + 10 * T + C + K)
    N, U = B * T, 2 * C
    h = _bf(torch.randn(N, U, generator=g) * 1.5)
    dout = _bf(torch.randn(N, C, generator=g))
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.1
    w = torch.randn(C, K, generator=g) * 0.2
    bias = torch.randn(C, generator=g)
    hr = h.double().requires_grad_(True)
    p64 = [t.double().requires_grad_(True) for t in (gamma, beta, w, bias)]
    a, gate = F.gelu(hr[:, :C]), F.gelu(hr[:, C:])
    ln = F.layer_norm(gate, (C,), p64[0], p64[1], eps=1e-12)
    conv = F.conv1d(ln.view(B, T, C).transpose(1, 2), p64[2].view(C, 1, K), p64[3], padding=(K - 1) // 2, groups=C)
    out = a * conv.transpose(1, 2).reshape(N, C)
    out.backward(dout.double())
    mean = gate.detach().mean(1)
    rstd = 1.0 / torch.sqrt(gate.detach().var(1, unbiased=False) + 1e-12)
    ref = dict(out=out.detach(), dh=hr.grad, dgamma=p64[0].grad, dbeta=p64[1].grad, dw=p64[2].grad, dbias=p64[3].grad,
               mean=mean, rstd=rstd)
    return dict(h=h, dout=dout, gamma=gamma, beta=beta, w=w, bias=bias), ref


def run_csgu(B, T, C, K, dt, p=0.0, seed=1234, backward=True):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    inp, _ = csgu_case(B, T, C, K)
    N, U = B * T, 2 * C
    st = ops.stream()
    h = inp["h"].to(dt).cuda()
    dout = inp["dout"].to(dt).cuda()
    gamma, beta, w, bias = (inp[k].cuda() for k in ("gamma", "beta", "w", "bias"))
    mean, rstd = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    assert lib.ea_csgu_stats(N, U, h.data_ptr(), ops.dt(h), 1e-12, mean.data_ptr(), rstd.data_ptr(), st) == 0
    out = torch.empty(N, C, dtype=dt, device="cuda")
    assert lib.ea_csgu_fwd(B, T, U, K, h.data_ptr(), ops.dt(h), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                           beta.data_ptr(), w.data_ptr(), bias.data_ptr(), p, seed, out.data_ptr(), st) == 0
    res = dict(out=out, mean=mean, rstd=rstd)
    if backward:
        n_dln, n_ws = _ws(lib.ea_csgu_bwd_ws_elems, B, T, U, K, n=2)
        dln = torch.empty(n_dln, device="cuda")
        ws = torch.empty(n_ws, device="cuda")
        dh = torch.full((N, U), float("nan"), dtype=dt, device="cuda")
        # parameter gradients accumulate onto what is there; dw | dbias adjacent as in the arena
        g = torch.Generator().manual_seed(5)
        pre = {k: torch.randn(n, generator=g) for k, n in (("dgamma", C), ("dbeta", C), ("dwb", C * K + C))}
        dgamma, dbeta, dwb = (pre[k].clone().cuda() for k in ("dgamma", "dbeta", "dwb"))
        assert lib.ea_csgu_bwd(B, T, U, K, dout.data_ptr(), h.data_ptr(), ops.dt(h), mean.data_ptr(), rstd.data_ptr(),
                               gamma.data_ptr(), beta.data_ptr(), w.data_ptr(), bias.data_ptr(), p, seed,
                               dh.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), dwb.data_ptr(),
                               dwb[C * K:].data_ptr(), 1, dln.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0
        torch.cuda.synchronize()
        res.update(dh=dh, dgamma=dgamma.cpu() - pre["dgamma"], dbeta=dbeta.cpu() - pre["dbeta"],
                   dw=(dwb.cpu() - pre["dwb"])[:C * K].view(C, K), dbias=(dwb.cpu() - pre["dwb"])[C * K:])
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("N,U", [(7, 144), (260, 1024)])
@pytest.mark.parametrize("dt", DTYPES)
def test_csgu_row_stats_vs_fp64(N, U, dt):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    g = torch.Generator().manual_seed(N + U)
    h = _bf(torch.randn(N, U, generator=g) * 1.5)
    hd = h.to(dt).cuda()
    mean, rstd = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    assert lib.ea_csgu_stats(N, U, hd.data_ptr(), ops.dt(hd), 1e-12, mean.data_ptr(), rstd.data_ptr(),
                             ops.stream()) == 0
    torch.cuda.synchronize()
    gate = F.gelu(h.double()[:, U // 2:])
    torch.testing.assert_close(mean.double().cpu(), gate.mean(1), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(rstd.double().cpu(), 1.0 / torch.sqrt(gate.var(1, unbiased=False) + 1e-12),
                               atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("B,T,C,K", CASES)
@pytest.mark.parametrize("dt", DTYPES)
def test_csgu_fwd_bwd_vs_fp64(B, T, C, K, dt):
    _, ref = csgu_case(B, T, C, K)
    r = run_csgu(B, T, C, K, dt)
    torch.testing.assert_close(r["mean"].double().cpu(), ref["mean"], atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(r["rstd"].double().cpu(), ref["rstd"], atol=1e-5, rtol=1e-5)
    out_tol = dict(atol=1e-4, rtol=1e-4) if dt == torch.float32 else dict(atol=1e-4, rtol=8e-3)
    for k, tol in (("out", out_tol), ("dh", dict(atol=3e-2, rtol=1e-2)), ("dw", dict(atol=2e-2, rtol=1e-3)),
                   ("dbias", dict(atol=2e-3, rtol=1e-4)), ("dgamma", dict(atol=2e-3, rtol=1e-4)),
                   ("dbeta", dict(atol=2e-3, rtol=1e-4))):
        got = r[k].double().cpu()
        err = (got - ref[k]).abs().max().item()
        print(f"csgu {(B, T, C, K)} {dt} {k}: max abs err {err:.3e} (max |ref| {ref[k].abs().max().item():.3e})")
        torch.testing.assert_close(got, ref[k], msg=lambda m, k=k: f"{k}: {m}", **tol)


@pytest.mark.parametrize("dt", DTYPES)
def test_csgu_dropout(dt):
    B, T, C, K = 2, 130, 512, 31
    p = 0.5
    r0 = run_csgu(B, T, C, K, dt)
    r1 = run_csgu(B, T, C, K, dt, p=p, seed=99)
    r2 = run_csgu(B, T, C, K, dt, p=p, seed=99, backward=False)
    r3 = run_csgu(B, T, C, K, dt, p=p, seed=100, backward=False)
    assert torch.equal(r1["out"], r2["out"])  # one seed, one mask
    assert not torch.equal(r1["out"], r3["out"])
    out0, out1 = r0["out"].float(), r1["out"].float()
    live = out0 != 0
    dropped = (out1 == 0) & live
    kept = ~dropped & live
    assert torch.equal(out1[kept], (out0 / (1 - p))[kept])  # scaling by 2 is exact in both dtypes
    frac = dropped.sum().item() / live.sum().item()
    print("dropped fraction", frac)
    assert abs(frac - 0.5) <= 0.05
    # the backward regenerates the mask: dx_r is zero exactly where the forward dropped
    dxr0, dxr1 = r0["dh"][:, :C].float(), r1["dh"][:, :C].float()
    assert bool((dxr1[dropped] == 0).all())
    live_g = kept & (dxr0 != 0)
    assert bool((dxr1[live_g] != 0).all()) and live_g.sum().item() > 0.4 * live.sum().item()
    assert torch.equal(dxr1[kept], (dxr0 / (1 - p))[kept])


@functools.lru_cache(maxsize=None)
def merge_case(B, T, C2, K):
    g = torch.Generator().manual_seed(77 * B + T + C2 + K)
    N = B * T
    xc = _bf(torch.randn(N, C2, generator=g))
    dm = _bf(torch.randn(N, C2, generator=g))
    w = torch.randn(C2, K, generator=g) * 0.2
    bias = torch.randn(C2, generator=g)
    xr = xc.double().requires_grad_(True)
    wr, br = w.double().requires_grad_(True), bias.double().requires_grad_(True)
    conv = F.conv1d(xr.view(B, T, C2).transpose(1, 2), wr.view(C2, 1, K), br, padding=(K - 1) // 2, groups=C2)
    m = xr + conv.transpose(1, 2).reshape(N, C2)
    m.backward(dm.double())
    return dict(xc=xc, dm=dm, w=w, bias=bias), dict(m=m.detach(), dxc=xr.grad, dw=wr.grad, dbias=br.grad)


def run_merge(B, T, C2, K, dt, p=0.0, seed_a=0, seed_b=0):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    inp, _ = merge_case(B, T, C2, K)
    N = B * T
    st = ops.stream()
    xc, dm = inp["xc"].to(dt).cuda(), inp["dm"].to(dt).cuda()
    w, bias = inp["w"].cuda(), inp["bias"].cuda()
    m = torch.empty(N, C2, dtype=dt, device="cuda")
    assert lib.ea_merge_conv_fwd(B, T, C2, K, xc.data_ptr(), ops.dt(xc), w.data_ptr(), bias.data_ptr(), m.data_ptr(),
                                 st) == 0
    (n_ws,) = _ws(lib.ea_merge_conv_bwd_ws_elems, B, T, C2, K)
    ws = torch.empty(n_ws, device="cuda")
    dxc = torch.full((N, C2), float("nan"), dtype=dt, device="cuda")
    dw, db = torch.zeros(C2, K, device="cuda"), torch.zeros(C2, device="cuda")  # not adjacent: two reductions
    assert lib.ea_merge_conv_bwd(B, T, C2, K, xc.data_ptr(), dm.data_ptr(), ops.dt(dm), w.data_ptr(), p, seed_a, seed_b,
                                 dxc.data_ptr(), dw.data_ptr(), db.data_ptr(), 1, ws.data_ptr(), ws.numel(), st) == 0
    torch.cuda.synchronize()
    return dict(m=m, dxc=dxc, dw=dw, dbias=db)


@pytest.mark.parametrize("B,T,C,K", CASES)
@pytest.mark.parametrize("dt", DTYPES)
def test_merge_conv_fwd_bwd_vs_fp64(B, T, C, K, dt):
    C2 = MERGE_C2[C]
    _, ref = merge_case(B, T, C2, K)
    r = run_merge(B, T, C2, K, dt)
    out_tol = dict(atol=1e-4, rtol=1e-4) if dt == torch.float32 else dict(atol=1e-4, rtol=8e-3)
    for k, tol in (("m", out_tol), ("dxc", dict(atol=3e-2, rtol=1e-2)), ("dw", dict(atol=2e-2, rtol=1e-3)),
                   ("dbias", dict(atol=2e-3, rtol=1e-4))):
        got = r[k].double().cpu()
        print(f"merge {(B, T, C2, K)} {dt} {k}: max abs err {(got - ref[k]).abs().max().item():.3e}")
        torch.testing.assert_close(got, ref[k], msg=lambda m, k=k: f"{k}: {m}", **tol)


@pytest.mark.parametrize("dt", DTYPES)
def test_merge_bwd_applies_the_branch_gemms_dropout_masks(dt):
    """With p > 0 the merge backward's store masks each half of dxc with the dropout stream of the
    GEMM that wrote that half of x_concat in the forward (N = d columns, into a strided view)."""
    from espnet_amd import hip_ops as ops
    from espnet_amd.layers.common import EPI_STORE
    B, T, C2, K = 2, 70, 128, 15
    N, d = B * T, C2 // 2
    p, seeds = 0.5, (4321, 8765)
    r0 = run_merge(B, T, C2, K, dt)
    r1 = run_merge(B, T, C2, K, dt, p=p, seed_a=seeds[0], seed_b=seeds[1])
    x = torch.ones(N, 16, dtype=dt, device="cuda")
    wgt = torch.ones(d, 16, dtype=dt, device="cuda")
    xcat = torch.zeros(N, C2, dtype=dt, device="cuda")
    for half, seed in enumerate(seeds):
        ops.linear(x, wgt, xcat[:, half * d:(half + 1) * d], epi=ops.make_epi(EPI_STORE, drop_p=p, seed=seed))
    torch.cuda.synchronize()
    keep = xcat.float() != 0  # 16 / (1 - p) where kept
    assert 0.45 < keep.float().mean().item() < 0.55
    assert not torch.equal(keep[:, :d], keep[:, d:])
    want = r0["dxc"].float() / (1 - p) * keep
    assert torch.equal(r1["dxc"].float(), want)
    torch.testing.assert_close(r1["dw"], r0["dw"], atol=0, rtol=0)  # the masks touch the store only
