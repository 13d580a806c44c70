"""The VGG2L kernels (csrc/vgg2l.hip) layer by layer against float64 F.conv2d / explicit pooling on
the CPU, in f32 and bf16.

Every layer is checked on the input the kernels themselves gave it (the stored activation of the
layer below, the stored gradient of the layer above), so a layer's reference never inherits
another layer's error: forward with ReLU (and the fused pool), input gradient, weight and bias
gradients of the four layers 1->64, 64->64, 64->128, 128->128.  bf16: float64 on the bf16-rounded
GEMM operands (weights, activations, the gradient read through the decisions); conv1_1 is a vector
kernel on f32 weights and features in both dtypes, the bias gradients sum unrounded values.

Tolerance (tests/lstm_train_goldens.py tolerance, MARGIN 4): 4 x err or 4 f32 ulps at the array's
magnitude, err = max |f32 - f64| of this same reference run in float32 on the CPU; an array the
kernels store in bf16 gets one bf16 rounding on top, element by element: 2^-8 |ref| (bf16 keeps 8
significant bits, so an ulp at x is 2^-7 of x's power of two and round-to-nearest is off by at most
half of it, 2^-8 2^floor(log2 |x|) <= 2^-8 |x|).

Shapes: B 2, T 13, F 10 (odd T; F 10 -> 5 -> 3, odd after the first pool); B 3, T 7, F 83 (the
recipes' odd feature count; pixel counts no multiple of the tile); B 1, T 1, F 2 (a one-row image);
B 1, T 3, F 1 (a one-column image); B 2, T 40, F 53 (4240 pixels: 133 chunks of 32, so the weight
gradient's pixel ranges hold two chunks each, 67 ranges).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vgg_rnn_goldens as G

pytestmark = pytest.mark.gpu
MARGIN = G.MARGIN
SHAPES = [(2, 13, 10), (3, 7, 83), (1, 1, 2), (1, 3, 1), (2, 40, 53)]
IDS = ["b2t13f10", "b3t7f83", "b1t1f2", "b1t3f1", "b2t40f53"]
CONVS = G.CONVS
BF_STEP = 2.0 ** -8


def _half(n):
    return (n + 1) // 2


def _rd(t, amp):
    return t.float().to(torch.bfloat16).to(t.dtype) if amp else t


def _nchw(t, B, H, W, C):
    return t.detach().float().cpu().view(B, H, W, C).permute(0, 3, 1, 2).contiguous()


_pool, _scatter, _dw = G.pool_scan, G.pool_scatter, G.conv_dw  # the restatement's explicit pooling


class Run:
    """One forward + backward of VGG2L on the GPU with everything it kept, on the CPU."""

    def __init__(self, shape, amp, seed, plant=None):
        from espnet_amd.asr.encoder.vgg_rnn_encoder import VGGRNNEncoder
        B, T, Fd = shape
        torch.manual_seed(seed)
        enc = VGGRNNEncoder(Fd, num_layers=1, hidden_size=4, output_size=4)
        vgg = enc.enc[0]
        if plant is not None:
            with torch.no_grad():
                plant(vgg)
        self.w = {n: getattr(vgg, n).weight.detach().clone() for n in CONVS}
        self.b = {n: getattr(vgg, n).bias.detach().clone() for n in CONVS}
        self.arena = G.prepare_encoder(enc, amp)
        gen = torch.Generator().manual_seed(100 + seed)
        self.xs = torch.randn(B, T, Fd, generator=gen)
        H4, W4 = _half(_half(T)), _half(_half(Fd))
        self.cot = torch.randn(H4 * B, 128 * W4, generator=gen)
        vgg.keep_decisions = True
        vgg.train()
        for p in vgg.parameters():
            p.grad.zero_()
        x, lens, T4 = vgg(self.xs.cuda(), torch.full((B,), T, device="cuda"), enc._anchor)
        assert T4 == H4 and x.shape == self.cot.shape and x.dtype == torch.float32
        x.backward(self.cot.cuda())
        torch.cuda.synchronize()
        self.shape, self.amp, self.vgg = shape, amp, vgg
        self.dec = {k: v.cpu() for k, v in vgg.decisions().items()}
        H2, W2 = _half(T), _half(Fd)
        L = vgg._last
        self.x1, self.d1 = _nchw(L["x1"], B, T, Fd, 64), _nchw(L["d1"], B, T, Fd, 64)
        self.p1, self.dp1 = _nchw(L["p1"], B, H2, W2, 64), _nchw(L["dp1"], B, H2, W2, 64)
        self.x3, self.d3 = _nchw(L["x3"], B, H2, W2, 128), _nchw(L["d3"], B, H2, W2, 128)
        self.out = L["out"].detach().cpu().view(H4, B, 128, W4).permute(1, 2, 0, 3).contiguous()
        self.dout = self.cot.view(H4, B, 128, W4).permute(1, 2, 0, 3).contiguous()
        self.grad = {n: (getattr(vgg, n).weight.grad.cpu().clone(), getattr(vgg, n).bias.grad.cpu().clone())
                     for n in CONVS}
        self.raw = (L["out"].detach().cpu().clone(), L["dec1"].cpu().clone(), L["dec2"].cpu().clone())

    def reference(self, dtype, dec=None):
        """Every layer's arrays in `dtype` from the kernels' own layer inputs.  dec: the decisions the
        backward routes by (default: this reference's own)."""
        amp, (B, T, Fd) = self.amp, self.shape
        c = lambda t: t.to(dtype)  # noqa: E731
        w = {n: c(_rd(self.w[n], amp and n != "conv1_1")) for n in CONVS}
        b = {n: c(self.b[n]) for n in CONVS}
        r = {}
        xs = c(self.xs).unsqueeze(1)
        r["pre0"] = F.conv2d(xs, w["conv1_1"], b["conv1_1"], padding=1)
        r["pre1"] = F.conv2d(c(self.x1), w["conv1_2"], b["conv1_2"], padding=1)
        r["p1"], r["pool0"] = _pool(torch.relu(r["pre1"]))
        r["pre2"] = F.conv2d(c(self.p1), w["conv2_1"], b["conv2_1"], padding=1)
        r["pre3"] = F.conv2d(c(self.x3), w["conv2_2"], b["conv2_2"], padding=1)
        r["out"], r["pool1"] = _pool(torch.relu(r["pre3"]))
        for i in range(4):
            r[f"relu{i}"] = r[f"pre{i}"] > 0
        d = dec if dec is not None else r
        H2, W2 = _half(T), _half(Fd)
        # conv2_2
        g3 = _scatter(c(self.dout), d["pool1"], d["relu3"], H2, W2)
        r["db.conv2_2"] = g3.sum((0, 2, 3))
        g3 = _rd(g3, amp)
        r["dw.conv2_2"] = _dw(c(self.x3), g3, w["conv2_2"].shape)
        r["d3"] = F.conv_transpose2d(g3, w["conv2_2"], padding=1) * (self.x3 > 0)
        # conv2_1, from the kernels' d3
        g2 = c(self.d3)
        r["db.conv2_1"] = g2.sum((0, 2, 3))
        r["dw.conv2_1"] = _dw(c(self.p1), g2, w["conv2_1"].shape)
        r["dp1"] = F.conv_transpose2d(g2, w["conv2_1"], padding=1)
        # conv1_2, from the kernels' dp1
        g1 = _scatter(c(self.dp1), d["pool0"], d["relu1"], T, Fd)
        r["db.conv1_2"] = g1.sum((0, 2, 3))
        g1 = _rd(g1, amp)
        r["dw.conv1_2"] = _dw(c(self.x1), g1, w["conv1_2"].shape)
        r["d1"] = F.conv_transpose2d(g1, w["conv1_2"], padding=1) * (self.x1 > 0)
        # conv1_1, from the kernels' d1
        g0 = c(self.d1)
        r["db.conv1_1"] = g0.sum((0, 2, 3))
        r["dw.conv1_1"] = _dw(xs, g0, w["conv1_1"].shape)
        return r


def _check(got, r64, r32, key, what, stored_bf16=False):
    ref = r64[key].double().numpy()
    err = float((r32[key].double() - r64[key].double()).abs().max())
    got = np.asarray(got.double().numpy())
    base = G.tolerance(ref, err, MARGIN)
    tol = base + (BF_STEP * np.abs(ref) if stored_bf16 else 0.0)  # the bf16 rounding: element by element
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    dev = np.abs(got - ref)
    worst = float(dev.max()) if ref.size else 0.0
    over = float((dev - tol).max()) if ref.size else 0.0
    print(f"{what}: max |err| {worst:.3e}, tolerance {base:.3e}" + (" + 2^-8 |ref| per element" if stored_bf16 else "")
          + f" (reference f32 err {err:.1e})")
    assert over <= 0.0, f"{what}: exceeds the tolerance by {over:.3e} (max |err| {worst:.3e}, base {base:.3e})"


@pytest.mark.parametrize("amp", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_layer_forward_and_backward(shape, amp):
    run = Run(shape, amp, seed=0)
    r64, r32 = run.reference(torch.float64, run.dec), run.reference(torch.float32, run.dec)
    r64["y0"], r32["y0"] = torch.relu(r64["pre0"]), torch.relu(r32["pre0"])
    r64["y2"], r32["y2"] = torch.relu(r64["pre2"]), torch.relu(r32["pre2"])
    _check(run.x1, r64, r32, "y0", "conv1_1 + relu", amp)
    _check(run.p1, r64, r32, "p1", "conv1_2 + relu + pool", amp)
    _check(run.x3, r64, r32, "y2", "conv2_1 + relu", amp)
    _check(run.out, r64, r32, "out", "conv2_2 + relu + pool")
    _check(run.d3, r64, r32, "d3", "conv2_2 input gradient", amp)
    _check(run.dp1, r64, r32, "dp1", "conv2_1 input gradient")
    _check(run.d1, r64, r32, "d1", "conv1_2 input gradient", amp)
    for n in CONVS:
        _check(run.grad[n][0], r64, r32, "dw." + n, n + " weight gradient")
        _check(run.grad[n][1], r64, r32, "db." + n, n + " bias gradient")
    # the kernels' decisions are decisions float64 could have taken: a set ReLU bit has a
    # pre-activation above -MARGIN x err, a cleared one below +MARGIN x err, and the winner is within
    # MARGIN x err of the window's maximum
    for i in range(4):
        e = MARGIN * float((r32[f"pre{i}"].double() - r64[f"pre{i}"]).abs().max())
        pre, bit = r64[f"pre{i}"], run.dec[f"relu{i}"]
        assert bool((pre[bit] > -e).all()) and bool((pre[~bit] < e).all()), f"relu{i}"
    for j, (i, val) in enumerate(((1, "p1"), (3, "out"))):
        e = MARGIN * float((r32[f"pre{i}"].double() - r64[f"pre{i}"]).abs().max())
        y = torch.relu(r64[f"pre{i}"])
        pad = torch.zeros(*y.shape[:2], 2 * _half(y.shape[2]), 2 * _half(y.shape[3]), dtype=y.dtype)
        pad[:, :, :y.shape[2], :y.shape[3]] = y
        win = torch.stack([pad[:, :, a::2, b::2] for a in (0, 1) for b in (0, 1)], dim=-1)
        picked = win.gather(-1, run.dec[f"pool{j}"].unsqueeze(-1)).squeeze(-1)
        assert bool((picked >= r64[val] - e).all()), f"pool{j}"


@pytest.mark.parametrize("amp", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES[:4], ids=IDS[:4])
def test_decisions_equal_float64s(shape, amp):
    """Inputs drawn (first seed that qualifies) so that in float64 no pre-activation and no window's
    top-two gap lies within MARGIN x the f32-vs-f64 error of that array: then every ReLU bit and
    every argmax must be float64's.  bf16 accumulates in f32 within a layer, so the same guard holds."""
    for seed in range(40):
        run = Run(shape, amp, seed)
        r64, r32 = run.reference(torch.float64), run.reference(torch.float32)
        ok = True
        for i in range(4):
            e = MARGIN * float((r32[f"pre{i}"].double() - r64[f"pre{i}"]).abs().max())
            ok = ok and float(r64[f"pre{i}"].abs().min()) > e
            if i in (1, 3):
                ok = ok and float(G.pool_gap(torch.relu(r64[f"pre{i}"])).min()) > e
        if ok:
            break
    assert ok, "no seed in 0..39 clears the guard"
    print(f"seed {seed}")
    for i in range(4):
        assert torch.equal(run.dec[f"relu{i}"], r64[f"relu{i}"]), f"relu{i}"
    for j in range(2):
        assert run.dec[f"pool{j}"].dtype == torch.int64
        assert torch.equal(run.dec[f"pool{j}"], r64[f"pool{j}"]), f"pool{j}"


@pytest.mark.parametrize("amp", [False, True], ids=["f32", "bf16"])
def test_two_runs_are_bit_equal(amp):
    a, b = Run((3, 7, 83), amp, seed=2), Run((3, 7, 83), amp, seed=2)
    for x, y in zip(a.raw, b.raw):
        assert torch.equal(x, y)
    for k in ("x1", "p1", "x3", "d3", "dp1", "d1"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for n in CONVS:
        assert torch.equal(a.grad[n][0], b.grad[n][0]) and torch.equal(a.grad[n][1], b.grad[n][1]), n


def _plant(layer, bias):
    def f(vgg):
        getattr(vgg, layer).weight.zero_()
        getattr(vgg, layer).bias.fill_(bias)
    return f


@pytest.mark.parametrize("amp", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("layer,pool", [("conv1_2", "pool0"), ("conv2_2", "pool1")])
def test_exactly_equal_positive_values_route_to_the_first(layer, pool, amp):
    """Zero weights and bias 0.5: every value of every window is exactly 0.5, in full windows and in
    the one-row and one-column windows at the odd edges (T 13, F 10 -> 5).  The winner is position 0
    and the whole gradient goes there: the layer's weight gradient is the one float64 computes with
    all-zero argmax, not the one of any other routing."""
    run = Run((2, 13, 10), amp, seed=3, plant=_plant(layer, 0.5))
    val = run.p1 if layer == "conv1_2" else run.out
    assert bool((val == 0.5).all()) and not run.dec[pool].any()
    assert bool(run.dec["relu1" if layer == "conv1_2" else "relu3"].all())
    r64, r32 = run.reference(torch.float64), run.reference(torch.float32)
    assert not r64[pool].any()
    _check(run.grad[layer][0], r64, r32, "dw." + layer, layer + " weight gradient, ties")
    _check(run.grad[layer][1], r64, r32, "db." + layer, layer + " bias gradient, ties")
    last = {k: (torch.full_like(v, 3) if k == pool else v) for k, v in run.dec.items()}
    other = run.reference(torch.float64, last)["dw." + layer]
    assert float((other - r64["dw." + layer]).abs().max()) > 1e-3  # the routing is visible in this gradient


@pytest.mark.parametrize("amp", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("layer", ["conv1_2", "conv2_2"])
def test_all_nonpositive_windows_give_zero_output_and_zero_gradient(layer, amp):
    run = Run((2, 13, 10), amp, seed=4, plant=_plant(layer, -0.5))
    val, pool, relu = (run.p1, "pool0", "relu1") if layer == "conv1_2" else (run.out, "pool1", "relu3")
    assert not val.any() and not run.dec[pool].any() and not run.dec[relu].any()
    below = CONVS[:CONVS.index(layer) + 1]
    for n in below:  # nothing passes the pool: the layer and everything below it get exactly zero
        assert not run.grad[n][0].any() and not run.grad[n][1].any(), n
    assert not (run.d1 if layer == "conv1_2" else run.d3).any()
