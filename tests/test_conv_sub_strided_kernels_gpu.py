"""The strided valid-conv kernels (csrc/conv_sub.hip), conv.2 of input_layer conv2d6 (5x5 stride 3) and
conv2d2 (3x3 stride 1), alone against float64 F.conv2d on the CPU, f32 and bf16: forward with bias +
ReLU, input gradient under conv1's ReLU mask, weight and bias gradients, each on the operands the
kernels themselves read (x1, the masked dY as stored), bf16-rounded under bf16.

Tolerance (tests/test_vgg2l_kernels_gpu.py's rule, MARGIN 4): 4 x err or 4 f32 ulps at the array's
magnitude, err = max |f32 - f64| of the same reference in float32; arrays the kernels store in bf16
(x2, dx1) get one bf16 rounding on top, 2^-8 |ref| per element.

Shapes (B, T, F, C) of the features, x1 (B, (T-1)//2, (F-1)//2, C): conv2d6's minimum (x1 5x5, one output
pixel, a K chunk shorter than 32); x1 11x9 with an uncovered last column and C = 24 (N and K tails); x1
12x13 with an uncovered last row, partial tiles, nine populated residue classes; several weight-gradient
pixel ranges with a partial last one; conv2d2's minimum (x1 3x3)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lstm_train_goldens import tolerance

pytestmark = pytest.mark.gpu
MARGIN = 4
BF_STEP = 2.0 ** -8
KS = {"conv2d6": (5, 3), "conv2d2": (3, 1)}
SHAPES = [(2, 11, 11, 8), (1, 23, 20, 24), (3, 26, 27, 40), (2, 64, 83, 72)]
CASES = [(layer, s) for layer in KS for s in SHAPES] + [("conv2d2", (1, 7, 7, 8))]


def _nchw(t, B, H, W, C):
    return t.float().cpu().view(B, H, W, C).permute(0, 3, 1, 2).contiguous()


def _check(got, r64, r32, what, stored_bf16=False):
    ref = r64.double().numpy()
    err = float((r32.double() - r64.double()).abs().max())
    base = tolerance(ref, err, MARGIN)
    tol = base + (BF_STEP * np.abs(ref) if stored_bf16 else 0.0)
    dev = np.abs(got.double().numpy() - ref)
    print(f"{what}: max |err| {dev.max():.3e}, tolerance {base:.3e} (reference f32 err {err:.1e})")
    assert got.shape == r64.shape and float((dev - tol).max()) <= 0.0, what


@pytest.mark.parametrize("amp", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("layer,shape", CASES, ids=[f"{c[0]}-b{c[1][0]}t{c[1][1]}f{c[1][2]}c{c[1][3]}" for c in CASES])
def test_conv2_forward_and_gradients(layer, shape, amp):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    (k, s), (B, T, Fd, C) = KS[layer], shape
    T1, F1 = (T - 1) // 2, (Fd - 1) // 2
    T2, F2 = (T1 - k) // s + 1, (F1 - k) // s + 1
    cd = torch.bfloat16 if amp else torch.float32
    gen = torch.Generator().manual_seed(7)
    w = (torch.randn(C, C, k, k, generator=gen) / (k * C ** 0.5)).cuda()
    bias = (0.1 * torch.randn(C, generator=gen)).cuda()
    x1 = torch.relu(torch.randn(B, T1, F1, C, generator=gen)).to(cd).cuda()
    geo, st = (B, T1, F1, C, k, s), ops.stream()
    dt = ops.dt(x1)

    w2 = torch.empty(C, k * k * C, dtype=cd, device="cuda")
    ops.permute3(w, w2, C, C, k * k)
    x2 = torch.empty(B, T2, F2, C, dtype=cd, device="cuda")
    lib.ea_conv_sub_fwd(*geo, dt, x1.data_ptr(), w2.data_ptr(), bias.data_ptr(), x2.data_ptr(), st)
    dy = (torch.randn(B, T2, F2, C, generator=gen).cuda() * (x2 > 0)).to(cd)  # the masked dY, as stored
    w2t = torch.empty(C, k * k * C, dtype=cd, device="cuda")
    ops.permute3(w, w2t, 1, C, C * k * k)
    dx1 = torch.full((B, T1, F1, C), float("nan"), dtype=cd, device="cuda")
    lib.ea_conv_sub_dgrad(*geo, dt, dy.data_ptr(), w2t.data_ptr(), x1.data_ptr(), dx1.data_ptr(), st)
    n = ctypes.c_int(0)
    lib.ea_conv_sub_wgrad_splits(*geo, ctypes.addressof(n))
    part = torch.empty(n.value, C * k * k * C, device="cuda")
    lib.ea_conv_sub_wgrad(*geo, dt, x1.data_ptr(), dy.data_ptr(), part.data_ptr(), n.value, st)
    dw2 = torch.empty(C, k * k * C, device="cuda")
    lib.ea_reduce_partials(n.value, dw2.numel(), part.data_ptr(), dw2.numel(), dw2.data_ptr(), 0, st)
    dw = torch.zeros(C, C, k, k, device="cuda")
    ops.permute3(dw2, dw, C, k * k, C, accumulate=True)
    db = torch.zeros(C, device="cuda")
    ops.colsum(dy.view(-1, C), db)
    torch.cuda.synchronize()
    assert shape != (2, 64, 83, 72) or (n.value > 1 and (B * T2 * F2) % 32)  # ranges, the last one partial

    xs, dys = _nchw(x1, B, T1, F1, C), _nchw(dy, B, T2, F2, C)
    wr = w.cpu().to(cd).float()
    op = (T1 - (s * (T2 - 1) + k), F1 - (s * (F2 - 1) + k))  # x1 rows / columns no window covers
    ref = {}
    for dtype in (torch.float64, torch.float32):
        c = lambda t: t.to(dtype)  # noqa: E731
        ref[dtype] = dict(
            x2=torch.relu(F.conv2d(c(xs), c(wr), c(bias.cpu()), stride=s)),
            dx1=F.conv_transpose2d(c(dys), c(wr), stride=s, output_padding=op) * (xs > 0),
            dw=torch.nn.grad.conv2d_weight(c(xs), w.shape, c(dys), stride=s),
            db=c(dys).sum((0, 2, 3)))
    r64, r32 = ref[torch.float64], ref[torch.float32]
    got_dx1 = _nchw(dx1, B, T1, F1, C)
    _check(_nchw(x2, B, T2, F2, C), r64["x2"], r32["x2"], "forward, bias + relu", amp)
    _check(got_dx1, r64["dx1"], r32["dx1"], "input gradient", amp)
    _check(dw.cpu(), r64["dw"], r32["dw"], "weight gradient")
    _check(db.cpu(), r64["db"], r32["db"], "bias gradient")
    assert not got_dx1[:, :, T1 - op[0]:].any() and not got_dx1[:, :, :, F1 - op[1]:].any()  # exact zeros
