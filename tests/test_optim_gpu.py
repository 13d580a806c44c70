"""Adam update kernel (ea_adam_step: torch.optim.Adam arithmetic, grad-clip coefficient,
bf16 shadow) against an f32 torch restatement of the same element formula (odd n, aligned
and misaligned views); the gradient norm (ea_sqnorm) against f64; and the device-resident step
(ea_adam_step_dev: step count, skip on a non-finite norm, clip coefficient, warm-up lr and bias
corrections in ea_opt_state) against an f64 restatement of the bookkeeping."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def adam_restatement(rp, rg, rm, rv, coef, lr, b1, b2, eps, wd, step):
    """One torch.optim.Adam update (L2 weight decay, clipped gradient) in f32 torch."""
    gg = rg * coef + wd * rp
    rm = rm + (1 - b1) * (gg - rm)
    rv = rv * b2 + (1 - b2) * gg * gg
    denom = rv.sqrt() / math.sqrt(1 - b2 ** step) + eps
    rp = rp - (lr / (1 - b1 ** step)) * (rm / denom)
    return rp, rm, rv


@pytest.mark.parametrize("n,off", [(1_000_003, 0), (4096, 0), (777, 1)])
def test_adam_step_matches_restatement(n, off):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    g_ = torch.Generator().manual_seed(n)
    buf = lambda s=1.0: (torch.randn(n + 4, generator=g_) * s).cuda()  # noqa: E731
    p, g, m, v = buf(), buf(0.1), buf(0.01), buf(0.001).abs()
    p16 = torch.empty(n + 4, dtype=torch.bfloat16, device="cuda")
    norm = torch.tensor([7.5], device="cuda")
    lr, b1, b2, eps, wd, step, max_norm = 1e-3, 0.9, 0.98, 1e-9, 1e-6, 3, 5.0
    ref = [t[off:off + n].clone() for t in (p, g, m, v)]
    sl = lambda t: t[off:off + n]  # noqa: E731
    lib.ea_adam_step(n, sl(p).data_ptr(), sl(g).data_ptr(), sl(m).data_ptr(), sl(v).data_ptr(),
                     sl(p16).data_ptr(), lr, b1, b2, eps, wd, step, norm.data_ptr(), max_norm, ops.stream())
    torch.cuda.synchronize()
    rp, rg, rm, rv = ref
    coef = min(max_norm / (7.5 + 1e-6), 1.0)
    rp, rm, rv = adam_restatement(rp, rg, rm, rv, coef, lr, b1, b2, eps, wd, step)
    # a few ulps of each state's scale (the kernel may contract the lerp / moment updates
    # into FMAs; torch rounds every op)
    torch.testing.assert_close(sl(m), rm, rtol=1e-6, atol=3e-8)
    torch.testing.assert_close(sl(v), rv, rtol=1e-6, atol=3e-9)
    torch.testing.assert_close(sl(p), rp, rtol=1e-6, atol=3e-7)
    assert torch.equal(sl(p16), sl(p).to(torch.bfloat16))


@pytest.mark.parametrize("n", [1, 3, 1023, 1025, 1_000_003])
@pytest.mark.parametrize("off", [0, 1])
def test_sqnorm_matches_f64(n, off):
    """16-byte aligned (float4 path) and offset by one float (scalar path).  The kernel sums
    squares in f64 and rounds sqrt once: the result is within 1 ulp of f32 (rtol 2^-23) of the
    f64 norm.  Squares that overflow f32 stay finite; inf and NaN give a non-finite norm, which
    the skip rule of the optimizer step depends on."""
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    g = torch.Generator().manual_seed(n)
    buf = (torch.randn(n + 4, generator=g) * 3).cuda()
    assert buf.data_ptr() % 16 == 0
    ws = torch.full((2048,), float("nan"), dtype=torch.float64, device="cuda")
    norm = torch.full((2,), -1.0, device="cuda")

    def run(x):
        assert x.data_ptr() % 16 == 4 * off
        lib.ea_sqnorm(n, x.data_ptr(), ws.data_ptr(), norm.data_ptr(), ops.stream())
        torch.cuda.synchronize()
        assert norm[1].item() == -1.0
        return norm[0].item()

    x = buf[off:off + n]
    ref = x.cpu().double().norm().item()
    got = run(x)
    print(f"sqnorm n={n} off={off}: rel err {abs(got - ref) / ref:.3g}")
    assert abs(got - ref) <= 2.0 ** -23 * ref
    big = torch.zeros(n + 4)
    big[off], big[off + n - 1] = 3e19, (4e19 if n > 1 else 3e19)
    ref = big[off:off + n].double().norm().item()  # 5e19: the squares overflow f32
    got = run(big.cuda()[off:off + n])
    assert math.isfinite(got) and abs(got - ref) <= 2.0 ** -23 * ref
    for bad in (float("inf"), float("-inf"), float("nan")):
        y = buf.clone()
        y[off + n // 2] = bad
        assert not math.isfinite(run(y[off:off + n]))


def _opt_state(state_dev):
    from espnet_amd import _lib
    return _lib.STRUCTS["ea_opt_state"].from_buffer_copy(state_dev.cpu().numpy().tobytes())


def test_adam_step_dev_bookkeeping_and_skip():
    """Three calls with grad norms above max_norm, NaN, below max_norm under a warm-up schedule
    (warmup_steps = 2: step 1 is on the ramp, step 2 at the peak, step 3 on the decay).  The
    state's f32 scalars are f64 values rounded once (lr, bias corrections: rtol 2^-23, one ulp)
    or two f32 operations (coef: 2 ulp)."""
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import OPT_STATE_BYTES, SCHED_WARMUP, LrSchedule, lib
    from oracle.asr_oracle import warmup_lr
    n, off = 777, 1
    g_ = torch.Generator().manual_seed(n)
    buf = lambda s=1.0: (torch.randn(n + 4, generator=g_) * s).cuda()  # noqa: E731
    p, m, v = buf(), buf(0.01), buf(0.001).abs()
    p16 = torch.zeros(n + 4, dtype=torch.bfloat16, device="cuda")
    sl = lambda t: t[off:off + n]  # noqa: E731
    base_lr, warm, b1, b2, eps, wd, max_norm = 2e-3, 2.0, 0.9, 0.98, 1e-9, 1e-6, 5.0
    sched = LrSchedule(SCHED_WARMUP, warm, base_lr)
    state = torch.zeros(OPT_STATE_BYTES // 8, dtype=torch.int64, device="cuda")
    norm = torch.zeros(1, device="cuda")
    ulp = 2.0 ** -23
    b1f, b2f = (torch.tensor(b, dtype=torch.float32).item() for b in (b1, b2))  # the ABI takes float betas
    step, last = 0, None
    for nrm in (7.5, float("nan"), 2.0):
        grad = buf(0.1)
        norm.fill_(nrm)
        before = [sl(t).clone() for t in (p, m, v, p16)]
        lib.ea_adam_step_dev(n, sl(p).data_ptr(), sl(grad).data_ptr(), sl(m).data_ptr(), sl(v).data_ptr(),
                             sl(p16).data_ptr(), ctypes.byref(sched), b1, b2, eps, wd, state.data_ptr(),
                             norm.data_ptr(), max_norm, ops.stream())
        torch.cuda.synchronize()
        st = _opt_state(state)
        if math.isnan(nrm):  # skipped: the step does not advance, nothing is touched
            assert (st.step, st.skip) == (step, 1) and math.isnan(st.last_norm)
            assert st.next_lr == pytest.approx(warmup_lr(base_lr, step + 1, warm), rel=ulp, abs=0)
            assert (st.lr, st.coef, st.bc1, st.bc2_sqrt) == last
            for t, b in zip((p, m, v, p16), before):
                assert torch.equal(sl(t), b)
            continue
        step += 1
        coef = min(max_norm / (nrm + 1e-6), 1.0)
        assert (st.step, st.skip, st.last_norm) == (step, 0, nrm)
        assert st.coef == pytest.approx(coef, rel=2 * ulp, abs=0)
        assert st.lr == pytest.approx(warmup_lr(base_lr, step, warm), rel=ulp, abs=0)
        assert st.next_lr == pytest.approx(warmup_lr(base_lr, step + 1, warm), rel=ulp, abs=0)
        assert st.bc1 == pytest.approx(1 - b1f ** step, rel=ulp, abs=0)
        assert st.bc2_sqrt == pytest.approx(math.sqrt(1 - b2f ** step), rel=ulp, abs=0)
        last = (st.lr, st.coef, st.bc1, st.bc2_sqrt)
        rp, rm, rv = adam_restatement(before[0], sl(grad), before[1], before[2], coef,
                                      warmup_lr(base_lr, step, warm), b1, b2, eps, wd, step)
        torch.testing.assert_close(sl(m), rm, rtol=1e-6, atol=3e-8)
        torch.testing.assert_close(sl(v), rv, rtol=1e-6, atol=3e-9)
        torch.testing.assert_close(sl(p), rp, rtol=1e-6, atol=3e-7)
        assert torch.equal(sl(p16), sl(p).to(torch.bfloat16))
        assert not torch.equal(sl(p), before[0])
    assert step == 2
