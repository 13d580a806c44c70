"""Linear bias gradients from the grouped weight-gradient GEMM's dY operand
(ea_group_gemm.a_sum, hip_ops.linear_dw(db=...)): the kernel against a ones-column product
(bit for bit) and fp64, the queue against colsum + linear_dw, a tiny model with the switch on
and off."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
PAD = 40  # a_sum buffers are this much longer than M
# (M out-features, N in-features, K tokens, beta, with a_sum)
SHAPES = [(96, 160, 1000, 1.0, True),    # M below one wave group, K % 32 = 8
          (264, 512, 64, 0.0, True),     # two tile rows, two N tiles: only tn == 0 may write
          (520, 64, 31, 1.0, True),      # K shorter than one slice: tail path only
          (256, 256, 7968, 1.0, True),   # the C3 token count
          (300, 520, 130, 0.0, False)]   # no a_sum


def _ops():
    from espnet_amd import hip_ops
    from espnet_amd import _lib
    return hip_ops, _lib


def mk(shape, dtype, gen, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(dtype).cuda()


def _launch(probs, sums=True, xchunk=4, ones=False):
    """One ea_gemm_grouped launch of `probs` from their starting values -> [(C, a_sum)].
    ones: X replaced by all ones and C's column 0 started from a_sum's starting values."""
    ops, L = _ops()
    arr = (L.GroupGemm * len(probs))()
    outs, keep, ntiles = [], [], 0
    for i, p in enumerate(probs):
        C, S = p["C0"].clone(), p["S0"].clone()
        B = p["B"]
        if ones:
            B = torch.ones_like(B)
            C[:, 0] = S[:p["M"]]
            keep.append(B)
        outs.append((C, S))
        arr[i] = L.GroupGemm(p["A"].data_ptr(), B.data_ptr(), C.data_ptr(), p["A"].stride(0), B.stride(0),
                             C.stride(0), p["M"], p["N"], p["K"], p["beta"],
                             S.data_ptr() if sums and p["sum"] else None)
        ntiles += ((p["M"] + 255) // 256) * ((p["N"] + 255) // 256)
    nb = ctypes.c_long(0)
    L.lib.ea_gemm_grouped_ws_bytes(len(probs), ntiles, ctypes.addressof(nb))
    ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    L.lib.ea_gemm_grouped_set_xcd_chunk(xchunk)
    try:
        L.lib.ea_gemm_grouped(0, 0, len(probs), ctypes.addressof(arr), ws.data_ptr(), ws.numel(), ops.stream())
        torch.cuda.synchronize()
    finally:
        L.lib.ea_gemm_grouped_set_xcd_chunk(4)
    return outs


@pytest.fixture(scope="module")
def group():
    """The mixed problems (longest K first, leading dimensions padded as in
    test_gemm_grouped_vs_fp64) and one launch of them with a_sum: (probs, outs)."""
    g = torch.Generator().manual_seed(21)
    up = lambda n: (n + 7) // 8 * 8 + 8  # noqa: E731
    probs = []
    for M, N, K, beta, s in sorted(SHAPES, key=lambda t: -t[2]):
        S0 = torch.randn(M + PAD, generator=g)
        S0[M:] = SENTINEL
        probs.append(dict(M=M, N=N, K=K, beta=beta, sum=s, A=mk((K, up(M)), torch.bfloat16, g),
                          B=mk((K, up(N)), torch.bfloat16, g), C0=torch.randn(M, N + 4, generator=g).cuda(),
                          S0=S0.cuda()))
    return probs, _launch(probs)


def test_a_sum_bitwise_vs_ones_column(group):
    """(a) a_sum == column 0 of the same A times an all-ones X through the same entry point,
    same beta and starting values: pins the slice order and the tail."""
    probs, outs = group
    ref = _launch(probs, sums=False, ones=True)
    for p, (_, S), (C1, _) in zip(probs, outs, ref):
        if p["sum"]:
            assert torch.equal(S[:p["M"]], C1[:, 0]), (p["M"], p["N"], p["K"])


def test_a_sum_vs_fp64(group):
    """(b) a_sum against the fp64 column sums of the bf16 dY, the bound test_gemm_grouped_vs_fp64
    applies to dW of the same launch (dW checked too)."""
    probs, outs = group
    for p, (C, S) in zip(probs, outs):
        M, N, K = p["M"], p["N"], p["K"]
        a = p["A"].double().cpu()[:K, :M]
        ref = p["beta"] * p["C0"][:, :N].double().cpu() + a.t() @ p["B"].double().cpu()[:K, :N]
        torch.testing.assert_close(C[:, :N].double().cpu(), ref, atol=2e-3 * K ** 0.5, rtol=2e-3)
        if p["sum"]:
            sref = p["beta"] * p["S0"][:M].double().cpu() + a.sum(0)
            err = (S[:M].double().cpu() - sref).abs().max().item()
            print(f"a_sum M={M} K={K}: max abs err {err:.3e} (atol {2e-3 * K ** 0.5:.3e})")
            torch.testing.assert_close(S[:M].double().cpu(), sref, atol=2e-3 * K ** 0.5, rtol=2e-3)


def test_a_sum_changes_nothing_else(group):
    """(c) entries past M keep the sentinel, a problem without a_sum keeps its buffer, and C is
    bit-equal to a launch of the same problems without a_sum."""
    probs, outs = group
    plain = _launch(probs, sums=False)
    for p, (C, S), (Cp, Sp) in zip(probs, outs, plain):
        assert torch.equal(C, Cp), (p["M"], p["N"], p["K"])
        assert torch.equal(Sp, p["S0"])
        assert (S[p["M"]:] == SENTINEL).all(), "a_sum written past M"
        if not p["sum"]:
            assert torch.equal(S, p["S0"])


def test_a_sum_independent_of_grouping(group):
    """(d) each problem flushed alone gives the bits it gives among the others; a second
    launch of the group reproduces the first."""
    probs, outs = group
    for p, (C, S) in zip(probs, outs):
        (C1, S1), = _launch([p])
        assert torch.equal(S1, S) and torch.equal(C1, C), (p["M"], p["N"], p["K"])
    for (C, S), (C2, S2) in zip(outs, _launch(probs)):
        assert torch.equal(S2, S) and torch.equal(C2, C)


@pytest.mark.parametrize("xchunk", [1, 0])
def test_a_sum_xcd_mappings(group, xchunk):
    """(e) every tile -> XCD mapping gives the bits of the default (4, the fixture's)."""
    probs, outs = group
    for (C, S), (C2, S2) in zip(outs, _launch(probs, xchunk=xchunk)):
        assert torch.equal(S2, S) and torch.equal(C2, C)


def test_a_sum_host_checks(group):
    """a_sum must be 4-byte aligned and overlap neither a C nor another a_sum of the call."""
    ops, L = _ops()
    probs, _ = group
    p, q = probs[0], probs[1]
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")

    Cs = [p["C0"].clone(), q["C0"].clone()]

    def call(sp, sq):
        arr = (L.GroupGemm * 2)()
        for i, (r, s) in enumerate(((p, sp), (q, sq))):
            arr[i] = L.GroupGemm(r["A"].data_ptr(), r["B"].data_ptr(), Cs[i].data_ptr(), r["A"].stride(0),
                                 r["B"].stride(0), Cs[i].stride(0), r["M"], r["N"], r["K"], r["beta"], s)
        L.lib.ea_gemm_grouped(0, 0, 2, ctypes.addressof(arr), ws.data_ptr(), ws.numel(), ops.stream())

    buf = torch.zeros(4096, device="cuda")
    with pytest.raises(L.HipError):
        call(buf.data_ptr() + 2, None)                                  # misaligned
    with pytest.raises(L.HipError):
        call(buf.data_ptr(), buf.data_ptr() + 4 * (p["M"] - 1))         # two a_sum overlap
    with pytest.raises(L.HipError):
        call(None, Cs[0].data_ptr() + 64)                               # a_sum inside the other problem's C
    call(buf.data_ptr(), buf.data_ptr() + 4 * p["M"])                   # adjacent: fine
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------- the queue
R = 1000


@pytest.fixture
def switches_on():
    """The deferral switches at their defaults (on), whatever the environment says."""
    from espnet_amd import deferred
    prev = deferred.DEFER_WGRAD, deferred.DEFER_REDUCE, deferred.WGRAD_BIAS
    deferred.DEFER_WGRAD = deferred.DEFER_REDUCE = deferred.WGRAD_BIAS = True
    yield deferred
    deferred.DEFER_WGRAD, deferred.DEFER_REDUCE, deferred.WGRAD_BIAS = prev


DIMS = [(96, 160), (256, 512), (512, 64)]


def _queue_case(g):
    dys = [mk((R, n), torch.bfloat16, g) for n, _ in DIMS]
    xs = [mk((R, k), torch.bfloat16, g) for _, k in DIMS]
    w0 = [torch.randn(n, k, generator=g).cuda() for n, k in DIMS]
    b0 = [torch.randn(n, generator=g).cuda() for n, _ in DIMS]
    return dys, xs, w0, b0


def _immediate(ops, dys, xs, w0, b0):
    """colsum + linear_dw outside the queue."""
    ws, bs = [w.clone() for w in w0], [b.clone() for b in b0]
    for dy, x, w, b in zip(dys, xs, ws, bs):
        ops.colsum(dy, b)
        ops.linear_dw(dy, x, w, accumulate=True)
    torch.cuda.synchronize()
    return ws, bs


def _close(got, want):
    # test_deferred_linear_dw_queue's bound for the immediate -> queued change of summation order
    torch.testing.assert_close(got, want, atol=1e-5 * R ** 0.5, rtol=1e-5)


def test_queue_linear_dw_db(switches_on):
    """linear_dw(db=...) inside deferred_wgrad(): every problem carries its bias, and weights and
    biases match colsum + linear_dw on the immediate path."""
    ops, L = _ops()
    deferred = switches_on
    dys, xs, w0, b0 = _queue_case(torch.Generator().manual_seed(31))
    want_w, want_b = _immediate(ops, dys, xs, w0, b0)
    ws, bs = [w.clone() for w in w0], [b.clone() for b in b0]
    with ops.deferred_wgrad() as q:
        for dy, x, w, b in zip(dys, xs, ws, bs):
            ops.linear_dw(dy, x, w, accumulate=True, db=b)
        assert len(q.items) == 3 and all(it[-2] is not None for it in q.items)
        assert not deferred.REDUCE_Q.colsums
    torch.cuda.synchronize()
    for got, want in zip(ws + bs, want_w + want_b):
        _close(got, want)


def test_queue_db_overlapping_reduce_output(switches_on):
    """A db that REDUCE_Q already writes is not carried (and the reverse: a later REDUCE_Q claim
    of a carried db launches the weight-gradient queue first); a db that does not share the
    weight gradient's accumulate is not carried either.  All still correct."""
    ops, L = _ops()
    deferred = switches_on
    g = torch.Generator().manual_seed(32)
    dys, xs, w0, b0 = _queue_case(g)
    other = mk((R, DIMS[0][0]), torch.bfloat16, g)
    want_w, want_b = _immediate(ops, dys, xs, w0, b0)
    ops.colsum(other, want_b[0])
    ops.colsum(dys[2], want_b[2], accumulate=False)  # not accumulated below
    torch.cuda.synchronize()
    for order in ("reduce_first", "wgrad_first"):
        ws, bs = [w.clone() for w in w0], [b.clone() for b in b0]
        with ops.deferred_wgrad() as q:
            if order == "reduce_first":
                ops.colsum(other, bs[0])
                ops.linear_dw(dys[0], xs[0], ws[0], accumulate=True, db=bs[0])
                assert len(q.items) == 1 and q.items[0][-2] is None
                assert len(deferred.REDUCE_Q.colsums) + len(deferred.REDUCE_Q.reduces) >= 1
            else:
                ops.linear_dw(dys[0], xs[0], ws[0], accumulate=True, db=bs[0])
                assert q.items[0][-2] is not None
                ops.colsum(other, bs[0])
                assert not q.items, "the carried bias must be written before REDUCE_Q's sum is queued"
            ops.linear_dw(dys[1], xs[1], ws[1], accumulate=True, db=bs[1])
            assert q.items[-1][-2] is not None
            ops.linear_dw(dys[2], xs[2], ws[2], accumulate=True, db=bs[2], db_accumulate=False)
            assert q.items[-1][-2] is None
        torch.cuda.synchronize()
        for got, want in zip(ws + bs, want_w + want_b):
            _close(got, want)


@pytest.mark.parametrize("mode", ["switch_off", "f32"])
def test_queue_carries_nothing(switches_on, mode):
    """EA_WGRAD_BIAS=0, or f32 operands (the parity mode): the queue carries no bias and the
    column sums run as before, bit-equal to colsum + linear_dw queued separately."""
    ops, L = _ops()
    deferred = switches_on
    dys, xs, w0, b0 = _queue_case(torch.Generator().manual_seed(33))
    if mode == "f32":
        dys, xs = [t.float() for t in dys], [t.float() for t in xs]

    def run(fused_call):
        ws, bs = [w.clone() for w in w0], [b.clone() for b in b0]
        with ops.deferred_wgrad() as q:
            for dy, x, w, b in zip(dys, xs, ws, bs):
                if fused_call:
                    ops.linear_dw(dy, x, w, accumulate=True, db=b)
                else:
                    ops.colsum(dy, b)
                    ops.linear_dw(dy, x, w, accumulate=True)
            assert all(it[-2] is None for it in q.items)
            assert len(q.items) == (0 if mode == "f32" else 3)
        torch.cuda.synchronize()
        return ws + bs

    deferred.WGRAD_BIAS = mode != "switch_off"
    got = run(True)
    deferred.WGRAD_BIAS = True
    for a, b in zip(got, run(False)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------- a model
def test_model_switch_on_off(switches_on):
    """A tiny bf16 hybrid model (2 Conformer blocks, d = 64, 1 decoder block, B = 2, T = 70),
    one backward pass with the switch on and off: every bias within the queue test's bound
    (R = the fewest rows any bias sums, the decoder's tokens), everything else bit-equal."""
    import bench
    ops, L = _ops()
    deferred = switches_on
    cfg = bench.c3_config()
    cfg.update(vocab_size=50, B=2, T=70, L=5)
    cfg["encoder_conf"] = dict(cfg["encoder_conf"], output_size=64, attention_heads=4, linear_units=128,
                               num_blocks=2, cnn_module_kernel=15)
    cfg["decoder_conf"] = dict(cfg["decoder_conf"], attention_heads=4, linear_units=128, num_blocks=1)
    batch = {k: v.cuda() for k, v in bench.synthetic_batch(cfg, 3).items()}
    grads, carried = [], []
    add = deferred.WGRAD_Q.add

    def counting_add(*a, **k):
        r = add(*a, **k)
        carried[-1] += r == "db"
        return r

    deferred.WGRAD_Q.add = counting_add
    try:
        for on in (True, False):
            deferred.WGRAD_BIAS = on
            carried.append(0)
            m = bench.build(cfg)
            m.prepare(torch.device("cuda", 0), amp=True, seed=1234)
            m.train()
            loss, _, _ = m(**batch)
            with ops.deferred_wgrad():
                loss.backward()
            torch.cuda.synchronize()
            grads.append(m.arena.grad.clone())
    finally:
        del deferred.WGRAD_Q.add
    assert carried[0] >= 2 * 4 + 4 and carried[1] == 0, carried
    rows = cfg["B"] * (cfg["L"] + 1)
    a = m.arena
    for n in a.names:
        s = slice(a.offsets[n], a.offsets[n] + a._params[n].numel())
        on, off = grads[0][s], grads[1][s]
        assert torch.isfinite(on).all()
        if n.endswith(".bias"):
            torch.testing.assert_close(on, off, atol=1e-5 * rows ** 0.5, rtol=1e-5, msg=lambda t, n=n: f"{n}: {t}")
        else:
            assert torch.equal(on, off), n
