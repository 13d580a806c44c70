"""The decoder / loss-end kernels that only whole-model goldens reached, through the C-ABI against
float64 torch on the CPU: ea_lsm_loss_bwd, ea_embed_fwd / ea_embed_bwd, ea_softmax_rows,
ea_argmax_rows, ea_add_sos_eos, ea_subsample_lens.

Integer outputs, masks, zeros, sentinels and untouched buffers are compared exactly.  f32 outputs
get 8x the f32 noise floor (the same formula in f32 torch against f64 on the tests' own inputs,
f32_floors() below), relative to the size of the operands of the last cancelling operation:
  lsm bwd   grad = g * (p - q):      |err| <= LSM_BOUND * |g| * (p + q)   (floor: g * (softmax - q) in
            f32, the kernel's formula, checked in f64 to be the oracle's autograd gradient)
            floor 7.4e-7, bound 5.9e-6, kernel worst 1.3e-6
  embed bwd dE += sum of terms:      |err| <= EMB_BOUND * (|dE0| + sum |terms|)
            floor 1.8e-7, bound 1.4e-6, kernel worst 2.0e-7
  softmax   p:                       |err| <= SM_BOUND * (p + 1e-4 / V)
            floor 7.4e-7, bound 5.9e-6, kernel worst 6.4e-7
  log_softmax:                       |err| <= LOGSM_BOUND * (|logp| + 1)
            floor 1.0e-7, bound 8.1e-7, kernel worst 1.1e-7 (3.6e-6 by f32 emulation of the
            earlier x - (m + log(sum)); the kernel now subtracts m, then log(sum), as torch does)
bf16 outputs add 2^-8 * |ref|.
"""
import numpy as np
import pytest
import torch

LSM_BOUND = 5.9e-6
EMB_BOUND = 1.4e-6
SM_BOUND = 5.9e-6
LOGSM_BOUND = 8.1e-7
BF16 = 2.0 ** -8
SENT = -7.25

LSM_SHAPES = [(9, 4, 4, 4), (64, 301, 303, 304), (77, 5000, 5000, 5000)]
EMB_BWD = [(1, 4), (255, 260), (256, 260), (257, 260), (1312, 260), (4096, 260)]
SM_V = [1, 2, 255, 256, 257, 5000]
ARGMAX_V = [1, 5, 63, 64, 65, 100, 300, 5000]
NEG_INF = float("-inf")


# ------------------------------------------------------------------ label smoothing backward
def lsm_case(rows, V, ldx):
    g = torch.Generator().manual_seed(rows + V)
    x = torch.randn(rows, ldx, generator=g) * 3
    tgt = torch.randint(0, V, (rows,), generator=g)
    tgt[::7] = -1  # ignore_id
    tgt[1], tgt[2] = 0, V - 1
    batch = {9: 3, 64: 4, 77: 7}[rows]
    return x, tgt, batch


def lsm_grad_ref(x, tgt, batch, V, sm, norm_len, g, dtype=torch.float64):
    """Autograd of the oracle's loss w.r.t. the logits, times g; and p + q (the error's scale)."""
    from oracle.asr_oracle import label_smoothing_loss
    xv = x[:, :V].to(dtype).clone().requires_grad_(True)
    label_smoothing_loss(xv.view(batch, -1, V), tgt.view(batch, -1), sm, -1, norm_len).backward()
    valid = (tgt != -1)[:, None]
    q = torch.full((len(tgt), V), sm / (V - 1), dtype=torch.float64)
    q.scatter_(1, tgt.clamp(min=0)[:, None], 1 - sm)
    denom = int(valid.sum()) if norm_len else batch
    den = abs(g) / denom * (torch.softmax(x[:, :V].double(), -1) + q) * valid
    return xv.grad * g, den


def lsm_grad_formula(x, tgt, batch, V, sm, norm_len, g, dtype):
    """The kernel's formula g / denom * (softmax(x) - q), 0 on ignored rows, in `dtype`."""
    valid = (tgt != -1)[:, None]
    q = torch.full((len(tgt), V), sm / (V - 1), dtype=dtype)
    q.scatter_(1, tgt.clamp(min=0)[:, None], 1 - sm)
    denom = int(valid.sum()) if norm_len else batch
    k = torch.tensor(g, dtype=dtype) * (torch.tensor(1.0, dtype=dtype) / denom)
    return k * (torch.softmax(x[:, :V].to(dtype), -1) - q) * valid


@pytest.mark.gpu
@pytest.mark.parametrize("rows,V,ldx,ldg", LSM_SHAPES)
@pytest.mark.parametrize("norm_len", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lsm_loss_bwd_matches_f64_autograd(rows, V, ldx, ldg, norm_len, dtype):
    """Kernel worst error (f32 grad) 1.3e-6 of LSM_BOUND = 5.9e-6."""
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import dt, lib
    x, tgt, batch = lsm_case(rows, V, ldx)
    sm, gscale, coef = 0.1, 0.7, 1.3
    xd, td = x.cuda(), tgt.cuda()
    lse = torch.empty(rows, device="cuda")
    loss_row = torch.empty(rows, dtype=torch.float64, device="cuda")
    stat = torch.empty(2, dtype=torch.int32, device="cuda")
    loss, acc, inv = (torch.empty(1, device="cuda") for _ in range(3))
    lib.ea_lsm_loss_fwd(rows, V, xd.data_ptr(), ldx, td.data_ptr(), sm, -1, norm_len, float(batch), lse.data_ptr(),
                        loss_row.data_ptr(), stat.data_ptr(), loss.data_ptr(), acc.data_ptr(), inv.data_ptr(),
                        ops.stream())
    gs = torch.tensor([gscale], device="cuda")
    grad = torch.full((rows, ldg), float("nan"), dtype=dtype, device="cuda")
    lib.ea_lsm_loss_bwd(rows, V, xd.data_ptr(), ldx, td.data_ptr(), sm, -1, lse.data_ptr(), gs.data_ptr(),
                        inv.data_ptr(), coef, grad.data_ptr(), dt(grad), ldg, ops.stream())
    torch.cuda.synchronize()
    grad = grad.cpu()
    ref, den = lsm_grad_ref(x, tgt, batch, V, sm, norm_len, gscale * coef)
    got = grad[:, :V].double()
    ign = tgt == -1
    assert int(ign.sum()) > 0
    assert torch.equal(got[ign], torch.zeros(int(ign.sum()), V, dtype=torch.float64))  # exactly 0 over the NaN
    assert bool(grad[:, V:].isnan().all())  # padding untouched
    tol = LSM_BOUND * den + (BF16 * ref.abs() if dtype == torch.bfloat16 else 0)
    err = ((got - ref).abs() / (den + 1e-300)).max().item()
    if dtype == torch.float32:
        print(f"lsm_loss_bwd rows={rows} V={V} norm_len={norm_len}: err {err:.3g}")
    assert bool(((got - ref).abs() <= tol).all()), err


# ------------------------------------------------------------------ embeddings
def fma_f32(a, b, c):
    """round_to_f32(a * b + c) of f32 tensors with ONE rounding, as a hardware fused multiply-add.
    The product of two f32 is exact in f64; the f64 sum is turned into round-to-odd with the
    two-sum residual, so the final cast to f32 cannot round twice."""
    p, c = a.double() * b.double(), c.double()
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)  # exact: p + c == s + e
    odd = (s.view(torch.int64) & 1) == 1
    toward = torch.where(e > 0, torch.full_like(s, float("inf")), torch.full_like(s, NEG_INF))
    return torch.where((e != 0) & ~odd, torch.nextafter(s, toward), s).float()


def embed_fwd_ref(E, tok, pe, L, xscale):
    """E[tok] * xscale + pe[r % L] in f32 as the kernel evaluates it: the multiply and the add are
    one FMA (rounded once).  torch rounds the product first and can differ in the last bit."""
    rows = len(tok)
    return fma_f32(E[tok], torch.tensor(xscale, dtype=E.dtype), pe[torch.arange(rows) % L])


def test_fma_f32_rounds_once():
    """1 + 2^-24 + 2^-60 lies just above an f32 tie: one rounding gives 1 + 2^-23, the f64 sum
    cast to f32 (two roundings) gives 1."""
    a, b, c = torch.tensor([4097.0]), torch.tensor([16773121.0 * 2.0 ** -60]), torch.tensor([1.0])
    assert (a.double() * b.double()).item() == 2.0 ** -24 + 2.0 ** -60
    assert fma_f32(a, b, c).item() == 1.0 + 2.0 ** -23
    assert (a.double() * b.double() + c.double()).float().item() == 1.0
    g = torch.Generator().manual_seed(1)
    x, y, z = (torch.randn(4096, generator=g) for _ in range(3))
    exact = x.double() * y.double() + z.double()  # off by at most half an f64 ulp
    assert bool(((fma_f32(x, y, z).double() - exact).abs() <= 2.0 ** -24 * exact.abs() * (1 + 2.0 ** -20)).all())


def embed_scatter_ref(dE0, tok, terms):
    """dE0 (V, d), terms (rows, d) -> dE0 with terms[r] added into row tok[r]; and the sum of
    absolute values, which an f32 error is relative to."""
    out, den = dE0.clone(), dE0.abs()
    out.index_add_(0, tok, terms)
    den.index_add_(0, tok, terms.abs())
    return out, den


def mask_rows(mask_flat, rows, d):
    """The keep mask of element (r, c) lives at index r*d + c, forward and backward."""
    return mask_flat.view(rows, d)


def token_patterns(rows, V, g):
    base = lambda: torch.randint(10, V, (rows,), generator=g)  # noqa: E731
    placed = base()
    placed[[r for r in (0, 255, 256, 511, rows - 1) if r < rows]] = 5
    late = base()
    late[rows - 1] = 7  # a token whose first occurrence is the last row
    return {"same": torch.full((rows,), 3), "distinct": torch.randperm(V, generator=g)[:rows],
            "placed": placed, "late": late, "random": torch.randint(0, min(40, V), (rows,), generator=g)}


def embed_bwd_case(rows, d):
    g = torch.Generator().manual_seed(rows * 7 + d)
    V = rows + 16
    dy = torch.randn(rows, d, generator=g)
    dE0 = torch.randn(V, d, generator=g)
    return V, dy, dE0, token_patterns(rows, V, g)


def run_embed_bwd(tok, dy, dE0, xscale, p=0.0, seed=0):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    rows, d = dy.shape
    assert 0 <= int(tok.min()) and int(tok.max()) < dE0.shape[0] and len(tok) == rows
    dE, td, dyd = dE0.cuda(), tok.cuda(), dy.cuda()
    lib.ea_embed_bwd(rows, d, td.data_ptr(), dyd.data_ptr(), xscale, float(p), seed, dE.data_ptr(), ops.stream())
    torch.cuda.synchronize()
    return dE.cpu()


def run_embed_fwd(tok, E, pe, L, xscale, p=0.0, seed=0):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    rows, d = len(tok), E.shape[1]
    assert 0 <= int(tok.min()) and int(tok.max()) < E.shape[0] and pe.shape == (L, d)
    y = torch.full((rows + 1, d), SENT, device="cuda")  # one guard row
    Ed, ped, td = E.cuda(), pe.cuda(), tok.cuda()
    lib.ea_embed_fwd(rows, d, L, td.data_ptr(), Ed.data_ptr(), xscale, ped.data_ptr(), float(p), seed, y.data_ptr(),
                     ops.stream())
    torch.cuda.synchronize()
    y = y.cpu()
    assert torch.equal(y[rows], torch.full((d,), SENT))
    return y[:rows]


def test_embed_scatter_ref_matches_embedding_autograd():
    g = torch.Generator().manual_seed(5)
    V, d, rows = 23, 6, 300
    tok = torch.randint(0, V, (rows,), generator=g)
    dy = torch.randn(rows, d, generator=g, dtype=torch.float64)
    E = torch.randn(V, d, generator=g, dtype=torch.float64, requires_grad=True)
    (torch.nn.functional.embedding(tok, E) * 1.5 * dy).sum().backward()
    ours, _ = embed_scatter_ref(torch.zeros(V, d, dtype=torch.float64), tok, dy * 1.5)
    torch.testing.assert_close(ours, E.grad, rtol=1e-13, atol=1e-13)
    used = torch.zeros(V, dtype=torch.bool)
    used[tok] = True
    assert torch.equal(ours[~used], torch.zeros(int((~used).sum()), d, dtype=torch.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("d,L,rows,xscale", [(4, 7, 45, 1.7), (256, 7, 45, 1.7), (256, 3, 2, 16.0), (4, 1, 300, 2.0)])
def test_embed_fwd_bit_exact(d, L, rows, xscale):
    """p = 0: y = E[tok] * xscale + pe[r % L] bit-exact against the same f32 expression evaluated as
    the kernel does, multiply and add fused (embed_fwd_ref); and within the rounding of the product
    of torch's unfused f32 expression."""
    g = torch.Generator().manual_seed(d + rows)
    V = 50
    E, pe = torch.randn(V, d, generator=g), torch.randn(L, d, generator=g)
    tok = torch.randint(0, V, (rows,), generator=g)
    tok[0], tok[rows - 1] = V - 1, 0
    y = run_embed_fwd(tok, E, pe, L, xscale)
    assert torch.equal(y, embed_fwd_ref(E, tok, pe, L, xscale))
    prod = E[tok] * torch.tensor(xscale)
    unfused = prod + pe[torch.arange(rows) % L]
    assert bool(((y - unfused).abs().double() <= 2.0 ** -23 * (prod.abs() + y.abs()).double()).all())


@pytest.mark.gpu
@pytest.mark.parametrize("rows,d", EMB_BWD)
def test_embed_bwd_matches_f64_scatter(rows, d):
    """Accumulates into a random dE; every token pattern; two runs bit-equal; unused token rows
    unchanged.  Kernel worst error 2.0e-7 of EMB_BOUND = 1.4e-6."""
    V, dy, dE0, pats = embed_bwd_case(rows, d)
    xscale = 1.7
    worst = 0.0
    for name, tok in pats.items():
        got = run_embed_bwd(tok, dy, dE0, xscale)
        assert torch.equal(run_embed_bwd(tok, dy, dE0, xscale), got), name  # bit-reproducible
        ref, den = embed_scatter_ref(dE0.double(), tok, dy.double() * xscale)
        used = torch.zeros(V, dtype=torch.bool)
        used[tok] = True
        assert torch.equal(got[~used], dE0[~used]), name
        err = ((got.double() - ref).abs() / den).max().item()
        worst = max(worst, err)
        assert err <= EMB_BOUND, (name, err)
    print(f"embed_bwd rows={rows} d={d}: worst err {worst:.3g}")


@pytest.mark.gpu
def test_embed_bwd_row_limit_is_4096():
    """The documented ceiling (rows <= 4096: the token table lives in LDS): one more row is
    refused and nothing is written."""
    from espnet_amd._lib import HipError
    rows, d = 4097, 4
    dE0 = torch.randn(20, d)
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    dE, td, dyd = dE0.cuda(), torch.zeros(rows, dtype=torch.int64).cuda(), torch.ones(rows, d).cuda()
    with pytest.raises(HipError, match="bad argument"):
        lib.ea_embed_bwd(rows, d, td.data_ptr(), dyd.data_ptr(), 1.0, 0.0, 0, dE.data_ptr(), ops.stream())
    torch.cuda.synchronize()
    assert torch.equal(dE.cpu(), dE0)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,d,L", [(257, 36, 11), (1312, 256, 41)])
def test_embed_dropout_mask_is_shared_by_fwd_and_bwd(rows, d, L):
    g = torch.Generator().manual_seed(rows)
    V, p, seed, xscale = 60, 0.1, 4242, 1.7
    E, pe = torch.randn(V, d, generator=g), torch.randn(L, d, generator=g)
    tok = torch.randint(0, V, (rows,), generator=g)
    undropped = embed_fwd_ref(E, tok, pe, L, xscale)
    assert bool((undropped != 0).all())  # so the mask is recovered everywhere
    y = run_embed_fwd(tok, E, pe, L, xscale, p=p, seed=seed)
    keep = y != 0
    np.testing.assert_allclose(y[keep].numpy(), (undropped[keep].double() / (1 - p)).numpy(), rtol=1e-6, atol=0)
    n, q = rows * d, 1 - round(p * 65536) / 65536
    assert abs(int(keep.sum()) - n * q) <= 6 * (n * q * (1 - q)) ** 0.5
    assert torch.equal(run_embed_fwd(tok, E, pe, L, xscale, p=p, seed=seed), y)
    assert not torch.equal(run_embed_fwd(tok, E, pe, L, xscale, p=p, seed=seed + 1) != 0, keep)
    dy, dE0 = torch.randn(rows, d, generator=g), torch.randn(V, d, generator=g)
    mask = mask_rows(keep.reshape(-1), rows, d).double()
    ref, den = embed_scatter_ref(dE0.double(), tok, dy.double() * xscale * mask / (1 - p))
    got = run_embed_bwd(tok, dy, dE0, xscale, p=p, seed=seed)
    err = ((got.double() - ref).abs() / den).max().item()
    assert err <= EMB_BOUND, err
    nomask, _ = embed_scatter_ref(dE0.double(), tok, dy.double() * xscale)
    assert float((got.double() - nomask).abs().max()) > 1e-2


# ------------------------------------------------------------------ softmax rows
def softmax_rows_case(V):
    g = torch.Generator().manual_seed(V)
    x = torch.randn(6, V + 3, generator=g) * 3
    x[1] += 80
    x[2] -= 80
    hole = torch.rand(V, generator=g) < 0.3
    hole[V // 2] = False  # keep one finite entry
    x[3, :V][hole] = NEG_INF
    x[4, :V][hole] = NEG_INF
    x[4] += 80
    x[:, V:] = float("nan")  # the padding columns are never read
    return x


def softmax_rows_errs(got, ref, log, V):
    fin = torch.isfinite(ref)
    assert torch.equal(got.double()[~fin], ref[~fin])  # log(0) = -inf exactly
    a = 1.0 if log else 1e-4 / V
    return ((got.double() - ref).abs()[fin] / (ref.abs()[fin] + a)).max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("V", SM_V)
@pytest.mark.parametrize("log", [0, 1])
def test_softmax_rows_matches_f64(V, log):
    """Rows offset by +-80 and rows with -inf entries (softmax exactly 0, log_softmax exactly -inf).
    Kernel worst error: softmax 6.4e-7 of SM_BOUND = 5.9e-6,
    log_softmax 1.1e-7 of LOGSM_BOUND = 8.1e-7."""
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    x = softmax_rows_case(V)
    rows = x.shape[0]
    xd = x.cuda()
    out = torch.full((rows + 1, V), SENT, device="cuda")
    lib.ea_softmax_rows(rows, V, xd.data_ptr(), V + 3, out.data_ptr(), log, ops.stream())
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.equal(out[rows], torch.full((V,), SENT))
    xv = x[:, :V].double()
    ref = torch.log_softmax(xv, -1) if log else torch.softmax(xv, -1)
    err = softmax_rows_errs(out[:rows], ref, log, V)
    print(f"softmax_rows V={V} log={log}: err {err:.3g}")
    assert err <= (LOGSM_BOUND if log else SM_BOUND), err
    if not log:
        assert torch.equal(out[:rows][xv == NEG_INF], torch.zeros(int((xv == NEG_INF).sum())))


# ------------------------------------------------------------------ argmax rows
def argmax_ref(x):
    """torch.argmax: the first maximal index; a NaN is maximal."""
    return torch.argmax(x, -1)


def argmax_rows_case(V):
    g = torch.Generator().manual_seed(V)
    rows = [torch.randn(V, generator=g) for _ in range(3)]
    last = torch.randn(V, generator=g)
    last[V - 1] = 9.0  # maximum in the last column
    rows += [last, torch.full((V,), 0.25), torch.full((V,), NEG_INF)]
    for a, b in [(70, 6), (6, 70), (200, 9), (V - 1, 0), (V - 1, V // 2), (129, 64)]:
        if max(a, b) < V and a != b:
            t = torch.randn(V, generator=g).clamp(max=3.0)
            t[a] = t[b] = 5.0  # equal maxima: other lanes, other 64-strides
            rows.append(t)
    for nans in [(5,), (70, 6), (V - 1,), (131, 200), (64, 1), (0,)]:
        if max(nans) < V:
            t = torch.randn(V, generator=g)
            t[list(nans)] = float("nan")
            if V > 3:
                t[3] = float("inf")  # a NaN beats +inf too
            rows.append(t)
    x = torch.full((len(rows), V + 3), float("inf"))  # the padding columns would win if read
    x[:, :V] = torch.stack(rows)
    return x


def test_argmax_case_expectations():
    """The cases the kernel once got wrong, pinned on the reference side."""
    x = torch.randn(100)
    x[5] = float("nan")
    assert int(argmax_ref(x)) == 5
    x = torch.randn(300)
    x[[70, 6]] = float("nan")
    assert int(argmax_ref(x)) == 6
    x = torch.zeros(300)
    x[[70, 6]] = 1.0
    assert int(argmax_ref(x)) == 6
    assert int(argmax_ref(torch.full((9,), NEG_INF))) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("V", ARGMAX_V)
def test_argmax_rows_matches_torch(V):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    x = argmax_rows_case(V)
    rows = x.shape[0]
    xd = x.cuda()
    out = torch.full((rows + 1,), -5, dtype=torch.int64, device="cuda")
    lib.ea_argmax_rows(rows, V, xd.data_ptr(), V + 3, out.data_ptr(), ops.stream())
    torch.cuda.synchronize()
    out = out.cpu()
    assert int(out[rows]) == -5
    assert out[:rows].tolist() == argmax_ref(x[:, :V]).tolist()


# ------------------------------------------------------------------ add_sos_eos, subsample_lens
@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 40, 300])
def test_add_sos_eos_matches_oracle(L):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    from oracle.asr_oracle import add_sos_eos
    g = torch.Generator().manual_seed(L)
    B, ldys, V = 5, L + 5, 50
    ylens = torch.tensor([L, 0, L // 2, 1, max(L - 1, 0)])
    ys = torch.full((B, ldys), 777)  # stride padding: never read
    ys[:, :L] = torch.randint(1, V - 1, (B, L), generator=g)
    for b in range(B):
        ys[b, int(ylens[b]):L] = -1
    sos, eos, ign = V - 1, V - 2, -1
    yd, ld = ys.cuda(), ylens.cuda()
    ys_in = torch.full((B + 1, L + 1), -9, dtype=torch.int64, device="cuda")
    ys_out = torch.full((B + 1, L + 1), -9, dtype=torch.int64, device="cuda")
    in_lens = torch.full((B + 1,), -9, dtype=torch.int64, device="cuda")
    lib.ea_add_sos_eos(B, L, yd.data_ptr(), ldys, ld.data_ptr(), sos, eos, ign, ys_in.data_ptr(), ys_out.data_ptr(),
                       in_lens.data_ptr(), ops.stream())
    torch.cuda.synchronize()
    ref_in, ref_out = add_sos_eos(ys[:, :L], ylens, sos, eos, ign)
    assert torch.equal(ys_in.cpu()[:B], ref_in)
    assert torch.equal(ys_out.cpu()[:B], ref_out)
    assert torch.equal(in_lens.cpu()[:B], ylens + 1)
    for t in (ys_in, ys_out, in_lens):
        assert bool((t.cpu()[B] == -9).all())


@pytest.mark.gpu
@pytest.mark.parametrize("T", [7, 8, 9, 10, 11, 100])
def test_subsample_lens_exhaustive(T):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    from oracle.asr_oracle import subsample_lens
    ilens = torch.arange(0, T + 1)
    B = T + 1
    idev = ilens.cuda()
    olens = torch.full((B + 1,), -9, dtype=torch.int64, device="cuda")
    lib.ea_subsample_lens(B, T, idev.data_ptr(), olens.data_ptr(), ops.stream())
    torch.cuda.synchronize()
    assert olens.cpu()[:B].tolist() == subsample_lens(ilens, T).tolist()
    assert int(olens[B]) == -9


def f32_floors():
    """Worst error of the f32 torch evaluation of the same formulas on the tests' own inputs."""
    out = {"lsm": 0.0, "emb": 0.0, "sm": 0.0, "logsm": 0.0}
    for rows, V, ldx, _ in LSM_SHAPES:
        x, tgt, batch = lsm_case(rows, V, ldx)
        for nl in (0, 1):
            ref, den = lsm_grad_ref(x, tgt, batch, V, 0.1, nl, 0.91)
            f32 = lsm_grad_formula(x, tgt, batch, V, 0.1, nl, 0.91, torch.float32)
            f64 = lsm_grad_formula(x, tgt, batch, V, 0.1, nl, 0.91, torch.float64)
            assert float(((f64 - ref).abs() / (den + 1e-300)).max()) < 1e-13  # the formula is the oracle's gradient
            out["lsm"] = max(out["lsm"], ((f32.double() - ref).abs() / (den + 1e-300)).max().item())
    for rows, d in EMB_BWD:
        V, dy, dE0, pats = embed_bwd_case(rows, d)
        for tok in pats.values():
            ref, den = embed_scatter_ref(dE0.double(), tok, dy.double() * 1.7)
            f32, _ = embed_scatter_ref(dE0, tok, dy * 1.7)
            out["emb"] = max(out["emb"], ((f32.double() - ref).abs() / den).max().item())
    for V in SM_V:
        xv = softmax_rows_case(V)[:, :V]
        out["sm"] = max(out["sm"], softmax_rows_errs(torch.softmax(xv, -1), torch.softmax(xv.double(), -1), 0, V))
        out["logsm"] = max(out["logsm"], softmax_rows_errs(torch.log_softmax(xv, -1),
                                                            torch.log_softmax(xv.double(), -1), 1, V))
    return out


if __name__ == "__main__":
    print(f32_floors())
