"""The two row kernels of the intermediate-CTC taps through the C ABI — ea_softmax_lse_rows
(log-sum-exp + softmax in the compute dtype) and ea_interctc_dlogits (CTC gradient fused with
the softmax backward of the conditioning branch) — against a float64 restatement in torch.

Shapes: (B,T) = (3,7) with hlens [7,4,1] and (1,1); V in {1, 50, 257, 5000} plus the first
sizes past the kernels' LDS-staging limits (12500: the forward's; 8200: the backward's for
both dtypes — it stages rows only when it has no CTC term, test_dlogits_without_a_loss), where
they take the re-reading path; dense rows (ld = V), rows V+3 apart (no row
base 16-B aligned, the element-wise path) and, for the new kernels alone, rows V+4 apart from a
base one element off alignment.  Logits are 4*randn: peaked rows whose smallest reference
probability stays above 1e-20.  Padding between rows is NaN on input and must be untouched on
output.
"""
import numpy as np
import pytest
import torch

from goldens import assert_grad_close

pytestmark = pytest.mark.gpu

SHAPES = {"b3t7": (3, 7, [7, 4, 1], [3, 2, 1]), "b1t1": (1, 1, [1], [1])}
VS = [1, 50, 257, 5000, 8200, 12500]
LAYOUTS = {"dense": (0, 0), "ld+3": (3, 0), "ld+4,off1": (4, 1)}  # (ld - V, base offset in elements)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
SENTINEL = -777.0


def _strided(rows, V, pad, off, dtype, fill):
    """(flat buffer, rows x V view with row stride V+pad starting `off` elements in)."""
    ld = V + pad
    buf = torch.full((off + rows * ld + 8,), fill, dtype=dtype, device="cuda")
    return buf, torch.as_strided(buf, (rows, V), (ld, 1), off)


def _pad_untouched(buf, view, fill):
    mask = torch.ones_like(buf, dtype=torch.bool)
    torch.as_strided(mask, view.shape, view.stride(), view.storage_offset()).fill_(False)
    return bool((buf[mask] == fill).all())


class Case:
    """Inputs of one (shape, V, layout) and its float64 references, built once."""

    def __init__(self, shape, V, layout):
        B, T, hlens, ylens = SHAPES[shape]
        pad, off = LAYOUTS[layout]
        g = torch.Generator().manual_seed(1000 * V + 10 * B + pad + off)
        self.B, self.T, self.V, self.pad, self.off = B, T, V, pad, off
        N = B * T
        x = 4.0 * torch.randn(N, V, generator=g)
        if V == 1:
            ylens = [0] * B
        self.Lmax = 3
        ys = torch.full((B, self.Lmax), -1, dtype=torch.long)
        for b, l in enumerate(ylens):
            ys[b, :l] = torch.randint(1, max(V, 2), (l,), generator=g)
        self.hl, self.yl, self.ys = torch.tensor(hlens), torch.tensor(ylens), ys
        self.xbuf, self.x = _strided(N, V, pad, off, torch.float32, float("nan"))
        self.x.copy_(x)
        self.dp_cpu = torch.randn(N, V, generator=g)
        self.gscale = 0.37
        # ---- float64 references
        x64 = x.double().requires_grad_(True)
        self.lse_ref = torch.logsumexp(x64.detach(), dim=1)
        self.p_ref = torch.exp(x64.detach() - self.lse_ref[:, None])
        lp = torch.log_softmax(x64.view(B, T, V), dim=-1).transpose(0, 1)
        tgt = torch.cat([ys[b, :ylens[b]] for b in range(B)])
        nll = torch.nn.CTCLoss(reduction="none", zero_infinity=True)(lp, tgt, self.hl, self.yl)
        (nll.sum() / B).backward()
        self.ctc_ref = x64.grad  # (1/B)(p - occupancy) on live rows, 0 on padded / infeasible ones
        self.padded = torch.tensor([t >= hlens[b] for b in range(B) for t in range(T)])

    def sm_ref(self, dtype):
        dp = self.dp_cpu.to(dtype).double()  # the values the kernel is given
        return self.p_ref * (dp - (self.p_ref * dp).sum(1, keepdim=True))

    # ---- kernel calls
    def lattice(self, lse_given=None):
        from espnet_amd import hip_ops as ops
        from espnet_amd._lib import lib
        B, T, V = self.B, self.T, self.V
        S = 2 * self.Lmax + 1
        dev = "cuda"
        z = dict(lse=torch.empty(B * T, device=dev), alpha=torch.empty(B * T * S, dtype=torch.float64, device=dev),
                 beta=torch.empty(B * T * S, dtype=torch.float64, device=dev),
                 nll=torch.empty(B, dtype=torch.float64, device=dev), lu=torch.empty(B, device=dev),
                 loss=torch.empty((), device=dev), hl=self.hl.to(dev), ys=self.ys.to(dev), yl=self.yl.to(dev))
        args = (B, T, V, self.x.data_ptr(), V + self.pad, z["hl"].data_ptr(), z["ys"].data_ptr(), self.Lmax,
                z["yl"].data_ptr(), self.Lmax)
        tail = (z["alpha"].data_ptr(), z["beta"].data_ptr(), z["nll"].data_ptr(), z["lu"].data_ptr(),
                z["loss"].data_ptr(), ops.stream())
        if lse_given is None:
            lib.ea_ctc_loss_fwd(*args, z["lse"].data_ptr(), *tail)
        else:
            z["lse"] = lse_given
            lib.ea_ctc_loss_fwd_lse(*args, lse_given.data_ptr(), *tail)
        return z

    def softmax(self, dtype):
        from espnet_amd import hip_ops as ops
        from espnet_amd._lib import lib
        N, V = self.B * self.T, self.V
        lse = torch.empty(N, device="cuda")
        pbuf, p = _strided(N, V, self.pad, self.off, dtype, SENTINEL)
        lib.ea_softmax_lse_rows(N, V, self.x.data_ptr(), V + self.pad, lse.data_ptr(), p.data_ptr(), ops.dt(p),
                                V + self.pad, ops.stream())
        torch.cuda.synchronize()
        assert _pad_untouched(pbuf, p, SENTINEL)
        return lse, p

    def dlogits(self, z, dtype, gscale, dp):
        """dp: 'zero' | 'rand' | None (NULL)."""
        from espnet_amd import hip_ops as ops
        from espnet_amd._lib import lib
        B, T, V = self.B, self.T, self.V
        N = B * T
        gs = torch.full((1,), gscale, device="cuda")
        obuf, out = _strided(N, V, self.pad, self.off, dtype, SENTINEL)
        dpt = None
        if dp is not None:
            _, dpt = _strided(N, V, self.pad, self.off, dtype, float("nan"))
            dpt.copy_(self.dp_cpu.to(dtype) if dp == "rand" else torch.zeros(N, V))
        lib.ea_interctc_dlogits(B, T, V, self.x.data_ptr(), V + self.pad, z["hl"].data_ptr(), z["ys"].data_ptr(),
                                self.Lmax, z["yl"].data_ptr(), self.Lmax, z["lse"].data_ptr(), z["alpha"].data_ptr(),
                                z["beta"].data_ptr(), z["nll"].data_ptr(), gs.data_ptr(), 1.0 / B, ops.ptr(dpt),
                                V + self.pad, out.data_ptr(), ops.dt(out), V + self.pad, ops.stream())
        torch.cuda.synchronize()
        assert _pad_untouched(obuf, out, SENTINEL)
        return out

    def ctc_bwd(self, z, dtype, gscale):
        from espnet_amd import hip_ops as ops
        from espnet_amd._lib import lib
        B, T, V = self.B, self.T, self.V
        gs = torch.full((1,), gscale, device="cuda")
        _, out = _strided(B * T, V, self.pad, self.off, dtype, SENTINEL)
        lib.ea_ctc_loss_bwd(B, T, V, self.x.data_ptr(), V + self.pad, z["hl"].data_ptr(), z["ys"].data_ptr(), self.Lmax,
                            z["yl"].data_ptr(), self.Lmax, z["lse"].data_ptr(), z["alpha"].data_ptr(),
                            z["beta"].data_ptr(), z["nll"].data_ptr(), gs.data_ptr(), 1.0 / B, out.data_ptr(),
                            ops.dt(out), V + self.pad, ops.stream())
        torch.cuda.synchronize()
        return out


_CASES = {}


def case(shape, V, layout):
    key = (shape, V, layout)
    if key not in _CASES:
        _CASES[key] = Case(*key)
    return _CASES[key]


ALL = [(s, V, l) for s in SHAPES for V in VS for l in LAYOUTS]
ABI_ALIGNED = [(s, V, l) for (s, V, l) in ALL if LAYOUTS[l][1] == 0]  # layouts ea_ctc_loss_* accept too


def _close(mine, ref, name, dtype):
    """assert_grad_close with tests/test_model_gpu.py's numbers; bf16 adds its rounding, 2^-8 |ref|."""
    extra = 2.0 ** -8 if dtype == torch.bfloat16 else 0.0
    assert_grad_close(mine.double().cpu().numpy(), ref.numpy(), name, rtol=2e-4 + extra, scale_tol=1e-5)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,V,layout", ALL)
def test_softmax_lse_rows(shape, V, layout, dt):
    c = case(shape, V, layout)
    dtype = DTYPES[dt]
    lse, p = c.softmax(dtype)
    if LAYOUTS[layout][1] == 0:  # the row reduction is ea_ctc_loss_fwd's own: bit-equal
        assert torch.equal(lse, c.lattice()["lse"])
    np.testing.assert_allclose(lse.double().cpu().numpy(), c.lse_ref.numpy(), rtol=2e-6)
    mine, ref = p.double().cpu().numpy(), c.p_ref.numpy()
    assert ref.min() > 1e-20
    print(f"{shape} V={V} {layout} {dt}: max rel err p {np.abs(mine / ref - 1).max():.3e}")
    if dtype == torch.float32:
        np.testing.assert_allclose(mine, ref, rtol=2e-4, atol=1e-12)
    else:
        assert (np.abs(mine - ref) <= 2.0 ** -8 * np.abs(ref)).all()
    lse2, p2 = c.softmax(dtype)
    assert torch.equal(lse, lse2) and torch.equal(p, p2)  # deterministic


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,V,layout", ABI_ALIGNED)
def test_lattice_with_given_lse_and_shared_ctc_term(shape, V, layout, dt):
    """ea_ctc_loss_fwd_lse on ea_softmax_lse_rows' lse gives ea_ctc_loss_fwd's lattice bit for
    bit, and with dp = 0 (and with dp NULL) the fused gradient is ea_ctc_loss_bwd's output."""
    c = case(shape, V, layout)
    dtype = DTYPES[dt]
    z = c.lattice()
    lse, _ = c.softmax(dtype)
    z2 = c.lattice(lse_given=lse)
    torch.cuda.synchronize()
    for k in ("nll", "lu", "loss"):
        assert torch.equal(z[k], z2[k]), k
    want = c.ctc_bwd(z, dtype, c.gscale)
    assert torch.equal(c.dlogits(z2, dtype, c.gscale, "zero"), want)
    assert torch.equal(c.dlogits(z2, dtype, c.gscale, None), want)
    if not torch.isinf(z["nll"]).any():
        _close(want, c.gscale * c.ctc_ref, "ctc term", dtype)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,V,layout", ALL)
def test_dlogits_softmax_term_and_both(shape, V, layout, dt):
    c = case(shape, V, layout)
    dtype = DTYPES[dt]
    lse, _ = c.softmax(dtype)
    z = c.lattice(lse_given=lse)
    sm = c.sm_ref(dtype)
    only_sm = c.dlogits(z, dtype, 0.0, "rand")
    _close(only_sm, sm, "softmax term (gscale 0)", dtype)
    both = c.dlogits(z, dtype, c.gscale, "rand")
    if not torch.isinf(z["nll"]).any():
        _close(both, c.gscale * c.ctc_ref + sm, "both terms", dtype)
    pad = c.padded.cuda()
    assert torch.equal(both[pad], only_sm[pad])  # padded rows: the softmax term alone
    assert torch.equal(both, c.dlogits(z, dtype, c.gscale, "rand"))  # deterministic


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("V,layout", [(257, "ld+3"), (5000, "dense"), (8200, "dense")])
def test_dlogits_without_a_loss(V, layout, dt):
    """alpha NULL (a tap that only conditions): the softmax term on every row.  This form keeps
    the row in LDS between its two passes where it fits (V = 8200 does not)."""
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    c = case("b3t7", V, layout)
    dtype = DTYPES[dt]
    lse, _ = c.softmax(dtype)
    N, V, ld = c.B * c.T, c.V, c.V + c.pad
    _, dp = _strided(N, V, c.pad, 0, dtype, float("nan"))
    dp.copy_(c.dp_cpu.to(dtype))
    obuf, out = _strided(N, V, c.pad, 0, dtype, SENTINEL)
    lib.ea_interctc_dlogits(c.B, c.T, V, c.x.data_ptr(), ld, None, None, 0, None, 0, lse.data_ptr(), None, None, None,
                            None, 0.0, dp.data_ptr(), ld, out.data_ptr(), ops.dt(out), ld, ops.stream())
    torch.cuda.synchronize()
    assert _pad_untouched(obuf, out, SENTINEL)
    _close(out, c.sm_ref(dtype), "softmax term, no lattice", dtype)
