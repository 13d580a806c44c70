"""The transducer kernels (csrc/transducer.hip) against a plain float64 restatement on the CPU:
log_softmax of the joint output, the alpha recursion written as two loops, autograd.  bf16: rd rounds a
product's operand in the forward (h, W_out) and passes the gradient through; GradRound rounds a gradient
the backward stores in bf16 (dlogits).  Tolerance (tests/lstm_train_goldens.py, MARGIN 4): 4 x err or 4 f32
ulps at the array's magnitude, err = max |f32 - f64| of this restatement run in float32.  Every compared
array is stored in f32, so none gets a bf16 step on top."""
import functools

import numpy as np
import pytest
import torch

from lstm_train_goldens import tolerance

pytestmark = pytest.mark.gpu
MARGIN, DT = 4, {"f32": torch.float32, "bf16": torch.bfloat16}
# (B, T, Umax, V, J) -> (t_len, u_len): every utterance but the first is shorter than T and Umax
SHAPES = {(1, 1, 0, 5, 8): ([1], [0]),
          (3, 7, 5, 37, 40): ([7, 4, 5], [5, 0, 3]),
          (2, 9, 6, 300, 72): ([9, 6], [6, 4]),
          (2, 40, 12, 130, 640): ([40, 33], [12, 7])}


_ids = "b%dt%du%dv%dj%d".__mod__
_bf = lambda t: t.float().to(torch.bfloat16).to(t.dtype)  # noqa: E731


def rd(t, amp):
    return t + (_bf(t) - t).detach() if amp else t


class GradRound(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, amp):
        ctx.amp = amp
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return (_bf(g) if ctx.amp else g), None


@functools.lru_cache(maxsize=None)
def inputs(shape, scale=1.0):
    B, T, U, V, J = shape
    g = torch.Generator().manual_seed(sum(shape))
    E, D = torch.randn(B, T, J, generator=g) * 0.7, torch.randn(B, U + 1, J, generator=g) * 0.7
    W = torch.randn(V, J, generator=g) * (scale * 2.0 / J ** 0.5)
    b = torch.randn(V, generator=g) * (0.3 * scale)
    y = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32)
    if V == 300:  # labels from the last N-tile and from column 1
        y[0] = torch.tensor([1, 299, 257, 1, 280, 299], dtype=torch.int32)
    tl, ul = (torch.tensor(v, dtype=torch.int32) for v in SHAPES.get(shape, ([T] * B, [U] * B)))  # (default: full)
    return E, D, W, b, y, tl, ul


def lattice_dp(lpb, lpl, Tl, Ul, back=False):  # alpha (beta when back) of one utterance, two loops
    a = [[None] * (Ul + 1) for _ in range(Tl)]
    for t in (range(Tl - 1, -1, -1) if back else range(Tl)):
        for u in (range(Ul, -1, -1) if back else range(Ul + 1)):
            if back:
                p = a[t + 1][u] + lpb[t, u] if t + 1 < Tl else None
                q = a[t][u + 1] + lpl[t, u] if u < Ul else None
                first = lpb[t, u]
            else:
                p = a[t - 1][u] + lpb[t - 1, u] if t else None
                q = a[t][u - 1] + lpl[t, u - 1] if u else None
                first = lpb.new_zeros(())
            a[t][u] = first if p is None and q is None else p if q is None else q if p is None else torch.logaddexp(p, q)
    return torch.stack([torch.stack(r) for r in a])


def rnnt_loss(logits, y, tl, ul):  # (B, T, U1, V) logits -> (batch-mean loss, lp_blank, lp_label)
    lp = torch.log_softmax(logits, dim=-1)
    B, T, U1, _ = lp.shape
    yl = torch.cat([y.long(), torch.zeros(B, 1, dtype=torch.long)], dim=1)
    lpb, lpl = lp[..., 0], lp.gather(3, yl[:, None, :, None].expand(B, T, U1, 1))[..., 0]
    ll = [lattice_dp(lpb[i], lpl[i], int(tl[i]), int(ul[i]))[-1, -1] + lpb[i, int(tl[i]) - 1, int(ul[i])] for i in range(B)]
    return -torch.stack(ll).sum() / B, lpb, lpl


@functools.lru_cache(maxsize=None)
def restate(shape, amp, dtype, scale=1.0):
    E, D, W, b, y, tl, ul = inputs(shape, scale)
    E, D, W, b = (v.to(dtype).clone().requires_grad_(True) for v in (E, D, W, b))
    h = torch.tanh(E[:, :, None, :] + D[:, None, :, :])  # (B, T, U1, J)
    logits = GradRound.apply(rd(h, amp) @ rd(W, amp).t() + b, amp)
    loss, lpb, lpl = rnnt_loss(logits, y, tl, ul)
    loss.backward()
    return dict(lse=torch.logsumexp(logits.detach(), dim=-1), lpb=lpb.detach(), lpl=lpl.detach(), loss=loss.detach(),
                dE=E.grad, dD=D.grad, dW=W.grad, db=b.grad)


def close(name, got, ref, r32):
    tol = tolerance(ref, float((r32.double() - ref).abs().max()), MARGIN)
    dev = float((got.detach().double().cpu() - ref).abs().max())
    print(f"{name}: dev {dev:.3e} tol {tol:.3e}")
    assert dev <= tol, (name, dev, tol)  # (a NaN fails it too)
    return tol


def check(name, got, shape, amp, scale=1.0, sel=...):
    ref, r32 = (restate(shape, amp, d, scale)[name] for d in (torch.float64, torch.float32))
    close(name, got.cpu()[sel], ref[sel], r32[sel])


@pytest.mark.parametrize("cd", DT)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_joint_lse(shape, cd):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import dt, lib
    B, T, U, V, J = shape
    E, D, W, b, y, tl, ul = (v.cuda() for v in inputs(shape))
    w = W.to(DT[cd])
    out = torch.full((3, B, T, U + 1), float("nan"), device="cuda")
    lib.ea_rnnt_joint_lse(dt(w), B, T, U + 1, V, J, E.data_ptr(), D.data_ptr(), w.data_ptr(), J, b.data_ptr(),
                          y.data_ptr(), tl.data_ptr(), ul.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                          out[2].data_ptr(), ops.stream())
    t, u = torch.arange(T)[None, :, None], torch.arange(U + 1)[None, None, :]
    live = (t < tl.cpu()[:, None, None]) & (u <= ul.cpu()[:, None, None])
    assert torch.isnan(out.cpu()[:, ~live]).all()  # padding nodes store nothing
    has_label = live & (u < ul.cpu()[:, None, None])
    check("lse", out[0], shape, cd == "bf16", sel=live)
    check("lpb", out[1], shape, cd == "bf16", sel=live)
    if has_label.any():
        check("lpl", out[2], shape, cd == "bf16", sel=has_label)


# (T, Umax, t_len, u_len): t_len = 1; u_len = 0 and u_len = Umax; U1 wider than the block; a long T
@pytest.mark.parametrize("T,U,tl,ul", [(4, 3, [1, 4], [3, 2]), (5, 3, [5, 3], [0, 3]), (3, 300, [3, 2], [300, 157]),
                                       (300, 2, [300, 211], [2, 1])], ids=["tlen1", "ulen0", "t3u300", "t300u2"])
def test_lattice(T, U, tl, ul):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import lib
    B = len(tl)
    g = torch.Generator().manual_seed(T * 1000 + U)
    lp = torch.log_softmax(torch.randn(B, T, U + 1, 3, generator=g, dtype=torch.float64) * 2, dim=-1)
    lpb, lpl = lp[..., 0].contiguous(), lp[..., 1].contiguous()
    tld, uld = torch.tensor(tl, dtype=torch.int32).cuda(), torch.tensor(ul, dtype=torch.int32).cuda()
    buf, co = torch.zeros(2, B, T, U + 1, dtype=torch.float64, device="cuda"), torch.zeros(3, B, T, U + 1, device="cuda")
    pb, pl = lpb.float().cuda(), lpl.float().cuda()
    ll, loss = torch.zeros(B, dtype=torch.float64, device="cuda"), torch.zeros((), device="cuda")
    lib.ea_rnnt_lattice(B, T, U + 1, pb.data_ptr(), pl.data_ptr(), tld.data_ptr(), uld.data_ptr(), buf[0].data_ptr(),
                        buf[1].data_ptr(), ll.data_ptr(), co[0].data_ptr(), co[1].data_ptr(), co[2].data_ptr(),
                        loss.data_ptr(), ops.stream())
    buf, ll = buf.cpu(), ll.cpu()
    for i in range(B):
        Tl, Ul = tl[i], ul[i]
        ref, r32 = ([lattice_dp(pb[i].cpu().to(d), pl[i].cpu().to(d), Tl, Ul, back) for back in (False, True)]
                    for d in (torch.float64, torch.float32))
        for k, name in enumerate(("alpha", "beta")):
            tol = close(f"{name}[{i}]", buf[k, i, :Tl, :Ul + 1], ref[k], r32[k])
        assert abs(float(ll[i] - ref[1][0, 0])) <= tol
        assert abs(float(buf[0, i, Tl - 1, Ul] + pb[i, Tl - 1, Ul].double().cpu() - ll[i])) <= tol
    assert abs(float(loss) + float(ll.sum()) / B) <= 4 * np.spacing(np.float32(abs(float(ll.sum()) / B)))


def run_node(shape, cd, cap, scale=1.0):
    from espnet_amd.asr.joint_network import RNNTJointLossFn
    E, D, W, b, y, tl, ul = (v.cuda() for v in inputs(shape, scale))
    E, D = E.requires_grad_(True), D.requires_grad_(True)
    weight, bias = torch.nn.Parameter(W), torch.nn.Parameter(b)
    weight.grad, bias.grad = torch.zeros_like(W), torch.zeros_like(b)
    loss = RNNTJointLossFn.apply(E, D, y, tl, ul, (weight, bias, W.to(DT[cd])), cap)
    loss.backward()
    torch.cuda.synchronize()
    return dict(loss=loss, dE=E.grad, dD=D.grad, dW=weight.grad, db=bias.grad)


@pytest.mark.parametrize("chunked", [False, True], ids=["onechunk", "chunked"])
@pytest.mark.parametrize("cd", DT)
@pytest.mark.parametrize("shape", [(3, 7, 5, 37, 40), (2, 9, 6, 300, 72)], ids=_ids)
def test_node(shape, cd, chunked):
    from espnet_amd.asr.joint_network import chunk_rows
    B, T, U, V, J = shape
    esz = 2 if cd == "bf16" else 4
    cap = 5 * (U + 1) * ((V + 7) // 8 * 8) * esz if chunked else 1 << 30  # 5 (b, t) rows: boundaries inside utterances
    assert chunk_rows(B * T, U + 1, V, esz, cap) == (5 if chunked else B * T) and B * T / 5 >= 3 and T % 5
    got = run_node(shape, cd, cap)
    for name in ("loss", "dE", "dD", "dW", "db"):
        check(name, got[name], shape, cd == "bf16")
    if not chunked and V == 37:  # logits scaled by 30: most paths underflow, the loss stays finite and within tolerance
        check("loss", run_node(shape, cd, cap, scale=30.0)["loss"], shape, cd == "bf16", scale=30.0)
    _, _, _, _, _, tl, ul = inputs(shape)
    for i in range(B):  # padding positions are exactly zero
        assert not got["dE"][i, int(tl[i]):].any() and not got["dD"][i, int(ul[i]) + 1:].any()


@pytest.mark.parametrize("cd", DT)
def test_node_memory(cd):
    # the f32 logits alone would be 64 MB; the growth is the 4 MB cap, the chunk's h / dh, ten f32 worth per node
    run_node((3, 7, 5, 37, 40), cd, 1 << 30)  # the launch layer's persistent scratch is allocated here
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = run_node((4, 64, 31, 2048, 64), cd, 4 << 20)["loss"]
    growth = torch.cuda.max_memory_allocated() - base
    print(f"growth {growth / 2 ** 20:.2f} MB")
    assert torch.isfinite(loss) and growth < 32 << 20
