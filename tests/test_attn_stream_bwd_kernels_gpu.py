"""ea_attn_stream_fwd_train + ea_attn_stream_bwd (csrc/attn_stream.hip) through layers.common against float64
autograd over the score law restated in tests/test_attn_stream_kernels_gpu.py (its Case: (rows, 3d) operand
views, NaN in never-read columns and the band's padding, B = 3, H = 2, klen = [T2 + 3, 0, T2 // 2 + 1]), on the
same f32 or bf16-rounded operands and dO.  Outputs land in NaN-filled buffers, so an element left unwritten fails.
Dropout: the reference takes its mask from the parent's unfused forward at the same (p, seed) (Pd != 0 where
P > 0); the keep law is shared, so a different law in the new path shows as a gross error.
Tolerance, per output (O, dq, dk, dv, dbd): err = max |got - ref| / max |ref| (the absolute error where the
reference is all zeros: the dq / dk of a softmax over one key) <= 4 x the error of the parent's unfused attn_fwd +
attn_bwd against the same reference at the same shape (T2 = 2048 for 2049), measured here and printed.  Legacy
dbd: the unfused path writes 0 at band column T1 (its table row is the constant zero row) where the score law has a
gradient, so its yardstick is measured on the other columns and the new path is held to it on every column.  The
klen = 0 batch entry and every band position whose reference gradient is 0 (no source, or a masked one) are
exact zeros.
Measured on MI355X, err new / unfused.  f32: T2 = 1: exact zeros in dq / dk on
both paths;  cross 1x130 dk 8: dq 2.74e-07 / 1.96e-07, dk 1.64e-07 / 9.69e-08, dv 1.95e-07 / 1.36e-07;  cross 65x65
dk 128 p 0.1: O 8.11e-07 / 5.42e-07, dq 3.4e-07 / 4.52e-07, dk 6.82e-07 / 4.71e-07, dv 5.72e-07 / 6.66e-07;  legacy 130
dk 64 p 0.1: dq 3.67e-07 / 3.91e-07, dk 4.87e-07 / 4.36e-07, dv 4.78e-07 / 4.78e-07, dbd 2.45e-07 / 2.6e-07 (0.392 with
column T1 counted).
cross 17x2049 dk 8 (unfused at 2048 keys): O 1.26e-06 / 6.31e-07, dq 8.54e-07 / 6.56e-07, dk 3.94e-07 / 2.45e-07, dv
3.4e-07 / 1.35e-07.  Closest to its bound: O of cross 17x65 dk 8 f32, 5.68e-07 / 1.84e-07 (3.1 x); bf16 cases 1.1 x or
below (1.5e-03 .. 3.0e-03 against 1.8e-03 .. 4.2e-03)."""
import pytest
import torch

from test_attn_stream_kernels_gpu import B, H, Case

pytestmark = pytest.mark.gpu
SEED = 77
SHAPES = ([("cross", t1, t2) for t2 in (1, 63, 64, 65, 130) for t1 in (1, 17, 65)] + [("cross", 17, 2049)] +
          [("causal", 65, 65)] + [(k, t, t) for k in ("latest", "legacy") for t in (65, 130)])
F32, BF16 = torch.float32, torch.bfloat16


def heads(x2d, T, dk):
    return x2d.float().cpu().view(B, T, H, dk).permute(0, 2, 1, 3)


def reference(c, dO, mask, p):
    """O and the gradients of sum(O * dO) in float64; mask (B, H, T1, T2) bool or None."""
    T1, T2, d = c.T1, c.T2, c.d
    q, k, v = (b[:, col:col + d].view(B, T, H, c.dk).permute(0, 2, 1, 3).double().requires_grad_() for b, T, col in
               ((c.qb, T1, 0), (c.kvb, T2, d), (c.kvb, T2, 2 * d)))
    s = q @ k.transpose(-1, -2)
    i, j = torch.arange(T1)[:, None], torch.arange(T2)[None, :]
    bd = None if c.bd is None else c.bd.double().requires_grad_()
    if bd is not None:
        s = s + bd[:, :, i + (j > i) if c.kind == "legacy" else i.expand(T1, T2), T1 - 1 - i + j]
    keep = (j < c.klen.clamp(max=T2)[:, None, None, None]) & ((j <= i) | (c.kind != "causal"))
    P = torch.softmax((s * c.scale).masked_fill(~keep, float("-inf")), -1).nan_to_num(0.0)
    O = (P if mask is None else P * mask / (1 - p)) @ v
    O.backward(dO)
    ref = dict(O=O.detach(), dq=q.grad, dk=k.grad, dv=v.grad)
    return ref if bd is None else dict(ref, dbd=bd.grad)


def device_run(c, dO, p, new):
    """-> (outputs as the reference lays them out, the unfused path's dropout mask or None)"""
    from espnet_amd.layers import common as C
    ops, a = c.device_args()
    d, nan = c.d, float("nan")
    g = torch.full((B * c.T1, 3 * d), nan, dtype=c.dtype, device="cuda")
    gkv = g if c.kind != "cross" else torch.full((B * c.T2, 3 * d), nan, dtype=c.dtype, device="cuda")
    out = dict(dq=g, lddq=3 * d, dk_=gkv[:, d:], lddk=3 * d, dv=gkv[:, 2 * d:], lddv=3 * d)
    dbd = None if c.bd is None else torch.full((H, B, c.T1, a["ldbd"]), nan, dtype=c.dtype, device="cuda")
    dOd = dO.permute(0, 2, 1, 3).reshape(B * c.T1, d).to(c.dtype).cuda()
    mask = None
    if new:
        O, lse = C.attn_stream_train_fwd(*ops, p=p, seed=SEED, **a)
        C.attn_stream_bwd(dOd, *ops, lse, p=p, seed=SEED, dbd=dbd, lddbd=a.get("ldbd", 0), **out,
                          **{k: x for k, x in a.items() if k != "cd"})
    else:
        O, P, Pd, ldT = C.attn_fwd(*ops, p=p, seed=SEED, **a)
        C.attn_bwd(dOd, *ops, P, Pd, ldT, p=p, seed=SEED, dbd=dbd, **out,
                   **{k: x for k, x in a.items() if k not in ("klen", "causal", "bd")})
        mask = ((Pd.float() != 0) | ~(P > 0)).view(B, H, c.T1, ldT)[..., :c.T2].cpu() if p else None
    got = dict(O=heads(O, c.T1, c.dk), dq=heads(g[:, :d], c.T1, c.dk), dk=heads(gkv[:, d:2 * d], c.T2, c.dk),
               dv=heads(gkv[:, 2 * d:], c.T2, c.dk))
    if dbd is not None:
        got["dbd"] = dbd[..., :2 * c.T1 - 1].float().cpu().permute(1, 0, 2, 3)
    return got, mask


def errors(got, ref, skip_band_column=None):
    diff = {n: (got[n].double() - r).abs() for n, r in ref.items()}
    if skip_band_column is not None:
        diff["dbd"][..., skip_band_column] = 0.0
    return {n: float(diff[n].max() / (r.abs().max() or 1.0)) for n, r in ref.items()}


def baseline(kind, T1, T2, dk, dtype, p):
    """The case, its dO and float64 reference, and the unfused path's errors (at 2048 keys past them)."""
    c = Case(kind, T1, T2, dk, dtype)
    dO = torch.randn(B, H, T1, dk, generator=torch.Generator().manual_seed(T1 + T2)).to(dtype).double()
    if T2 > 2048:
        return c, dO, reference(c, dO, None, 0.0), baseline(kind, T1, 2048, dk, dtype, p)[3]
    got, mask = device_run(c, dO, p, new=False)
    ref = reference(c, dO, mask, p)
    return c, dO, ref, errors(got, ref, T1 if kind == "legacy" else None)


# 2049 keys with p = 0 only: the unfused path, the source of the reference's mask, does not serve them
@pytest.mark.parametrize("kind,T1,T2,dk,dtype,p", [
    s + (dk, dtype, p) for s in SHAPES for dk in (8, 64, 128) for dtype in (F32, BF16) for p in (0.0, 0.1)
    if s[2] <= 2048 or p == 0] + [("latest", 65, 65, 24, F32, 0.1)])
def test_stream_train_fwd_bwd_match_f64_autograd(kind, T1, T2, dk, dtype, p):
    c, dO, ref, base = baseline(kind, T1, T2, dk, dtype, p)
    got, _ = device_run(c, dO, p, new=True)
    err = errors(got, ref)
    print(f"attn_stream_bwd {kind} T1={T1} T2={T2} dk={dk} {dtype} p={p}: err new / unfused " +
          ", ".join(f"{n} {err[n]:.3g} / {base[n]:.3g}" for n in err))
    for n, x in got.items():
        assert torch.equal(x[1], torch.zeros_like(x[1])), n  # klen = 0: exactly 0, never NaN
    if "dbd" in got:
        assert not got["dbd"][ref["dbd"] == 0].any()  # band positions without a (valid) source
    for n in err:
        assert err[n] <= 4 * base[n], (n, err[n], base[n])
