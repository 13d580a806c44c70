"""ea_attn_stream_fwd (csrc/attn_stream.hip) through layers.common.attn_stream_fwd against a float64
restatement of its score law on the same f32 (or bf16-rounded) operands:
    s[i,j] = (q_i . k_j + BD[i + (legacy and j > i)][T1-1-i+j]) * scale, key j valid iff j < klen[b]
    (and j <= i when causal);  O = softmax(s) v, lse = logsumexp(s);  no valid key: O = 0, lse = -inf.
Operands are views of (rows, 3d) buffers, H = 2, B = 3 with klen = [T2 + 3, 0, T2 // 2 + 1].
Tolerance.  O: err = max |got - ref| / max |ref| <= 4 x the error of the parent's unfused path
(layers.common.attn_fwd) against the same reference at the nearest shape it serves (the same shape, or
T2 = 2048 for 2049), measured in the test and printed.  lse has no counterpart there: 4 x the error of
the restatement evaluated in f32 torch + 4 ulp of max(1, |lse|) for __expf / __logf.
Measured on MI355X, O err new / unfused, f32:  T2 = 1: 0 / 0;  cross 17x65 dk 8: 5.68e-07 / 1.84e-07
(closest to its bound);  cross 17x2049 dk 8, 64, 128: 1.26e-06 / 6.30e-07, 1.03e-06 / 1.09e-06, 1.13e-06 /
1.01e-06;  causal 65 dk 64: 1.88e-07 / 1.99e-07;  latest 130 dk 32: 4.37e-07 / 3.75e-07;  legacy 130 dk 128:
4.65e-07 / 4.03e-07.  All f32 cases: 0.4 .. 3.1 x the unfused error; all bf16 cases 1.4e-07 .. 4.4e-07
against 2.8e-03 .. 3.9e-03 (that path rounds P and O to bf16).  lse: worst 1.06e-06 of a bound of 7.0e-06."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
B, H = 3, 2
SHAPES = ([("cross", t1, t2) for t2 in (1, 63, 64, 65, 2049) for t1 in (1, 17)] + [("causal", 65, 65)] +
          [(k, t, t) for k in ("latest", "legacy") for t in (65, 130)])


class Case:
    def __init__(self, kind, T1, T2, dk, dtype):
        g = torch.Generator().manual_seed(1000 * T2 + 10 * T1 + dk + len(kind))
        self.kind, self.T1, self.T2, self.dk, self.dtype, self.d = kind, T1, T2, dk, dtype, H * dk
        self.qb = torch.randn(B * T1, 3 * self.d, generator=g).to(dtype)
        self.kvb = self.qb if kind != "cross" else torch.randn(B * T2, 3 * self.d, generator=g).to(dtype)
        if kind == "cross":
            self.qb[:, self.d:] = float("nan")  # never read
        rel = kind in ("latest", "legacy")
        self.bd = torch.randn(B, H, T1, 2 * T1 - 1, generator=g) * dk ** 0.5 if rel else None
        self.klen = torch.tensor([T2 + 3, 0, T2 // 2 + 1])
        self.scale = (0.5 if rel else 1.0) / dk ** 0.5

    def reference(self, dtype=torch.float64):
        T1, T2, d = self.T1, self.T2, self.d
        q, k, v = (b[:, c:c + d].view(B, T, H, self.dk).permute(0, 2, 1, 3).to(dtype) for b, T, c in
                   ((self.qb, T1, 0), (self.kvb, T2, d), (self.kvb, T2, 2 * d)))
        s = q @ k.transpose(-1, -2)
        i, j = torch.arange(T1)[:, None], torch.arange(T2)[None, :]
        if self.bd is not None:
            rows = (i + (j > i) if self.kind == "legacy" else i.expand(T1, T2)).clamp(max=T1 - 1)
            s = s + self.bd.to(dtype)[:, :, rows, T1 - 1 - i + j]
        keep = (j < self.klen.clamp(max=T2)[:, None, None, None]) & ((j <= i) | (self.kind != "causal"))
        s = (s * self.scale).masked_fill(~keep, float("-inf"))
        return torch.softmax(s, -1).nan_to_num(0.0) @ v, torch.logsumexp(s, -1)

    def device_args(self):
        from espnet_amd.layers.common import REL_LATEST, REL_LEGACY
        d, n = self.d, 2 * self.T1 - 1
        kvb = self.kvb.cuda()
        a = dict(B=B, H=H, T1=self.T1, T2=self.T2, dk=self.dk, ldq=3 * d, ldk=3 * d, ldv=3 * d,
                 klen=self.klen.cuda(), causal=self.kind == "causal", scale=self.scale, cd=self.dtype)
        if self.bd is not None:  # the kernel's [h][b][i][ldBD], NaN in the padding columns
            bdd = torch.full((H, B, self.T1, (n + 7) // 8 * 8), float("nan"))
            bdd[..., :n] = self.bd.permute(1, 0, 2, 3)
            a.update(bd=bdd.cuda(), ldbd=bdd.shape[-1], rel_mode=REL_LEGACY if self.kind == "legacy" else REL_LATEST)
        return (self.qb.cuda(), kvb[:, d:], kvb[:, 2 * d:]), a

    def o_err(self, O, ref):
        got = O.float().cpu().view(B, self.T1, H, self.dk).permute(0, 2, 1, 3)
        return got, float((got.double() - ref).abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=None)
def unfused_err(kind, T1, T2, dk, dtype):
    from espnet_amd.layers.common import attn_fwd
    c = Case(kind, T1, T2, dk, dtype)
    ops, a = c.device_args()
    return c.o_err(attn_fwd(*ops, p=0.0, seed=0, **a)[0], c.reference()[0])[1]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("dk", [8, 32, 64, 128])
@pytest.mark.parametrize("kind,T1,T2", SHAPES)
def test_stream_fwd_matches_f64(kind, T1, T2, dk, dtype):
    from espnet_amd.layers.common import attn_stream_fwd
    c = Case(kind, T1, T2, dk, dtype)
    ref, lse_ref = c.reference()
    ops, a = c.device_args()
    O, lse = attn_stream_fwd(*ops, lse=True, **dict(a, cd=torch.float32))
    got, err = c.o_err(O, ref)
    lse = lse.cpu().view(B, H, T1)
    bound = 4 * unfused_err(kind, T1, min(T2, 2048), dk, dtype)
    live = torch.isfinite(lse_ref)
    lse_err = float((lse.double() - lse_ref)[live].abs().max())
    lse_f32 = c.reference(torch.float32)[1].double()
    lse_bound = 4 * float((lse_f32 - lse_ref)[live].abs().max()) + 2.0 ** -21 * max(1.0, float(lse_ref[live].abs().max()))
    print(f"attn_stream {kind} T1={T1} T2={T2} dk={dk} {dtype}: O err {err:.3g} (bound {bound:.3g}), "
          f"lse err {lse_err:.3g} (bound {lse_bound:.3g})")
    assert torch.equal(got[1], torch.zeros(H, T1, dk))  # klen = 0: exactly 0, never NaN
    assert torch.equal(lse[~live], lse_ref[~live].float())  # -inf where no key is valid
    assert err <= bound and lse_err <= lse_bound


def test_refuses_dropout_and_wide_heads_by_name():
    from espnet_amd.layers.common import attn_stream_fwd
    ops, a = Case("cross", 1, 65, 8, torch.float32).device_args()
    with pytest.raises(NotImplementedError, match="dropout"):
        attn_stream_fwd(*ops, p=0.1, **a)
    with pytest.raises(NotImplementedError, match="head dim 136"):
        attn_stream_fwd(*ops, **dict(a, dk=136))
