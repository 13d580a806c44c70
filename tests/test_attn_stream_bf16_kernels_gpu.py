"""The bf16-MFMA streaming attention (csrc/attn_stream_bf16.hip) through layers.common's wrappers with
cores="bf16", against float64 autograd of the score law on the bf16-rounded operands and dO:
    s[i,j] = (q_i . k_j + BD[i + (legacy and j > i)][T1-1-i+j]) * scale, key j valid iff j < klen[b] (and j <= i when
    causal);  O = (softmax(s) m / (1-p)) v, m the keep mask of the unfused forward at the same (p, seed).
B = H = 2, operands are views of (rows, 3d) buffers with NaN in never-read columns, outputs land in NaN-filled
buffers.  klen = [T2, 1] on the self / rel-pos cases (an utterance of length 1), [T2, T2 // 2 + 1] otherwise.
Tolerance, per output (O, dq, dk, dv, dbd): err = max |got - ref| / max |ref| (absolute where the reference is all
zeros) <= FACTOR x the error of the unfused bf16 chain (attn_fwd + attn_bwd; legacy dbd without its band column T1,
see tests/test_attn_stream_bwd_kernels_gpu.py) on the same inputs + FLOOR, one bf16 ulp of the largest element.
Rounding P and dS to bf16 is the only excess the design allows; the measured ratios are in DESIGN.md §22.
Exact: lse against the f32-MFMA streaming kernel's at 1e-5 of the largest |lse| (both sum bf16 products in f32);
the inference entry bit-equal to the training entry at p = 0; the dropped set equal to attn_fwd's."""
import pytest
import torch

pytestmark = pytest.mark.gpu
B, H, SEED = 2, 2, 77
FACTOR, FLOOR = 1.5, 2.0 ** -9  # worst measured ratio 1.007
BF16 = torch.bfloat16
CASES = [("self", 1, 1, 8, 0.0), ("self", 63, 65, 32, 0.1), ("self", 65, 130, 24, 0.0), ("self", 130, 64, 128, 0.1),
         ("causal", 1, 1, 32, 0.0), ("causal", 63, 65, 24, 0.1), ("causal", 65, 130, 128, 0.0),
         ("causal", 130, 64, 8, 0.1), ("cross", 1, 1, 128, 0.1), ("cross", 63, 65, 128, 0.0),
         ("cross", 65, 130, 32, 0.1), ("cross", 130, 64, 24, 0.0), ("latest", 1, 1, 24, 0.1),
         ("latest", 65, 65, 32, 0.0), ("latest", 130, 130, 128, 0.1), ("legacy", 65, 65, 8, 0.1),
         ("legacy", 130, 130, 32, 0.0)]


def heads(x2d, T, dk):
    return x2d.float().cpu().view(B, T, H, dk).permute(0, 2, 1, 3)


class Case:
    def __init__(self, kind, T1, T2, dk):
        g = torch.Generator().manual_seed(1000 * T2 + 10 * T1 + dk + len(kind))
        self.kind, self.T1, self.T2, self.dk, self.d, self.rel = kind, T1, T2, dk, H * dk, kind in ("latest", "legacy")
        self.qb = torch.randn(B * T1, 3 * self.d, generator=g).to(BF16)
        self.kvb = torch.randn(B * T2, 3 * self.d, generator=g).to(BF16)
        self.qb[:, self.d:] = self.kvb[:, :self.d] = float("nan")  # never read
        self.bd = torch.randn(B, H, T1, 2 * T1 - 1, generator=g) * dk ** 0.5 if self.rel else None
        self.klen = torch.tensor([T2, 1 if kind not in ("causal", "cross") else T2 // 2 + 1])
        self.scale = (0.5 if self.rel else 1.0) / dk ** 0.5
        self.dO = torch.randn(B, H, T1, dk, generator=g).to(BF16).double()

    def reference(self, mask, p):
        """O, lse and the gradients of sum(O * dO) in float64; mask (B, H, T1, T2) bool or None"""
        T1, T2, d = self.T1, self.T2, self.d
        q, k, v = (b[:, c:c + d].view(B, T, H, self.dk).permute(0, 2, 1, 3).double().requires_grad_() for b, T, c in
                   ((self.qb, T1, 0), (self.kvb, T2, d), (self.kvb, T2, 2 * d)))
        s = q @ k.transpose(-1, -2)
        i, j = torch.arange(T1)[:, None], torch.arange(T2)[None, :]
        bd = self.bd.double().requires_grad_() if self.rel else None
        if self.rel:
            s = s + bd[:, :, i + (j > i) if self.kind == "legacy" else i.expand(T1, T2), T1 - 1 - i + j]
        keep = (j < self.klen[:, None, None, None]) & ((j <= i) | (self.kind != "causal"))
        P = torch.softmax((s * self.scale).masked_fill(~keep, float("-inf")), -1)
        O = (P if mask is None else P * mask / (1 - p)) @ v
        O.backward(self.dO)
        ref = dict(O=O.detach(), dq=q.grad, dk=k.grad, dv=v.grad)
        return dict(ref, dbd=bd.grad) if self.rel else ref

    def run(self, p, cores):
        """-> outputs as the reference lays them out, lse, the unfused path's dropout mask (cores None)"""
        from espnet_amd.layers import common as C
        d, n, nan = self.d, 2 * self.T1 - 1, float("nan")
        kvb = self.kvb.cuda()
        ops = (self.qb.cuda(), kvb[:, d:], kvb[:, 2 * d:])
        a = dict(B=B, H=H, T1=self.T1, T2=self.T2, dk=self.dk, ldq=3 * d, ldk=3 * d, ldv=3 * d,
                 klen=self.klen.cuda(), causal=self.kind == "causal", scale=self.scale)
        dbd = None
        if self.rel:  # the kernel's [h][b][i][ldBD], NaN in the padding columns
            bdd = torch.full((H, B, self.T1, (n + 7) // 8 * 8), nan)
            bdd[..., :n] = self.bd.permute(1, 0, 2, 3)
            a.update(bd=bdd.cuda(), ldbd=bdd.shape[-1],
                     rel_mode=C.REL_LEGACY if self.kind == "legacy" else C.REL_LATEST)
            dbd = torch.full(bdd.shape, nan, dtype=BF16, device="cuda")
        g = torch.full((B * self.T1, 3 * d), nan, dtype=BF16, device="cuda")
        gkv = torch.full((B * self.T2, 3 * d), nan, dtype=BF16, device="cuda")
        out = dict(dq=g, lddq=3 * d, dk_=gkv[:, d:], lddk=3 * d, dv=gkv[:, 2 * d:], lddv=3 * d)
        dOd = self.dO.permute(0, 2, 1, 3).reshape(B * self.T1, d).to(BF16).cuda()
        lse = mask = None
        if cores:
            O, lse = C.attn_stream_train_fwd(*ops, p=p, seed=SEED, cd=BF16, cores=cores, **a)
            if cores == "bf16":
                assert O.dtype == BF16
                C.attn_stream_bwd(dOd, *ops, lse, p=p, seed=SEED, dbd=dbd, lddbd=a.get("ldbd", 0), cores=cores,
                                  **out, **a)
                if p == 0:
                    assert torch.equal(O, C.attn_stream_fwd(*ops, cd=BF16, cores=cores, **a))
        else:
            O, P, Pd, ldT = C.attn_fwd(*ops, p=p, seed=SEED, cd=BF16, **a)
            C.attn_bwd(dOd, *ops, P, Pd, ldT, p=p, seed=SEED, cd=BF16, dbd=dbd, **out,
                       **{k: x for k, x in a.items() if k not in ("klen", "causal", "bd")})
            mask = ((Pd.float() != 0) | ~(P > 0)).view(B, H, self.T1, ldT)[..., :self.T2].cpu() if p else None
        got = dict(O=heads(O, self.T1, self.dk), dq=heads(g[:, :d], self.T1, self.dk),
                   dk=heads(gkv[:, d:2 * d], self.T2, self.dk), dv=heads(gkv[:, 2 * d:], self.T2, self.dk))
        if self.rel:
            got["dbd"] = dbd[..., :n].float().cpu().permute(1, 0, 2, 3)
        return got, lse, mask


def errors(got, ref, skip_band_column=None):
    diff = {n: (got[n].double() - r).abs() for n, r in ref.items()}
    if skip_band_column is not None:
        diff["dbd"][..., skip_band_column] = 0.0
    return {n: float(diff[n].max() / (r.abs().max() or 1.0)) for n, r in ref.items()}


@pytest.mark.parametrize("kind,T1,T2,dk,p", CASES)
def test_bf16_cores_match_f64_autograd(kind, T1, T2, dk, p):
    c = Case(kind, T1, T2, dk)
    old, _, mask = c.run(p, None)
    ref = c.reference(mask, p)
    base = errors(old, ref, T1 if kind == "legacy" else None)
    got, lse, _ = c.run(p, "bf16")
    err = errors(got, ref)
    print(f"attn_stream_bf16 {kind} T1={T1} T2={T2} dk={dk} p={p}: err new / unfused " +
          ", ".join(f"{n} {err[n]:.3g} / {base[n]:.3g}" for n in err))
    if "dbd" in got:
        assert not got["dbd"][ref["dbd"] == 0].any()  # band positions without a (valid) source: exact zeros
    for n in err:
        assert err[n] <= FACTOR * base[n] + FLOOR, (n, err[n], base[n])
    lse32 = c.run(p, "f32")[1]
    assert torch.isfinite(lse).all() and float((lse - lse32).abs().max()) <= 1e-5 * float(lse32.abs().max())


def test_bf16_cores_drop_what_attn_fwd_drops():
    """V = the identity block: O[i][j] is the dropped probability of key j itself."""
    c = Case("cross", 63, 65, 128)
    c.kvb[:, 2 * c.d:] = torch.eye(128)[:65].repeat(B, H)
    mask = c.run(0.1, None)[2]
    O = c.run(0.1, "bf16")[0]["O"][..., :65]
    live = torch.arange(65) < c.klen[:, None, None, None]
    assert torch.equal((O != 0) | ~live, mask | ~live) and 0.05 < float((~mask).float().mean()) < 0.15
