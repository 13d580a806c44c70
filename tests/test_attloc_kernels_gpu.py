"""ea_attloc_fwd / ea_attloc_bwd (csrc/attloc.hip) through the C ABI alone against a float64 torch
restatement of one AttLoc step written here (forward by hand, backward by autograd).

Cases (pairwise, not the full product): (T, F) in {(1, 2), (5, 100), (70, 100), (130, 3),
(515, 100)} x B in {1, 3, 17} (every T meets every B), with A in {8, 20, 320}, E in {8, 256} and
C in {1, 10} taken in turn, and one case with C = 90 (the backward's other path); ragged hlens that
always hold one utterance of length 1 and one of full length (B = 1: the full one); the first step
(aprev NULL, a dw_next, no daprev), a middle step and the last step (dw_next NULL) in turn; f32 and bf16 memory for hs and pre_enc.  The outputs that
accumulate (dpre, dhs, the partial rows) start from 0 and a second call into them must add the
same again, the others start from NaN; frames at and past hlens hold NaN in hs, pre_enc, aprev and in
the initial dpre / dhs (they are never read or written) and must come back exactly 0 in w and
daprev.

Bound, the rule of tests/test_lstm_train_kernels_gpu.py: element-wise max |err| <= max(1e-6, 4 x
the deviation from float64 of the same restatement run in f32 on the CPU).  The same call twice
gives bit-identical outputs.
"""
import pytest
import torch
import torch.nn.functional as F

TFS = [(1, 2), (5, 100), (70, 100), (130, 3), (515, 100)]
BS = [1, 3, 17]
AS, ES, CS = [8, 20, 320], [8, 256], [1, 10]
STEPS = ["first", "middle", "last"]
CASES = [(T, Fw, B, AS[(i + j) % 3], ES[(i + 2 * j) % 2], CS[(i + j + 1) % 2], STEPS[(2 * i + j) % 3])
         for i, (T, Fw) in enumerate(TFS) for j, B in enumerate(BS)]
# the backward stages (64 + 32) * C floats in LDS while they fit 32 KB (C <= 85) and reads them in place
# above; A = 70 is one full and one partial 64-unit chunk, T = 37 one full and one partial 32-frame tile
CASES.append((37, 4, 3, 70, 8, 90, "middle"))
NAN = float("nan")


def _lens(B, T):
    if B == 1:
        return [T]
    mid = [max(1, (T * (k + 1)) // (B + 1)) for k in range(B - 2)]
    return [T] + mid + [1]


def _make(T, Fw, B, A, E, C, step, bf):
    g = torch.Generator().manual_seed(T * 1000 + B * 10 + A)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    lens = torch.tensor(_lens(B, T))
    valid = torch.arange(T).unsqueeze(0) < lens.unsqueeze(1)
    d = dict(hs=r(B, T, E), pre=r(B, T, A), dec=r(B, A), K=r(C, 2 * Fw + 1) / (2 * Fw + 1) ** 0.5, M=r(A, C) / C ** 0.5,
             g=r(A) / A ** 0.5, g0=r(1), dc=r(B, E), lens=lens, valid=valid, aprev=None, dwn=None)
    if bf:
        d["hs"], d["pre"] = (d[k].to(torch.bfloat16).float() for k in ("hs", "pre"))
    if step != "first":
        d["aprev"] = torch.softmax(r(B, T).masked_fill(~valid, float("-inf")), dim=1)
    if step != "last":
        d["dwn"] = r(B, T)
    return d


def _ref(d, dtype):
    """-> dict of w, c and the gradients; param gradients per utterance (B, ..)."""
    c = lambda t: t.detach().clone().to(dtype)  # noqa: E731
    B, T, E = d["hs"].shape
    valid, lens = d["valid"], d["lens"]
    hs, pre, dec = (c(d[k]).requires_grad_(True) for k in ("hs", "pre", "dec"))
    K, M, g, g0 = (c(d[k]).requires_grad_(True) for k in ("K", "M", "g", "g0"))
    ap = (valid.to(dtype) / lens.to(dtype).unsqueeze(1)) if d["aprev"] is None else c(d["aprev"])
    ap.requires_grad_(True)
    Fw = (K.shape[1] - 1) // 2
    conv = F.conv2d(ap.view(B, 1, 1, T), K.view(-1, 1, 1, 2 * Fw + 1), padding=(0, Fw)).squeeze(2).transpose(1, 2)
    e = torch.tanh(conv @ M.t() + pre + dec.unsqueeze(1)) @ g + g0
    w = torch.softmax(2.0 * e.masked_fill(~valid, float("-inf")), dim=1)
    ctx = (hs * w.unsqueeze(2)).sum(1)
    per = (ctx * c(d["dc"])).sum(1)
    if d["dwn"] is not None:
        per = per + (w * c(d["dwn"])).sum(1)
    out = dict(w=w.detach(), c=ctx.detach())
    gin = torch.autograd.grad(per.sum(), (hs, pre, dec, ap), retain_graph=True)
    out["dhs"], out["dpre"], out["ddec"], out["daprev"] = (t.masked_fill(~valid.unsqueeze(2), 0.0) if t.dim() == 3 else t
                                                           for t in gin)
    out["daprev"] = out["daprev"].masked_fill(~valid, 0.0)
    parts = []
    for b in range(B):
        gM, gK, gg, gg0 = torch.autograd.grad(per[b], (M, K, g, g0), retain_graph=True)
        parts.append(torch.cat([gM.reshape(-1), gK.reshape(-1), gg, gg0]))
    out["part"] = torch.stack(parts)
    return out


def _dev(t, valid=None, dtype=torch.float32):
    t = t.clone()
    if valid is not None:  # frames past the length are never read
        t[~valid] = NAN
    return t.to(dtype).cuda()


def _run(d, bf, base):
    from espnet_amd._lib import BF16, F32, lib
    B, T, E = d["hs"].shape
    A, C, Fw = d["pre"].shape[2], d["K"].shape[0], (d["K"].shape[1] - 1) // 2
    md, mt = (BF16, torch.bfloat16) if bf else (F32, torch.float32)
    valid = d["valid"]
    hs, pre = _dev(d["hs"], valid, mt), _dev(d["pre"], valid, mt)
    lens = d["lens"].cuda()
    dec, dc = d["dec"].cuda(), d["dc"].cuda()
    K, M, g, g0 = (d[k].cuda().contiguous() for k in ("K", "M", "g", "g0"))
    aprev = None if d["aprev"] is None else _dev(d["aprev"], valid)
    dwn = None if d["dwn"] is None else d["dwn"].cuda()
    w = torch.full((B, T), NAN, device="cuda")
    c = torch.full((B, E), NAN, device="cuda")
    nch = (A + 63) // 64
    ws = torch.full((B * T * (1 + (3 + nch) * C),), NAN, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    lib.ea_attloc_fwd(md, B, T, E, A, C, Fw, hs.data_ptr(), E, T * E, pre.data_ptr(), A, T * A, lens.data_ptr(),
                      dec.data_ptr(), A, p(aprev), T, K.data_ptr(), M.data_ptr(), g.data_ptr(), g0.data_ptr(),
                      w.data_ptr(), T, c.data_ptr(), E, ws.data_ptr(), B * T * (1 + C), st)
    dpre, dhs, part = base["dpre"].cuda(), base["dhs"].cuda(), base["part"].cuda()
    ddec = torch.full((B, A), NAN, device="cuda")
    daprev = None if d["aprev"] is None else torch.full((B, T), NAN, device="cuda")
    ws.fill_(NAN)
    lib.ea_attloc_bwd(md, B, T, E, A, C, Fw, hs.data_ptr(), E, T * E, pre.data_ptr(), A, T * A, lens.data_ptr(),
                      dec.data_ptr(), A, p(aprev), T, w.data_ptr(), T, K.data_ptr(), M.data_ptr(), g.data_ptr(),
                      dc.data_ptr(), E, p(dwn), T, dpre.data_ptr(), A, T * A, dhs.data_ptr(), E, T * E,
                      ddec.data_ptr(), A, p(daprev), T, part.data_ptr(), part.shape[1], ws.data_ptr(), ws.numel(), st)
    torch.cuda.synchronize()
    return dict(w=w, c=c, dpre=dpre, dhs=dhs, ddec=ddec, daprev=daprev, part=part)


@pytest.mark.gpu
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("T,Fw,B,A,E,C,step", CASES)
def test_attloc_step(T, Fw, B, A, E, C, step, bf):
    d = _make(T, Fw, B, A, E, C, step, bf)
    r64, r32 = _ref(d, torch.float64), _ref(d, torch.float32)
    valid = d["valid"]
    pad3 = (~valid).unsqueeze(2)
    # the accumulating outputs start from 0 (NaN in the padded frames, which no launch may touch)
    base = dict(dpre=torch.zeros(B, T, A).masked_fill(pad3, NAN), dhs=torch.zeros(B, T, E).masked_fill(pad3, NAN),
                part=torch.zeros(B, A * C + C * (2 * Fw + 1) + A + 1))
    got = _run(d, bf, base)
    again = _run(d, bf, base)
    for k, v in got.items():
        if v is None:
            assert k == "daprev" and step == "first"
            continue
        assert torch.equal(v.cpu().nan_to_num(nan=-7.0), again[k].cpu().nan_to_num(nan=-7.0)), f"{k}: two equal calls differ"
        v = v.double().cpu()
        if k in ("dpre", "dhs"):
            assert bool(v[~valid].isnan().all()), f"{k}: a padded frame was written"
            v = v.masked_fill(pad3, 0.0)
        ref64, ref32 = r64[k], r32[k].double()
        bound = max(1e-6, 4 * float((ref32 - ref64).abs().max()))
        err = float((v - ref64).abs().max())
        assert err <= bound, f"{k}: max |err| {err:.3e} > bound {bound:.3e}"
    assert not got["w"].cpu()[~valid].any(), "attention weights at padded frames must be exactly 0"
    if got["daprev"] is not None:
        assert not got["daprev"].cpu()[~valid].any()
    # accumulation: a second call into the first one's buffers adds the same again.  dpre and dhs
    # take one addition per element (x + x is exact); a partial row may take one per 32-frame tile,
    # each rounded at the running sum's magnitude
    twice = _run(d, bf, {k: got[k].cpu() for k in base})
    for k in ("dpre", "dhs"):
        assert torch.equal(twice[k].cpu().nan_to_num(nan=-7.0), (2 * got[k].cpu()).nan_to_num(nan=-7.0)), k
    tiles = (T + 31) // 32
    slack = tiles * 2.0 ** -23 * 2 * float(got["part"].abs().max())
    assert float((twice["part"].cpu().double() - 2 * got["part"].cpu().double()).abs().max()) <= slack


@pytest.mark.gpu
def test_attloc_rejects_bad_arguments():
    from espnet_amd._lib import F32, HipError, lib
    t = torch.zeros(64, device="cuda")
    n = torch.ones(1, dtype=torch.long, device="cuda")
    p = t.data_ptr()
    with pytest.raises(HipError):  # ldw < T
        lib.ea_attloc_fwd(F32, 1, 4, 2, 2, 1, 1, p, 2, 8, p, 2, 8, n.data_ptr(), p, 2, None, 0, p, p, p, p, p, 3, p, 2, p,
                          64, 0)
    with pytest.raises(HipError):  # scratch too small
        lib.ea_attloc_fwd(F32, 1, 4, 2, 2, 1, 1, p, 2, 8, p, 2, 8, n.data_ptr(), p, 2, None, 0, p, p, p, p, p, 4, p, 2, p,
                          7, 0)
