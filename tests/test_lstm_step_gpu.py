"""ea_lstm_step (csrc/rnn_lm.hip) through the C ABI alone against a float64 restatement,
element-wise: arbitrary I / H (1, not a multiple of 8, below a tile, the recipes' 650, the
deepest K split), row counts on both sides of every row-tile choice (1, 3 | 16 | 17 | 61, and 65,
a second block row, at two small shapes), both
packed operand types, the parent gather (none, a permutation, one parent for every row, the
last with the token-id / embedding-table form of x), aligned and unaligned operand strides
(the 16-B and the element-wise operand loads), NaN-prefilled outputs with a row stride > H.

Bound (f32 pack): max |err| <= max(1e-6, 4 x the deviation from float64 of the same step
restated in plain f32 torch on the CPU).  bf16 pack: the float64 restatement rounds the
weights and the x / h operands to bf16 where the kernel does, and the f32 yardstick is that
same rounded restatement, with the same rule."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 3), (26, 26), (24, 40), (650, 650), (2048, 2048)]
ROWS = [1, 3, 16, 17, 61]
_CACHE = {}


def _weights(I, H):
    """torch's LSTM init, uniform(+-1/sqrt(H)) (no gate saturates); packs made once per shape."""
    if (I, H) not in _CACHE:
        from espnet_amd.lm.lstm_pack import pack_lstm_bias, pack_lstm_weights
        g = torch.Generator().manual_seed(17 * I + H)
        k = 1.0 / math.sqrt(H)
        w_ih, w_hh = [(torch.rand(4 * H, i, generator=g) * 2 - 1) * k for i in (I, H)]
        b_ih, b_hh = [(torch.rand(4 * H, generator=g) * 2 - 1) * k for _ in range(2)]
        dev = {dt: pack_lstm_weights(w_ih.cuda(), w_hh.cuda(), dt) for dt in (torch.float32, torch.bfloat16)}
        _CACHE[(I, H)] = (w_ih, w_hh, b_ih, b_hh, dev, pack_lstm_bias(b_ih, b_hh).cuda())
    return _CACHE[(I, H)]


def _restate(w_ih, w_hh, b_ih, b_hh, x, h, c, dtype, bf16):
    rd = (lambda t: t.to(torch.bfloat16).to(dtype)) if bf16 else (lambda t: t.to(dtype))
    g = rd(x) @ rd(w_ih).t() + b_ih.to(dtype) + rd(h) @ rd(w_hh).t() + b_hh.to(dtype)
    gi, gf, gg, go = g.chunk(4, dim=1)
    c2 = torch.sigmoid(gf) * c.to(dtype) + torch.sigmoid(gi) * torch.tanh(gg)
    return torch.sigmoid(go) * torch.tanh(c2), c2


def _strided(t, ld, rows=None, fill=0.0):
    """t (r, w) -> a cuda (rows, ld) buffer whose [:r, :w] is t; the rest `fill`."""
    buf = torch.full((rows or t.shape[0], ld), fill, dtype=torch.float32)
    buf[:t.shape[0], :t.shape[1]] = t
    return buf.cuda()


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("I,H", SHAPES)
def test_lstm_step_against_float64(I, H, dtype, n):
    _check_step(I, H, dtype, n)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("I,H", [(5, 3), (26, 26)])
def test_lstm_step_second_block_row_against_float64(I, H, dtype):
    """n = 65: grid.y = 2, the second block row holds one hypothesis (the small shapes only)."""
    _check_step(I, H, dtype, 65)


def _check_step(I, H, dtype, n):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import BF16, F32, lib
    w_ih, w_hh, b_ih, b_hh, packs, bias = _weights(I, H)
    bf = dtype == torch.bfloat16
    g = torch.Generator().manual_seed(n)
    x = torch.rand(n, I, generator=g) * 2 - 1
    hp = torch.rand(n, H, generator=g) * 2 - 1
    cp = torch.randn(n, H, generator=g)
    V = 7
    table = torch.rand(V, I, generator=g) * 2 - 1
    tok = torch.randint(0, V, (n, 3), generator=g)
    modes = {"identity": None, "permutation": torch.randperm(n, generator=g), "one_parent": torch.full((n,), n // 2)}
    for mode, src in modes.items():
        aligned = mode != "permutation"
        ldx = (I + 31) // 32 * 32 if aligned else I + 1
        ldp = (H + 31) // 32 * 32 if aligned else H + 3
        ldo = (H + 31) // 32 * 32 + 32 if aligned else H + 5
        use_tok = mode == "one_parent"
        xs = table[tok[:, -1]] if use_tok else x
        hs, cs = (hp, cp) if src is None else (hp[src], cp[src])
        ref_h, ref_c = _restate(w_ih, w_hh, b_ih, b_hh, xs, hs, cs, torch.float64, bf)
        f32_h, f32_c = _restate(w_ih, w_hh, b_ih, b_hh, xs, hs, cs, torch.float32, bf)
        bound_h = max(1e-6, 4 * float((f32_h.double() - ref_h).abs().max()))
        bound_c = max(1e-6, 4 * float((f32_c.double() - ref_c).abs().max()))

        # operands: the pad columns of x / h_prev / c_prev hold NaN — the kernel may not read them
        xd = _strided(table if use_tok else x, ldx, fill=float("nan"))
        hd, cd = _strided(hp, ldp, fill=float("nan")), _strided(cp, ldp, fill=float("nan"))
        h0, c0 = hd.clone(), cd.clone()
        tokd = tok.cuda() if use_tok else None
        srcd = None if src is None else src.to(torch.int32).cuda()
        ho = torch.full((n + 2, ldo), float("nan"), device="cuda")
        co = torch.full((n + 2, ldo), float("nan"), device="cuda")
        hb = torch.full((n + 2, ldo), float("nan"), device="cuda", dtype=torch.bfloat16) if bf else None
        sent = [t.clone() for t in (ho, co)] + ([hb.clone()] if bf else [])
        lib.ea_lstm_step(BF16 if bf else F32, n, I, H, packs[dtype].data_ptr(), bias.data_ptr(), xd.data_ptr(), ldx,
                         tokd[:, 2:].data_ptr() if use_tok else None, 3, V, hd.data_ptr(), cd.data_ptr(), ldp, n,
                         ops.ptr(srcd), ho.data_ptr(), co.data_ptr(), ldo, ops.ptr(hb), ops.stream())
        torch.cuda.synchronize()
        what = (I, H, n, mode)
        err_h = float((ho[:n, :H].cpu().double() - ref_h).abs().max())
        err_c = float((co[:n, :H].cpu().double() - ref_c).abs().max())
        print(f"lstm_step {what} {'bf16' if bf else 'f32'}: h err {err_h:.3e} (bound {bound_h:.3e}) "
              f"c err {err_c:.3e} (bound {bound_c:.3e})")
        assert err_h <= bound_h, (what, err_h, bound_h)
        assert err_c <= bound_c, (what, err_c, bound_c)
        outs = [ho, co] + ([hb] if bf else [])
        for t, s in zip(outs, sent):
            assert not t[:n, H:].cpu().float().abs().max() > 0 and not t[:n, H:].isnan().any(), (what, "pad != 0")
            bits = torch.int16 if t.dtype == torch.bfloat16 else torch.int32
            assert torch.equal(t[n:].view(bits), s[n:].view(bits)), (what, "rows >= n written")
        if bf:
            assert torch.equal(hb[:n, :H], ho[:n, :H].to(torch.bfloat16)), what
        assert torch.equal(hd.view(torch.int32), h0.view(torch.int32)), (what, "h_prev written")
        assert torch.equal(cd.view(torch.int32), c0.view(torch.int32)), (what, "c_prev written")


def test_lstm_step_rejects_bad_arguments():
    from espnet_amd._lib import F32, HipError, lib
    from espnet_amd.lm.lstm_pack import pack_lstm_bias, pack_lstm_weights
    H = 4
    w = pack_lstm_weights(torch.zeros(16, 4), torch.zeros(16, 4)).cuda()
    b = pack_lstm_bias(torch.zeros(16), torch.zeros(16)).cuda()
    t = torch.zeros(4, 2, 32, device="cuda")
    args = lambda **k: (F32, 2, k.get("I", 4), H, w.data_ptr(), b.data_ptr(), t[0].data_ptr(), k.get("ldx", 32), None,  # noqa: E731
                        0, 0, t[1].data_ptr(), t[2].data_ptr(), 32, k.get("n_prev", 2), None,
                        k.get("ho", t[3]).data_ptr(), t[0].data_ptr(), 32, None, 0)
    for bad in (dict(I=0), dict(ldx=3), dict(n_prev=1), dict(ho=t[1])):
        with pytest.raises(HipError, match="bad argument"):
            lib.ea_lstm_step(*args(**bad))
