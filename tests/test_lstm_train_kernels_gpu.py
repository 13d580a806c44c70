"""ea_lstm_cell_fwd / ea_lstm_cell_bwd (csrc/lstm_train.hip) through the C ABI alone against a
float64 restatement, element-wise, step by step through a small host loop.

Shapes: H in {3, 26, 30, 64} (the forward's 4-unit tile tail and the backward's 16-unit tile
tail, H below / off / on the K granule of 32) and H = 1024 at B = 3 and at B = 65 (two column
tiles per block in the forward, with one and with four row tiles: the instantiation a 2048-wide
training batch launches); B in {1, 17, 65} (one row tile, two, a second block row); every (H, B)
pair runs with ONE T of {1, 2, 5}, taken in turn so that each T meets every H and every B (the
first backward launch has no recurrent product, the later ones carry dc); non-zero initial
state; f32 and bf16 packs; NaN-prefilled outputs (pad columns must come back zero, rows >= n
untouched).

Every step is checked on its own: the restatement of step t starts from the kernel's outputs
of the step before, so nothing accumulates.  Bound, the rule of tests/test_lstm_step_gpu.py:
max |err| <= max(1e-6, 4 x the deviation from float64 of the same step restated in plain f32
torch on the CPU); with the bf16 pack both restatements round the weights and the h / dgates
operand to bf16 where the kernel does.  The bf16 copies the kernels write (h, dgates) must be
the bit-exact rounding of their f32 outputs.
"""
import math

import pytest
import torch

HS = [3, 26, 30, 64]
BS = [1, 17, 65]
TS = [1, 2, 5]
CASES = [(H, B, TS[(i + j) % 3]) for i, H in enumerate(HS) for j, B in enumerate(BS)] + [(1024, 3, 2), (1024, 65, 2)]
NAN = float("nan")


def _rup(x, g=32):
    return (x + g - 1) // g * g


def _w_hh(H):
    g = torch.Generator().manual_seed(1000 + H)
    return (torch.rand(4 * H, H, generator=g) * 2 - 1) / math.sqrt(H)


def _rd(bf, dtype):
    return (lambda t: t.float().to(torch.bfloat16).to(dtype)) if bf else (lambda t: t.to(dtype))


def _fwd_ref(w, xproj, h, c, dtype, bf):
    rd = _rd(bf, dtype)
    g = xproj.to(dtype) + rd(h) @ rd(w).t()
    i, f, gg, o = g.chunk(4, dim=1)
    i, f, gg, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
    c2 = f * c.to(dtype) + i * gg
    return o * torch.tanh(c2), c2, torch.stack([i, f, gg, o], dim=2)  # gates (B, H, 4)


def _bwd_ref(w, dgn, dho, gates, c, cp, dci, dtype, bf):
    rd = _rd(bf, dtype)
    dh = dho.to(dtype)
    if dgn is not None:
        dh = dh + rd(dgn) @ rd(w)
    i, f, g, o = [gates[:, :, q].to(dtype) for q in range(4)]
    tc = torch.tanh(c.to(dtype))
    d_o = dh * tc * o * (1 - o)
    dc = dci.to(dtype) + dh * o * (1 - tc * tc)
    d_i = dc * g * i * (1 - i)
    d_f = dc * cp.to(dtype) * f * (1 - f)
    d_g = dc * i * (1 - g * g)
    return torch.cat([d_i, d_f, d_g, d_o], dim=1), dc * f, dh


def _bound(a32, a64):
    return max(1e-6, 4 * float((a32.double() - a64).abs().max()))


def _close(got, ref64, ref32, what):
    err = float((got.double().cpu() - ref64).abs().max())
    bound = _bound(ref32, ref64)
    assert err <= bound, f"{what}: max |err| {err:.3e} > bound {bound:.3e}"


def _buf(rows, ld, dtype=torch.float32):
    return torch.full((rows, ld), NAN, dtype=dtype, device="cuda")


def _put(t, ld):
    b = torch.full((t.shape[0], ld), NAN, dtype=torch.float32)
    b[:, :t.shape[1]] = t
    return b.cuda()


def test_pack_round_trip_cpu():
    """Every weight_hh element sits at the documented address of both packs, the rest is 0."""
    from espnet_amd.lm.lstm_pack import pack_lstm_hh, pack_lstm_hh_t
    for H in (3, 26, 64):
        w = _w_hh(H)
        for dtype, SL in ((torch.float32, 16), (torch.bfloat16, 32)):
            wq = w.to(dtype).float()
            Hp, Gp = _rup(H), _rup(4 * H)
            nt, ntt = (H + 3) // 4, (H + 15) // 16
            P = pack_lstm_hh(w, dtype).float().view(nt, Hp // SL, 4, 4, SL)  # (t, s, u, gate, j)
            back = P.permute(3, 0, 2, 1, 4).reshape(4, nt * 4, Hp)  # (gate, unit, k)
            assert torch.equal(back[:, :H, :H], wq.view(4, H, H))
            back[:, :H, :H] = 0
            assert not back.any()
            Pt = pack_lstm_hh_t(w, dtype).float().view(ntt, Gp // SL, 16, SL)  # (t, s, r, j)
            back_t = Pt.permute(0, 2, 1, 3).reshape(ntt * 16, Gp)  # (unit, k)
            assert torch.equal(back_t[:H, :4 * H], wq.t())
            back_t[:H, :4 * H] = 0
            assert not back_t.any()
            # the address formula of include/espnet_amd.h on a few elements
            flat, flat_t = pack_lstm_hh(w, dtype).float(), pack_lstm_hh_t(w, dtype).float()
            for gate, unit, k in ((0, 0, 0), (3, H - 1, H - 1), (2, H // 2, 1)):
                t, u, s, j = unit // 4, unit % 4, k // SL, k % SL
                assert flat[((t * (Hp // SL) + s) * 16 + 4 * u + gate) * SL + j] == wq[gate * H + unit, k]
                kk = gate * H + k  # a row of weight_hh as the backward's K index
                t, r, s, j = unit // 16, unit % 16, kk // SL, kk % SL
                assert flat_t[((t * (Gp // SL) + s) * 16 + r) * SL + j] == wq[kk, unit]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,B,T", CASES)
def test_cell_fwd_bwd_against_float64(H, B, T, dtype):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import BF16, F32, lib
    from espnet_amd.lm.lstm_pack import pack_lstm_hh, pack_lstm_hh_t
    bf = dtype == torch.bfloat16
    wd = BF16 if bf else F32
    w = _w_hh(H)
    pack, pack_t = pack_lstm_hh(w.cuda(), dtype), pack_lstm_hh_t(w.cuda(), dtype)
    G, Hp = 4 * H, _rup(H)
    ldo, ldd, ldx = Hp + 32, _rup(G) + 32, G + 4
    gen = torch.Generator().manual_seed(H * 131 + B * 7 + T)
    st = ops.stream()

    # ---- forward, T steps from a non-zero state
    xproj = torch.randn(T, B, G, generator=gen)
    h = torch.rand(B, H, generator=gen) * 2 - 1
    c = torch.randn(B, H, generator=gen)
    hs = [_put(h, ldo)] + [_buf(B + 2, ldo) for _ in range(T)]
    cs = [_put(c, ldo)] + [_buf(B + 2, ldo) for _ in range(T)]
    hbs = [hs[0].to(torch.bfloat16)] + [_buf(B + 2, ldo, torch.bfloat16) for _ in range(T)] if bf else None
    gs = [_buf(B + 2, G) for _ in range(T)]
    xd = [_put(xproj[t], ldx) for t in range(T)]
    for t in range(T):
        hin = hbs[t] if bf else hs[t]
        lib.ea_lstm_cell_fwd(wd, B, H, pack.data_ptr(), xd[t].data_ptr(), ldx, hin.data_ptr(), cs[t].data_ptr(), ldo,
                             hs[t + 1].data_ptr(), cs[t + 1].data_ptr(), ldo, hbs[t + 1].data_ptr() if bf else None,
                             gs[t].data_ptr(), G, st)
    torch.cuda.synchronize()
    for t in range(T):
        hp, cp = hs[t][:B, :H].cpu(), cs[t][:B, :H].cpu()
        r64 = _fwd_ref(w, xproj[t], hp, cp, torch.float64, bf)
        r32 = _fwd_ref(w, xproj[t], hp, cp, torch.float32, bf)
        _close(hs[t + 1][:B, :H], r64[0], r32[0], f"h[{t}]")
        _close(cs[t + 1][:B, :H], r64[1], r32[1], f"c[{t}]")
        _close(gs[t][:B].view(B, H, 4), r64[2], r32[2], f"gates[{t}]")
        for name, o in (("h", hs[t + 1]), ("c", cs[t + 1])) + ((("hb", hbs[t + 1]),) if bf else ()):
            assert float(o[:B, H:].float().abs().max()) == 0.0, f"{name}[{t}] pad columns"
            assert bool(o[B:].isnan().all()), f"{name}[{t}] rows >= n were written"
        assert bool(gs[t][B:].isnan().all())
        if bf:
            assert torch.equal(hbs[t + 1][:B, :H], hs[t + 1][:B, :H].to(torch.bfloat16)), f"hb[{t}]"

    # ---- backward, t = T-1 .. 0 over the forward's saved gates and cell states
    dho = torch.randn(T, B, H, generator=gen)
    dhd = [_put(dho[t], ldo) for t in range(T)]
    dg = [_buf(B + 2, ldd) for _ in range(T)]
    dgb = [_buf(B + 2, ldd, torch.bfloat16) for _ in range(T)] if bf else None
    dcs = [_buf(B + 2, ldo) for _ in range(T)]
    dht = [_buf(B + 2, ldo) for _ in range(T)]
    for t in range(T - 1, -1, -1):
        first = t == T - 1
        nxt = None if first else (dgb[t + 1] if bf else dg[t + 1]).data_ptr()
        lib.ea_lstm_cell_bwd(wd, B, H, pack_t.data_ptr(), nxt, ldd, dhd[t].data_ptr(), ldo, gs[t].data_ptr(), G,
                             cs[t + 1].data_ptr(), cs[t].data_ptr(), ldo, None if first else dcs[t + 1].data_ptr(),
                             dcs[t].data_ptr(), ldo, dg[t].data_ptr(), dgb[t].data_ptr() if bf else None, ldd,
                             dht[t].data_ptr(), ldo, st)
    torch.cuda.synchronize()
    for t in range(T - 1, -1, -1):
        first = t == T - 1
        dgn = None if first else dg[t + 1][:B, :G].cpu()
        dci = torch.zeros(B, H) if first else dcs[t + 1][:B, :H].cpu()
        args = (w, dgn, dho[t], gs[t][:B].view(B, H, 4).cpu(), cs[t + 1][:B, :H].cpu(), cs[t][:B, :H].cpu(), dci)
        r64, r32 = _bwd_ref(*args, torch.float64, bf), _bwd_ref(*args, torch.float32, bf)
        _close(dg[t][:B, :G], r64[0], r32[0], f"dgates[{t}]")
        _close(dcs[t][:B, :H], r64[1], r32[1], f"dc_carry[{t}]")
        _close(dht[t][:B, :H], r64[2], r32[2], f"dh[{t}] (dh_out + the recurrent part)")
        assert float(dg[t][:B, G:].abs().max()) == 0.0 and float(dcs[t][:B, H:].abs().max()) == 0.0
        assert bool(dg[t][B:].isnan().all()) and bool(dcs[t][B:].isnan().all())
        if bf:
            assert torch.equal(dgb[t][:B, :G], dg[t][:B, :G].to(torch.bfloat16)), f"dgates_b[{t}]"
            assert float(dgb[t][:B, G:].float().abs().max()) == 0.0


@pytest.mark.gpu
def test_argument_checks():
    """n < 0, a misaligned pack, leading dimensions below the width and aliased in / out states
    return the error code before anything is launched; n = 0 is a no-op."""
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import F32, HipError, lib
    from espnet_amd.lm.lstm_pack import pack_lstm_hh, pack_lstm_hh_t
    H, B = 8, 4
    G, Hp = 4 * H, 32
    w = _w_hh(H).cuda()
    pk, pkt = pack_lstm_hh(w), pack_lstm_hh_t(w)
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    xp, h0, c0, h1, c1, gt = z(B, G), z(B, Hp), z(B, Hp), z(B, Hp), z(B, Hp), z(B, G)
    st = ops.stream()

    def fwd(n=B, pack=pk.data_ptr(), hp=h0, ho=h1, co=c1, ldp=Hp, ldg=G):
        lib.ea_lstm_cell_fwd(F32, n, H, pack, xp.data_ptr(), G, hp.data_ptr(), c0.data_ptr(), ldp, ho.data_ptr(),
                             co.data_ptr(), Hp, None, gt.data_ptr(), ldg, st)

    fwd()
    fwd(n=0)
    for bad in (dict(n=-1), dict(pack=pk.data_ptr() + 4), dict(ho=h0), dict(co=c0), dict(ldp=H - 1), dict(ldg=G - 4)):
        with pytest.raises(HipError, match="bad argument"):
            fwd(**bad)

    dgn, dho, dci, dco, dgo = z(B, G), z(B, Hp), z(B, Hp), z(B, Hp), z(B, G)

    def bwd(n=B, pack=pkt.data_ptr(), nxt=dgn, dc_in=dci, dc_out=dco, out=dgo, ldd=G):
        lib.ea_lstm_cell_bwd(F32, n, H, pack, nxt.data_ptr(), G, dho.data_ptr(), Hp, gt.data_ptr(), G, c1.data_ptr(),
                             c0.data_ptr(), Hp, dc_in.data_ptr(), dc_out.data_ptr(), Hp, out.data_ptr(), None, ldd,
                             None, 0, st)

    bwd()
    bwd(n=0)
    for bad in (dict(n=-1), dict(pack=pkt.data_ptr() + 4), dict(dc_out=dci), dict(out=dgn), dict(ldd=G - 1)):
        with pytest.raises(HipError, match="bad argument"):
            bwd(**bad)
    torch.cuda.synchronize()
