"""ea_lstm_bicell_fwd / ea_lstm_bicell_bwd (csrc/lstm_bidir.hip), driven through BiLSTMTape
(espnet_amd/lm/rnn_train.py), which adds nothing but the buffers and the operand blocks.

Bit-equality.  With every length = T the mask is never taken and a direction is exactly a sweep
of ea_lstm_cell_fwd / ea_lstm_cell_bwd (LSTMTape): the same block product on the same tiles, the
same epilogue.  ndir = 1 must equal that sweep bit for bit, and with ndir = 2 direction 0 must
equal it and direction 1 must equal the single-direction sweep of the reverse weights over the
time-reversed rows, state buffers (pad columns included), gates, the bf16 copies and the gate
gradients alike, f32 and bf16.  T = 3; H in {5, 24, 320} (pad columns; not a multiple of 4 / of
16), n in {1, 17, 33, 70} (every row-tile count, a partial row tile, a second block row), and one
H = 1024, n = 3 forward sweep for the two-column-tile blocks.

Masks.  B = 5, T = 7, H in {5, 24}, lengths (3, 7, 1, 7, 3): 1, T, repeated values, unsorted.  The
yardstick is torch.nn.LSTM(bidirectional=True) in float64 on the CPU over a pack_padded_sequence;
outputs, the input gradient and all eight parameter gradients are held to
max(1e-6, 4 x the deviation of the same module in float32 from float64), the rule of
tests/test_lstm_train_kernels_gpu.py.  Padded outputs, padded states and the gate gradients of
padded steps must be exactly 0 (f32 and bf16).
"""
import pytest
import torch

T3 = 3
EQ_CASES = [(H, n) for H in (5, 24, 320) for n in (1, 17, 33, 70)]
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])


def _layers(H, I, cd, seed, ndir=2):
    """A seeded CUDA nn.LSTM (one layer, bidirectional) and the LSTMLayer of each direction."""
    from espnet_amd.lm.rnn_train import LSTMLayer
    torch.manual_seed(seed)
    m = torch.nn.LSTM(I, H, 1, bidirectional=True).cuda()
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    out = []
    for d in range(ndir):
        w = getattr(m, "weight_ih_l0" + ("_reverse" if d else "")).detach().to(cd)
        lay = LSTMLayer(m, w, cd, k=0, reverse=bool(d))
        lay.refresh()
        out.append(lay)
    return m, out


def _single_sweep(layer, xproj, dy, T, n, fwd_only=False):
    """The parent kernels' sweep of one direction: LSTMTape over xproj / dy (T * n, .)."""
    from espnet_amd.lm.rnn_train import LSTMTape
    tape = LSTMTape(layer, T, n, xproj.device)
    step = tape.fwd_steps(xproj)
    for t in range(T):
        step(t)
    if not fwd_only:
        step = tape.bwd_steps(dy, dy.stride(0))
        for t in range(T - 1, -1, -1):
            step(t)
    return tape


def _flip(x, T):
    return x.view(T, -1, x.shape[-1]).flip(0).reshape(x.shape).contiguous()


def _eq(a, b, what):
    assert a.shape == b.shape and torch.equal(a, b), f"{what}: not bit-equal"


def _check_dir(bi, d, ref, flipped, bf, bwd=True):
    f = (lambda t: t.flip(0)) if flipped else (lambda t: t)
    _eq(bi.hs[d], f(ref.hs), f"hs[{d}]")
    _eq(bi.cs[d], f(ref.cs), f"cs[{d}]")
    _eq(bi.gates[d], f(ref.gates), f"gates[{d}]")
    if bf:
        _eq(bi.hb[d], f(ref.hb), f"hb[{d}]")
    if bwd:
        _eq(bi.dg[d], f(ref.dg), f"dgates[{d}]")
        if bf:
            _eq(bi.dgm[d], f(ref.dgn).reshape(-1, ref.dgn.shape[-1])[:, :bi.dgm[d].shape[1]], f"dgates_b[{d}]")


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("H,n", EQ_CASES)
def test_full_lengths_equal_the_single_direction_kernels(H, n, dtype):
    from espnet_amd.lm.rnn_train import BiLSTMTape
    T, bf = T3, dtype == torch.bfloat16
    _, lays = _layers(H, 4, dtype, 100 + H)
    gen = torch.Generator(device="cuda").manual_seed(H * 7 + n)
    xproj = [torch.randn(T * n, 4 * H, generator=gen, device="cuda") for _ in range(2)]
    dy = torch.randn(T * n, 2 * H, generator=gen, device="cuda")
    lens = torch.full((n,), T, dtype=torch.long, device="cuda")
    dys = [dy[:, :H].contiguous(), dy[:, H:].contiguous()]
    ref0 = _single_sweep(lays[0], xproj[0], dys[0], T, n)
    ref1 = _single_sweep(lays[1], _flip(xproj[1], T), _flip(dys[1], T), T, n)

    one = BiLSTMTape(lays[:1], lens, T, n, "cuda")
    one.forward(xproj[:1])
    one.backward(dys[0])
    _check_dir(one, 0, ref0, False, bf)
    _eq(one.outputs(), ref0.outputs(), "outputs, ndir 1")

    two = BiLSTMTape(lays, lens, T, n, "cuda")
    two.forward(xproj)
    two.backward(dy)
    _check_dir(two, 0, ref0, False, bf)
    _check_dir(two, 1, ref1, True, bf)
    _eq(two.outputs(), torch.cat([ref0.outputs(), _flip(ref1.outputs().contiguous(), T)], dim=1), "outputs, ndir 2")


@pytest.mark.gpu
@DTYPES
def test_two_column_tile_forward_equals_the_single_direction_kernel(dtype):
    """H = 1024: two column tiles per block (the forward's wide instantiation), n = 3."""
    from espnet_amd.lm.rnn_train import BiLSTMTape
    H, n, T, bf = 1024, 3, 1, dtype == torch.bfloat16
    _, lays = _layers(H, 4, dtype, 1024)
    gen = torch.Generator(device="cuda").manual_seed(5)
    xproj = [torch.randn(T * n, 4 * H, generator=gen, device="cuda") for _ in range(2)]
    lens = torch.full((n,), T, dtype=torch.long, device="cuda")
    ref0 = _single_sweep(lays[0], xproj[0], None, T, n, fwd_only=True)
    ref1 = _single_sweep(lays[1], xproj[1], None, T, n, fwd_only=True)
    two = BiLSTMTape(lays, lens, T, n, "cuda")
    two.forward(xproj)
    _check_dir(two, 0, ref0, False, bf, bwd=False)
    _check_dir(two, 1, ref1, True, bf, bwd=False)


MASK_LENS = (3, 7, 1, 7, 3)


def _packed_reference(m, x, dy, lens, dtype):
    """nn.LSTM on a pack_padded_sequence on the CPU in `dtype`: x (T, B, I), dy (T, B, 2H) ->
    (y, dx, {parameter name: gradient})."""
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    T = x.shape[0]
    ref = torch.nn.LSTM(m.input_size, m.hidden_size, 1, bidirectional=True).to(dtype)
    ref.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in m.state_dict().items()})
    xr = x.cpu().to(dtype).requires_grad_(True)
    packed = pack_padded_sequence(xr, torch.tensor(lens), enforce_sorted=False)
    y, _ = pad_packed_sequence(ref(packed)[0], total_length=T)
    y.backward(dy.cpu().to(dtype))
    return y.detach(), xr.grad, {k: p.grad for k, p in ref.named_parameters()}


def _close(got, r64, r32, what):
    err = float((got.double().cpu() - r64).abs().max())
    bound = max(1e-6, 4 * float((r32.double() - r64).abs().max()))
    print(f"{what}: max |err| {err:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{what}: max |err| {err:.3e} > bound {bound:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("H", [5, 24])
def test_masks_against_packed_float64(H):
    from espnet_amd.lm.rnn_train import BiLSTMLayerFn
    B, T, I = 5, 7, 6
    m, lays = _layers(H, I, torch.float32, 300 + H)
    gen = torch.Generator().manual_seed(H)
    x = torch.randn(T, B, I, generator=gen)
    dy = torch.randn(T, B, 2 * H, generator=gen)  # junk on the padded frames too: it must not count
    lens = torch.tensor(MASK_LENS, dtype=torch.long, device="cuda")
    xd = x.cuda().view(T * B, I).requires_grad_(True)
    y = BiLSTMLayerFn.apply(xd, lays, lens, T, B)
    tape = y.grad_fn.save[0]
    y.backward(dy.cuda().view(T * B, 2 * H))
    torch.cuda.synchronize()
    r64 = _packed_reference(m, x, dy, MASK_LENS, torch.float64)
    r32 = _packed_reference(m, x, dy, MASK_LENS, torch.float32)
    _close(y.detach().view(T, B, 2 * H), r64[0], r32[0], "y")
    _close(xd.grad.view(T, B, I), r64[1], r32[1], "dx")
    for k, p in m.named_parameters():
        _close(p.grad, r64[2][k], r32[2][k], "d" + k)
    pad = (torch.arange(T)[:, None] >= torch.tensor(MASK_LENS)[None, :]).cuda()  # (T, B)
    assert float(y.detach().view(T, B, -1)[pad].abs().max()) == 0.0, "padded outputs"
    for d in range(2):
        assert float(tape.dg[d][pad].abs().max()) == 0.0, f"gate gradients of padded steps, direction {d}"


@pytest.mark.gpu
@DTYPES
def test_padded_steps_are_exact_zeros(dtype):
    """The stores of inactive rows, both dtypes: states, bf16 states, gates, gate gradients and
    their bf16 copy, from NaN-free buffers whatever the operands of the padded frames hold."""
    from espnet_amd.lm.rnn_train import BiLSTMTape
    H, B, T, bf = 24, 5, 7, dtype == torch.bfloat16
    _, lays = _layers(H, 4, dtype, 77)
    gen = torch.Generator(device="cuda").manual_seed(9)
    xproj = [torch.randn(T * B, 4 * H, generator=gen, device="cuda") for _ in range(2)]
    dy = torch.randn(T * B, 2 * H, generator=gen, device="cuda")
    lens = torch.tensor(MASK_LENS, dtype=torch.long, device="cuda")
    tape = BiLSTMTape(lays, lens, T, B, "cuda")
    tape.forward(xproj)
    tape.backward(dy)
    pad = torch.arange(T, device="cuda")[:, None] >= lens[None, :]
    for d in range(2):
        hs = tape.hs[d][:T] if d else tape.hs[d][1:]
        cs = tape.cs[d][:T] if d else tape.cs[d][1:]
        for name, t in (("h", hs), ("c", cs), ("gates", tape.gates[d]), ("dgates", tape.dg[d])):
            assert not bool(t.isnan().any()), f"{name}[{d}]"
            assert float(t[pad].abs().max()) == 0.0, f"{name}[{d}] on padded steps"
        if bf:
            hb = tape.hb[d][:T] if d else tape.hb[d][1:]
            assert float(hb[pad].float().abs().max()) == 0.0
            assert float(tape.dgm[d].view(T, B, -1)[pad].float().abs().max()) == 0.0
    # the longest rows are untouched by the mask: non-zero everywhere
    assert float(tape.outputs().view(T, B, -1)[:, 1].abs().min()) > 0.0
