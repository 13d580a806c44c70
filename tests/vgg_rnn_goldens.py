"""Loader of the VGG2L + BLSTM(P) encoder fixtures written by tests/capture_vgg_rnn_goldens.py and
the tolerance rule that goes with them (tests/lstm_train_goldens.py tolerance, MARGIN 4).

The fixtures keep no weights: VGG2L alone has 259,008 parameters, more than a fixture may hold.  They
are regenerated from cfg.seed and checked against the recorded f64 sums (wsum.*); of every gradient
the fixture holds a strided sample of at most 4096 elements (gsamp.*, stride in cfg.gstride) with
its f64 L2 norm (gnorm.*).  bf16: bf.err.* (the tolerance yardstick of the restatement below with
bf=True on given decisions), cfg.bands (per convolution: how close to a decision boundary a kernel's
decision may differ from the restatement's own) and cfg.bf_nudge; see the capture script."""
import numpy as np
import torch

from goldens import load, section
from lstm_train_goldens import tolerance, ulp32  # noqa: F401
from rnn_encoder_goldens import prepare_encoder  # noqa: F401

NAMES = ("vgg_rnn_tiny", "vgg_rnn_noproj", "vgg_rnn_f83")
MARGIN = 4
CONVS = ("conv1_1", "conv1_2", "conv2_1", "conv2_2")


def encoder_kwargs(cfg):
    return dict(input_size=cfg["F"], rnn_type="lstm", bidirectional=cfg["bidirectional"],
                use_projection=cfg["use_projection"], num_layers=cfg["layers"], hidden_size=cfg["H"],
                output_size=cfg["proj"], dropout=0.0, in_channel=1)


def half2(n):
    """ceil(ceil(n / 2) / 2): what the two ceil-mode pools leave of an extent or a length."""
    return -(-(-(-n // 2)) // 2)


def make_inputs(cfg):
    """xs_pad with junk in the padded frames, unequal ilens, the cotangent on the output."""
    g = torch.Generator().manual_seed(1000 + cfg["seed"])
    B, T = len(cfg["ilens"]), max(cfg["ilens"])
    xs = torch.randn(B, T, cfg["F"], generator=g)
    cot = torch.randn(B, half2(T), cfg["proj"], generator=g)
    return dict(xs_pad=xs, ilens=torch.tensor(cfg["ilens"]), cot=cot)


def build(name, enc_cls):
    """-> (cfg, d, encoder on the CPU rebuilt from the fixture's seed, inputs)."""
    cfg, d = load(name)
    torch.manual_seed(cfg["seed"])
    enc = enc_cls(**encoder_kwargs(cfg))
    sd, sums = enc.state_dict(), section(d, "wsum")
    assert list(sd) == list(sums), "state_dict layout differs from the reference's"
    for k, v in sums.items():
        np.testing.assert_allclose(sd[k].double().sum().item(), float(v), rtol=1e-12, atol=1e-12, err_msg=k)
    return cfg, d, enc, make_inputs(cfg)


def pool_gap(y):
    """Of a ReLU output y (B, C, H, W): per 2x2 ceil-mode window the gap between its two largest
    values, +inf where the window has one element or holds no positive value (nothing to decide:
    the first position wins and no gradient passes)."""
    B, C, H, W = y.shape
    pad = torch.full((B, C, H + H % 2, W + W % 2), -1.0, dtype=y.dtype)
    pad[:, :, :H, :W] = y
    win = torch.stack([pad[:, :, a::2, b::2] for a in (0, 1) for b in (0, 1)], dim=-1)
    top = win.sort(dim=-1, descending=True).values
    gap = top[..., 0] - top[..., 1]
    gap[(top[..., 0] <= 0) | (top[..., 1] < 0)] = float("inf")
    return gap


def decision_room(pre32, pre64, margin=MARGIN):
    """How far the float64 run stays from a decision boundary, in units of margin x the f32 error of
    the array the decision is taken on: the smallest, over the four convolution outputs, of
    |pre-activation| and (conv1_2, conv2_2) of the pooling windows' top-two gaps.  > 1: every ReLU
    and argmax decision of an f32 computation within the tolerance is the float64 one."""
    room = float("inf")
    for n in CONVS:
        e = margin * float((pre32[n].double() - pre64[n].double()).abs().max())
        room = min(room, float(pre64[n].abs().min()) / e)
        if n.endswith("_2"):
            room = min(room, float(pool_gap(torch.relu(pre64[n])).min()) / e)
    return room


def pool_scan(y):
    """max_pool2d(2, 2, ceil_mode) of a ReLU output by the reference's scan: dt outer, df inner,
    strict >, so ties keep the first.  -> (values, argmax 2 * dt + df)."""
    B, C, H, W = y.shape
    pad = torch.full((B, C, H + H % 2, W + W % 2), float("-inf"), dtype=y.dtype)
    pad[:, :, :H, :W] = y
    best = pad[:, :, 0::2, 0::2].clone()
    arg = torch.zeros(best.shape, dtype=torch.long)
    for pos in (1, 2, 3):
        v = pad[:, :, pos >> 1::2, pos & 1::2]
        m = v > best
        best = torch.where(m, v, best)
        arg[m] = pos
    return best, arg


def pool_pick(y, arg):
    """The value of each 2x2 ceil-mode window of y at the given position arg = 2 * dt + df."""
    B, C, H, W = y.shape
    pad = torch.zeros(B, C, H + H % 2, W + W % 2, dtype=y.dtype)
    pad[:, :, :H, :W] = y
    win = torch.stack([pad[:, :, a::2, b::2] for a in (0, 1) for b in (0, 1)], dim=-1)
    return win.gather(-1, arg.unsqueeze(-1)).squeeze(-1)


def pool_scatter(dp, arg, relu, H, W):
    """The pooled gradient dp put at each window's winner, through the ReLU mask (B, C, H, W)."""
    B, C, H2, W2 = dp.shape
    full = torch.zeros(B, C, 2 * H2, 2 * W2, dtype=dp.dtype)
    for pos in range(4):
        full[:, :, pos >> 1::2, pos & 1::2] = dp * (arg == pos)
    return full[:, :, :H, :W] * relu


def conv_dw(x, dy, shape):
    return torch.nn.grad.conv2d_weight(x, shape, dy, padding=1)


def restate(sd, cfg, inp, dtype=torch.float64, bf=False, decisions=None, nudge=0.0):
    """VGGRNNEncoder.forward and its backward under the cotangent inp["cot"], written out on the CPU
    in `dtype`: VGG2L layer by layer with explicit decisions, then tests/rnn_encoder_goldens.py
    restate for the RNNP / RNN body (subsample all ones).

    bf: operands are rounded to bf16 where the HIP path rounds them: the weights of conv1_2, conv2_1
    and conv2_2; the stored activations (conv1_1's output, the first pooled map, conv2_1's output);
    the stored gradients (of conv2_1's and conv1_1's pre-activations); the pooled layers' gradients as
    the matrix operand their kernels read through the decisions; and the body's operands (its own
    bf).  conv1_1 works on f32 weights and features in both dtypes; the last pooled map, the gradient
    of the first pooled map and every bias gradient are not rounded.
    decisions: the ReLU masks relu0..3 (bool, NCHW) and argmax indices pool0..1 (2 * dt + df) to
    take instead of this computation's own (VGG2L.decisions() of a kernel run).
    nudge (with bf): every activation / gradient rounding decision is taken on operand x (1 + nudge).
    -> (out (B, T', D), olens, {parameter name: gradient}, {conv name: its output before the ReLU},
        the decisions taken)."""
    import torch.nn.functional as F

    import rnn_encoder_goldens as R

    def rd(t):
        return (t * (1.0 + nudge)).float().to(torch.bfloat16).to(t.dtype) if bf else t

    def rw(t):  # (a weight is the same f32 number everywhere)
        return t.float().to(torch.bfloat16).to(t.dtype) if bf else t

    w = {n: sd[f"enc.0.{n}.weight"].detach().to(dtype) for n in CONVS}
    b = {n: sd[f"enc.0.{n}.bias"].detach().to(dtype) for n in CONVS}
    wr = {n: (w[n] if n == "conv1_1" else rw(w[n])) for n in CONVS}
    xs = inp["xs_pad"].detach().to(dtype).unsqueeze(1)
    pre, D = {}, {}

    def relu(i, x):
        D[f"relu{i}"] = decisions[f"relu{i}"].bool() if decisions is not None else x > 0
        return torch.where(D[f"relu{i}"], x, torch.zeros_like(x))

    def pool(j, y):
        if decisions is None:
            v, D[f"pool{j}"] = pool_scan(y)
            return v
        D[f"pool{j}"] = decisions[f"pool{j}"].long()
        return pool_pick(y, D[f"pool{j}"])

    pre["conv1_1"] = F.conv2d(xs, wr["conv1_1"], b["conv1_1"], padding=1)
    x1 = rd(relu(0, pre["conv1_1"]))
    pre["conv1_2"] = F.conv2d(x1, wr["conv1_2"], b["conv1_2"], padding=1)
    p1 = rd(pool(0, relu(1, pre["conv1_2"])))
    pre["conv2_1"] = F.conv2d(p1, wr["conv2_1"], b["conv2_1"], padding=1)
    x3 = rd(relu(2, pre["conv2_1"]))
    pre["conv2_2"] = F.conv2d(x3, wr["conv2_2"], b["conv2_2"], padding=1)
    x4 = pool(1, relu(3, pre["conv2_2"]))
    B, C, T4, F4 = x4.shape
    feats = x4.transpose(1, 2).reshape(B, T4, C * F4)
    lens = (((inp["ilens"] + 1) // 2) + 1) // 2
    body = {"enc.0." + k[len("enc.1."):]: v for k, v in sd.items() if k.startswith("enc.1.")}
    out, olens, g = R.restate(body, dict(cfg, subsample=[1] * cfg["layers"]),
                              dict(xs_pad=feats, ilens=lens, cot=inp["cot"]), dtype, bf=bf, nudge=nudge)
    d4 = g.pop("xs_pad").to(dtype).view(B, T4, C, F4).transpose(1, 2)
    grads = {"enc.1." + k[len("enc.0."):]: v for k, v in g.items()}

    def put(n, dw, db):
        grads[f"enc.0.{n}.weight"], grads[f"enc.0.{n}.bias"] = dw, db

    (H, W), (H2, W2) = xs.shape[2:], p1.shape[2:]
    g3 = pool_scatter(d4, D["pool1"], D["relu3"], H2, W2)
    g3r = rd(g3)
    put("conv2_2", conv_dw(x3, g3r, w["conv2_2"].shape), g3.sum((0, 2, 3)))
    d3 = rd(F.conv_transpose2d(g3r, wr["conv2_2"], padding=1) * D["relu2"])
    put("conv2_1", conv_dw(p1, d3, w["conv2_1"].shape), d3.sum((0, 2, 3)))
    dp1 = F.conv_transpose2d(d3, wr["conv2_1"], padding=1)
    g1 = pool_scatter(dp1, D["pool0"], D["relu1"], H, W)
    g1r = rd(g1)
    put("conv1_2", conv_dw(x1, g1r, w["conv1_2"].shape), g1.sum((0, 2, 3)))
    d1 = rd(F.conv_transpose2d(g1r, wr["conv1_2"], padding=1) * D["relu0"])
    put("conv1_1", conv_dw(xs, d1, w["conv1_1"].shape), d1.sum((0, 2, 3)))
    return out, olens, grads, pre, D


def bands(pre_base, pre_alts, margin=MARGIN):
    """Per convolution: margin x the largest deviation of its output among the alternative runs."""
    return {n: margin * max(float((a[n].double() - pre_base[n].double()).abs().max()) for a in pre_alts)
            for n in CONVS}


def in_band(pre, band):
    """-> ({relu i: bool mask of pre-activations within the layer's band of 0},
           {pool j: bool mask of windows whose top-two gap is within the band})."""
    relu = {i: pre[n].abs() <= band[n] for i, n in enumerate(CONVS)}
    pool = {j: pool_gap(torch.relu(pre[n])) <= band[n] for j, n in enumerate(("conv1_2", "conv2_2"))}
    return relu, pool
