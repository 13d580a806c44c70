"""Loader of the BLSTM(P) encoder fixtures written by tests/capture_rnn_encoder_goldens.py, the
tolerance rule that goes with them (tests/lstm_train_goldens.py tolerance) and a restatement of
the encoder's forward in plain torch (restate): any dtype, given dropout masks, and optionally
the bf16 operand rounding of the HIP path."""
import numpy as np
import torch
import torch.nn.functional as F

from goldens import load, section
from lstm_train_goldens import tolerance, ulp32  # noqa: F401

NAMES = ("rnn_enc_tiny", "rnn_enc_noproj", "rnn_enc_uni", "rnn_enc_wide")
STORED = ("rnn_enc_tiny", "rnn_enc_noproj", "rnn_enc_uni")  # weights and whole gradients in the fixture
MARGIN = 4


_NUDGE = 0.0  # see restate(nudge=...)


def rd(t):
    """Round to bf16 and back (the value a bf16 operand holds).  With _NUDGE = e the rounding
    decision is taken on t (1 + e): every element within a relative e of a bf16 rounding boundary
    (on the side e points to) takes the other neighbour."""
    return (t * (1.0 + _NUDGE)).float().to(torch.bfloat16).to(t.dtype)


class _BfLinear(torch.autograd.Function):
    """y = rd(x) rd(w)^T + b with the backward's products on rounded operands too: dx = rd(dy)
    rd(w), dw = rd(dy)^T rd(x); the bias gradient sums the unrounded dy (rnn_decoder_goldens.py's,
    on this module's rd)."""

    @staticmethod
    def forward(ctx, x, w, b):
        xr, wr = rd(x), w.float().to(torch.bfloat16).to(w.dtype)  # (a weight is the same f32 number everywhere)
        ctx.save_for_backward(xr, wr)
        ctx.has_b = b is not None
        y = xr @ wr.t()
        return y + b if b is not None else y

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        dyr = rd(dy)
        return dyr @ wr, dyr.t() @ xr, (dy.sum(0) if ctx.has_b else None)


def encoder_kwargs(cfg):
    return dict(input_size=cfg["F"], rnn_type="lstm", bidirectional=cfg["bidirectional"],
                use_projection=cfg["use_projection"], num_layers=cfg["layers"], hidden_size=cfg["H"],
                output_size=cfg["proj"], dropout=0.0, subsample=cfg["subsample"])


def sub_law(cfg):
    """The subsampling factor after each layer (rnn_encoder.py:48-58; RNN applies none)."""
    if not cfg["use_projection"]:
        return [1] * cfg["layers"]
    s = list(cfg["subsample"] or [])[:cfg["layers"]]
    return s + [1] * (cfg["layers"] - len(s))


def out_frames(cfg, T):
    for s in sub_law(cfg):
        T = -(-T // s)
    return T


def make_inputs(cfg):
    """The fixture's inputs from its seed (kept in the fixture too for the stored ones): xs_pad with
    junk in the padded frames, ilens, the cotangent on the output."""
    g = torch.Generator().manual_seed(1000 + cfg["seed"])
    B, T = len(cfg["ilens"]), max(cfg["ilens"])
    xs = torch.randn(B, T, cfg["F"], generator=g)
    cot = torch.randn(B, out_frames(cfg, T), cfg["proj"], generator=g)
    return dict(xs_pad=xs, ilens=torch.tensor(cfg["ilens"]), cot=cot)


def build(name, enc_cls, dropout=0.0):
    """-> (cfg, d, encoder on the CPU with the fixture's weights, inputs)."""
    cfg, d = load(name)
    kw = dict(encoder_kwargs(cfg), dropout=dropout)
    if name in STORED:
        enc = enc_cls(**kw)
        enc.load_state_dict({k: torch.from_numpy(v) for k, v in section(d, "w").items()})
        inp = {k: torch.from_numpy(v) for k, v in section(d, "in").items()}
    else:
        torch.manual_seed(cfg["seed"])
        enc = enc_cls(**kw)
        sd, sums = enc.state_dict(), section(d, "wsum")
        assert list(sd) == list(sums), "state_dict layout differs from the reference's"
        for k, v in sums.items():
            np.testing.assert_allclose(sd[k].double().sum().item(), float(v), rtol=1e-12, atol=1e-12, err_msg=k)
        inp = make_inputs(cfg)
    return cfg, d, enc, inp


def _lstm_dir(x, lens, p, name, reverse, lin):
    """One direction of nn.LSTM on a packed sequence, time-major x (T, B, I): row b takes the
    frames t < lens[b], the reverse direction starts from zero at lens[b] - 1, padded outputs 0."""
    T, B, _ = x.shape
    sfx = "_reverse" if reverse else ""
    w_ih, w_hh = p[f"{name}.weight_ih_l{sfx}"], p[f"{name}.weight_hh_l{sfx}"]
    H = w_hh.shape[1]
    xproj = lin(x.reshape(T * B, -1), w_ih, p[f"{name}.bias_ih_l{sfx}"] + p[f"{name}.bias_hh_l{sfx}"]).view(T, B, -1)
    h = torch.zeros(B, H, dtype=x.dtype)
    c = torch.zeros(B, H, dtype=x.dtype)
    out = [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        gi, gf, gg, go = (xproj[t] + lin(h, w_hh)).chunk(4, dim=1)
        c2 = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
        h2 = torch.sigmoid(go) * torch.tanh(c2)
        act = (t < lens).unsqueeze(1)
        c = torch.where(act, c2, torch.zeros_like(c2))
        h = torch.where(act, h2, torch.zeros_like(h2))
        out[t] = h
    return torch.stack(out)


def restate(sd, cfg, inp, dtype=torch.float64, bf=False, masks=None, nudge=0.0):
    global _NUDGE
    _NUDGE = float(nudge)
    try:
        return _restate(sd, cfg, inp, dtype, bf, masks)
    finally:
        _NUDGE = 0.0


def _restate(sd, cfg, inp, dtype, bf, masks):
    """RNNEncoder.forward (espnet2/asr/encoder/rnn_encoder.py over RNNP / RNN of
    espnet/nets/pytorch_backend/rnn/encoders.py) in `dtype` on the CPU, differentiated by autograd
    under the cotangent inp["cot"].

    bf: every matrix product, forward and backward, takes operands rounded to bf16 where the HIP
    path rounds them (_BfLinear: both LSTM products of every direction, the projections); sums,
    the cells, tanh and the bias gradients stay in `dtype`.
    masks: dropout factors (0 or 1 / (1 - p)), time-major rows: "proj{i}" (T_i * B, proj) on the
    output of RNNP's projection i, "layer{k}" (T * B, ndir * H) on the output of RNN's layer k; a
    missing key is no dropout.
    nudge (restate's; with bf): the bf16 rounding decisions are taken on operand (1 + nudge): the
    restatement another computation of the same operands, off by a relative |nudge|, would give
    where it lands on the other side of a rounding boundary (the capture's bf.err).
    -> (out (B, T', D), olens, {name: gradient, "xs_pad": ..})."""
    masks = masks or {}
    p = {k[len("enc.0."):]: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    xs = inp["xs_pad"].detach().clone().to(dtype).requires_grad_(True)
    lens = inp["ilens"].clone()
    B, T, _ = xs.shape
    lin = (lambda x, w, b=None: _BfLinear.apply(x, w, b)) if bf else (lambda x, w, b=None: F.linear(x, w, b))
    ndir = 2 if cfg["bidirectional"] else 1
    x = xs.transpose(0, 1)  # (T, B, F)
    L = cfg["layers"]

    def layer(x, name, k):
        q = {kk.replace(f"_l{k}", "_l"): v for kk, v in p.items() if kk.startswith(name + ".") and f"_l{k}" in kk}
        return torch.cat([_lstm_dir(x, lens, q, name, bool(d), lin) for d in range(ndir)], dim=2)

    if cfg["use_projection"]:
        pre = "birnn" if ndir == 2 else "rnn"
        for i, sub in enumerate(sub_law(cfg)):
            x = layer(x, f"{pre}{i}", 0)
            if sub > 1:
                x = x[::sub]
                lens = (lens + 1) // sub
            Ti = x.shape[0]
            x = lin(x.reshape(Ti * B, -1), p[f"bt{i}.weight"], p[f"bt{i}.bias"])
            if i < L - 1:
                if f"proj{i}" in masks:
                    x = x * masks[f"proj{i}"].to(dtype)
                x = torch.tanh(x)
            x = x.view(Ti, B, -1)
    else:
        for k in range(L):
            x = layer(x, "nbrnn", k)
            if f"layer{k}" in masks:
                x = x * masks[f"layer{k}"].to(dtype).view(x.shape)
        Ti = x.shape[0]
        x = torch.tanh(lin(x.reshape(Ti * B, -1), p["l_last.weight"], p["l_last.bias"])).view(Ti, B, -1)
    out = x.transpose(0, 1)
    out = out.masked_fill((torch.arange(out.shape[1]).unsqueeze(0) >= lens.unsqueeze(1)).unsqueeze(2), 0.0)
    (out * inp["cot"].to(dtype)).sum().backward()
    grads = {"enc.0." + k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in p.items()}
    grads["xs_pad"] = xs.grad.detach()
    return out.detach(), lens, grads


def prepare_encoder(enc, amp=False, device="cuda:0"):
    """Bind a stand-alone encoder to a parameter arena of its own, as ESPnetASRModel.prepare does
    for its encoder.  -> the arena (keep it alive)."""
    from espnet_amd.arena import ParamArena
    holder = torch.nn.Module()
    holder.encoder = enc
    cd = torch.bfloat16 if amp else torch.float32
    arena = ParamArena(holder, torch.device(device), enc.arena_groups("encoder."), shadow_dtype=cd)
    anchor = torch.zeros(1, device=device, requires_grad=True)
    enc.bind(arena, "encoder.", cd, anchor)
    object.__setattr__(enc, "_holder", holder)  # (kept alive; not a submodule: the holder owns enc)
    return arena
