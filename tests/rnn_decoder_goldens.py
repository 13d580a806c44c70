"""Loader of the attention-RNN decoder fixtures written by tests/capture_rnn_decoder_goldens.py,
the tolerance rule that goes with them (tests/lstm_train_goldens.py tolerance)
and a restatement of the decoder's training forward in plain torch (restate): any dtype, given
dropout masks, and optionally the bf16 operand rounding of the HIP path."""
import numpy as np
import torch
import torch.nn.functional as F

from goldens import load, section
from lstm_train_goldens import tolerance, ulp32  # noqa: F401

NAMES = ("rnn_dec_tiny", "rnn_dec_one", "rnn_dec_wide")
STORED = ("rnn_dec_tiny", "rnn_dec_one")  # weights and whole gradients in the fixture
MARGIN = 4
# gradients that are exact-zero sums (their values are rounding noise of the terms): held to 4 ulps
# at the recorded magnitude of the sum of the terms' absolute values (mag.<name>)
ZERO_SUM_GRADS = ("att_list.0.gvec.bias",)


def rd(t):
    """Round to bf16 and back (the value a bf16 operand or a bf16 store holds)."""
    return t.float().to(torch.bfloat16).to(t.dtype)


class _BfLinear(torch.autograd.Function):
    """y = rd(x) rd(w)^T + b with the backward's products on rounded operands too: dx = rd(dy)
    rd(w), dw = rd(dy)^T rd(x); the bias gradient sums the unrounded dy."""

    @staticmethod
    def forward(ctx, x, w, b):
        xr, wr = rd(x), rd(w)
        ctx.save_for_backward(xr, wr)
        ctx.has_b = b is not None
        y = xr @ wr.t()
        return y + b if b is not None else y

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        dyr = rd(dy)
        return dyr @ wr, dyr.t() @ xr, (dy.sum(0) if ctx.has_b else None)


class _BfStore(torch.autograd.Function):
    """A tensor kept in bf16 memory: rounded forward, the gradient passes unchanged."""

    @staticmethod
    def forward(ctx, x):
        return rd(x)

    @staticmethod
    def backward(ctx, dy):
        return dy


def decoder_kwargs(cfg):
    return dict(vocab_size=cfg["V"], encoder_output_size=cfg["E"], rnn_type="lstm", num_layers=cfg["layers"],
                hidden_size=cfg["H"], dropout=0.0,
                att_conf=dict(atype="location", adim=cfg["A"], aconv_chans=cfg["C"], aconv_filts=cfg["F"]))


def make_inputs(cfg):
    """The fixture's inputs from its seed (kept in the fixture too for the stored ones): hs_pad with
    junk in the padded frames, hlens, ys_in_pad padded with <eos>, ys_in_lens, the cotangent."""
    g = torch.Generator().manual_seed(1000 + cfg["seed"])
    B, T, E, L, V = len(cfg["hlens"]), max(cfg["hlens"]), cfg["E"], max(cfg["ylens"]), cfg["V"]
    hs = torch.randn(B, T, E, generator=g)
    ys = torch.full((B, L), V - 1, dtype=torch.long)
    for i, n in enumerate(cfg["ylens"]):
        ys[i, :n] = torch.randint(1, V - 1, (n,), generator=g)
        ys[i, 0] = V - 1  # <sos>
    cot = torch.randn(B, L, V, generator=g)
    return dict(hs_pad=hs, hlens=torch.tensor(cfg["hlens"]), ys_in_pad=ys, ys_in_lens=torch.tensor(cfg["ylens"]),
                cot=cot)


def build(name, dec_cls, dropout=0.0):
    """-> (cfg, d, decoder on the CPU with the fixture's weights, inputs)."""
    cfg, d = load(name)
    kw = dict(decoder_kwargs(cfg), dropout=dropout)
    if name in STORED:
        dec = dec_cls(**kw)
        dec.load_state_dict({k: torch.from_numpy(v) for k, v in section(d, "w").items()})
        inp = {k: torch.from_numpy(v) for k, v in section(d, "in").items()}
    else:
        torch.manual_seed(cfg["seed"])
        dec = dec_cls(**kw)
        sd, sums = dec.state_dict(), section(d, "wsum")
        assert list(sd) == list(sums), "state_dict layout differs from the reference's"
        for k, v in sums.items():
            np.testing.assert_allclose(sd[k].double().sum().item(), float(v), rtol=1e-12, atol=1e-12, err_msg=k)
        inp = make_inputs(cfg)
    return cfg, d, dec, inp


def restate(sd, inp, dtype=torch.float64, bf=False, masks=None):
    """RNNDecoder.forward (espnet2/asr/decoder/rnn_decoder.py:167-249 over AttLoc) in `dtype` on the
    CPU, differentiated by autograd under the cotangent inp["cot"].

    bf: every matrix product, forward and backward, takes operands rounded to bf16 where the HIP
    path rounds them (_BfLinear: mlp_enc, mlp_dec, both LSTM products of every layer, the output
    Linear), pre_enc and the encoder memory the attention reads are bf16 stores (_BfStore); sums,
    tanh, softmax, the cells and the bias gradients stay in `dtype`.
    masks: dropout factors (0 or 1 / (1 - p)), time-major: "emb" (L, B, H), "query" (L, B, H; row
    0 unused), "layer{l}" (L, B, H), "out" (L, B, H); a missing key is no dropout.
    -> (logits (B, L, V), att_w (L, B, T), {name: gradient, "hs_pad": ..}, sum |de|)."""
    masks = masks or {}
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    hs = inp["hs_pad"].detach().clone().to(dtype).requires_grad_(True)
    hlens, ys, ylens = inp["hlens"], inp["ys_in_pad"], inp["ys_in_lens"]
    B, T, E = hs.shape
    L = ys.shape[1]
    H = p["embed.weight"].shape[1]
    NL = sum(1 for k in p if k.endswith("weight_hh"))
    Fw = (p["att_list.0.loc_conv.weight"].shape[-1] - 1) // 2
    lin = (lambda x, w, b=None: _BfLinear.apply(x, w, b)) if bf else (lambda x, w, b=None: F.linear(x, w, b))
    store = _BfStore.apply if bf else (lambda x: x)

    def m(v, key, i):
        return v * masks[key][i].to(dtype) if key in masks else v

    pad = torch.arange(T).unsqueeze(0) >= hlens.unsqueeze(1)  # (B, T)
    hm = store(hs)
    pre = store(lin(hm.reshape(B * T, E), p["att_list.0.mlp_enc.weight"], p["att_list.0.mlp_enc.bias"])).view(B, T, -1)
    K = p["att_list.0.loc_conv.weight"]
    z = [torch.zeros(B, H, dtype=dtype) for _ in range(NL)]
    c = [torch.zeros(B, H, dtype=dtype) for _ in range(NL)]
    aprev = (~pad).to(dtype) / hlens.to(dtype).unsqueeze(1)
    es, ws, outs = [], [], []
    for i in range(L):
        q = m(z[0], "query", i) if i > 0 else z[0]
        conv = F.conv2d(aprev.view(B, 1, 1, T), K, padding=(0, Fw)).squeeze(2).transpose(1, 2)  # (B, T, C)
        u = torch.tanh(conv @ p["att_list.0.mlp_att.weight"].t() + pre
                       + lin(q, p["att_list.0.mlp_dec.weight"]).view(B, 1, -1))
        e = (u @ p["att_list.0.gvec.weight"].t()).squeeze(2) + p["att_list.0.gvec.bias"]
        e.retain_grad()
        es.append(e)
        w = torch.softmax(2.0 * e.masked_fill(pad, float("-inf")), dim=1)
        ctxv = (hm * w.unsqueeze(2)).sum(1)
        ws.append(w)
        aprev = w
        x = torch.cat([m(p["embed.weight"][ys[:, i]], "emb", i), ctxv], dim=1)
        for l in range(NL):
            if l > 0:
                x = m(z[l - 1], f"layer{l}", i)
            g = lin(x, p[f"decoder.{l}.weight_ih"], p[f"decoder.{l}.bias_ih"] + p[f"decoder.{l}.bias_hh"]) \
                + lin(z[l], p[f"decoder.{l}.weight_hh"])
            gi, gf, gg, go = g.chunk(4, dim=1)
            c[l] = torch.sigmoid(gf) * c[l] + torch.sigmoid(gi) * torch.tanh(gg)
            z[l] = torch.sigmoid(go) * torch.tanh(c[l])
        outs.append(m(z[-1], "out", i))
    zall = torch.stack(outs, dim=1)  # (B, L, H)
    logits = lin(zall.reshape(B * L, H), p["output.weight"], p["output.bias"]).view(B, L, -1)
    logits = logits.masked_fill((torch.arange(L).unsqueeze(0) >= ylens.unsqueeze(1)).unsqueeze(2), 0.0)
    (logits * inp["cot"].to(dtype)).sum().backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in p.items()}
    grads["hs_pad"] = hs.grad.detach()
    de_abs = sum(float(e.grad.masked_fill(pad, 0.0).abs().sum()) for e in es)
    return logits.detach(), torch.stack(ws).detach(), grads, de_abs


def prepare_decoder(dec, amp=False, device="cuda:0"):
    """Bind a stand-alone decoder to a parameter arena of its own, as ESPnetASRModel.prepare does
    for its decoder.  -> the arena (keep it alive)."""
    from espnet_amd.arena import ParamArena
    holder = torch.nn.Module()
    holder.decoder = dec
    cd = torch.bfloat16 if amp else torch.float32
    arena = ParamArena(holder, torch.device(device), dec.arena_groups("decoder."), shadow_dtype=cd)
    dec.bind(arena, "decoder.", cd)
    object.__setattr__(dec, "_holder", holder)  # (kept alive; not a submodule: the holder owns dec)
    return arena
