"""Loader of the LM-training fixtures written by tests/capture_lstm_train_goldens.py, the
tolerance rule that goes with them and a float64 restatement of the training forward with given
dropout masks."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from goldens import load, section

NAMES = ("lstm_train_tiny", "lstm_train_nhid", "lstm_train_650")
STORED = ("lstm_train_tiny", "lstm_train_nhid")  # weights and whole gradients in the fixture


def ulp32(x: float) -> float:
    """The spacing of float32 at magnitude x."""
    return 2.0 ** (math.floor(math.log2(x)) - 23) if x > 0 else 2.0 ** -149


def tolerance(ref, err, margin) -> float:
    """margin x the reference's own f32-vs-f64 error of the array, or 4 ulps of float32 at the
    array's magnitude where that is larger (a deviation no f32 computation can be held below:
    it is what a different summation order costs)."""
    mag = float(np.abs(np.asarray(ref, dtype=np.float64)).max())
    return max(margin * float(err), 4 * ulp32(mag))


def build(name, lm_cls, model_cls, dropout_rate=0.0):
    """-> (cfg, d, ESPnetLanguageModel on the CPU with the fixture's weights)."""
    cfg, d = load(name)
    conf = dict(cfg["lm_conf"], dropout_rate=dropout_rate)
    if name in STORED:
        lm = lm_cls(**conf)
        lm.load_state_dict({k: torch.from_numpy(v) for k, v in section(d, "w").items()})
    else:
        torch.manual_seed(cfg["seed"])
        lm = lm_cls(**conf)
        sd, sums = lm.state_dict(), section(d, "wsum")
        assert list(sd) == list(sums), "state_dict layout differs from the reference's"
        for k, v in sums.items():
            np.testing.assert_allclose(sd[k].double().sum().item(), float(v), rtol=1e-12, atol=1e-12, err_msg=k)
    return cfg, d, model_cls(lm, conf["vocab_size"])


def batch(d):
    return torch.from_numpy(d["in.text"]), torch.from_numpy(d["in.text_lengths"])


def restate_train(sd, text, lens, V, masks, p_drop, dtype=torch.float64):
    """ESPnetLanguageModel(SequentialRNNLM) forward + loss in `dtype` on the CPU with the given
    dropout keep-masks (time-major (T*B, width) 0/1 tensors: "embed", "rnn{k}", "out"; scale
    1 / (1 - p)), differentiated by autograd.  -> (loss, nll (B, T), {name: gradient})."""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    x = F.pad(text, [1, 0], "constant", V - 1)
    t = F.pad(text, [0, 1], "constant", 0)
    for i, n in enumerate(lens.tolist()):
        t[i, n] = V - 1
    B, T = x.shape
    L = sum(1 for k in p if k.startswith("rnn.weight_ih_l"))
    H = p["rnn.weight_hh_l0"].shape[1]

    def drop(v, key):  # v (T, B, width)
        if key not in masks:
            return v
        return v * masks[key].to(dtype).view(T, B, -1) / (1.0 - p_drop[key])

    seq = drop(p["encoder.weight"][x.t()], "embed")  # (T, B, ninp)
    for k in range(L):
        w_ih, w_hh = p[f"rnn.weight_ih_l{k}"], p[f"rnn.weight_hh_l{k}"]
        b = p[f"rnn.bias_ih_l{k}"] + p[f"rnn.bias_hh_l{k}"]
        h = torch.zeros(B, H, dtype=dtype)
        c = torch.zeros(B, H, dtype=dtype)
        outs = []
        for s in range(T):
            g = seq[s] @ w_ih.t() + h @ w_hh.t() + b
            gi, gf, gg, go = g.chunk(4, dim=1)
            c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
            h = torch.sigmoid(go) * torch.tanh(c)
            outs.append(h)
        seq = torch.stack(outs)
        if k < L - 1:
            seq = drop(seq, f"rnn{k}")
    seq = drop(seq, "out")
    logits = seq @ p["decoder.weight"].t() + p["decoder.bias"]  # (T, B, V)
    nll = F.cross_entropy(logits.reshape(-1, V), t.t().reshape(-1), reduction="none").view(T, B).t()
    mask = torch.arange(T).unsqueeze(0) >= (lens + 1).unsqueeze(1)
    nll = nll.masked_fill(mask, 0.0)
    loss = nll.sum() / (lens + 1).sum()
    loss.backward()
    g = {k: v.grad.detach() for k, v in p.items()}
    g["encoder.weight"][0] = 0  # padding_idx
    return loss.detach(), nll.detach(), g


def restate_bf16(sd, text, lens, V, dtype=torch.float64):
    """The bf16 (amp) training step restated on the CPU in `dtype`, forward AND backward written
    out, with every matrix product's operands rounded to bf16 where the HIP path rounds them:

      forward   X, h_{t-1}, the last layer's output and W_ih, W_hh, decoder.weight
      backward  dlogits and decoder.weight / the decoder's input (dX, dW of the output Linear),
                dgates[t+1] and W_hh (the recurrent product), dgates and W_ih / X / h_{t-1}
                (dX, dW_ih, dW_hh)

    Sums, biases, states, gates, the cell's forward and backward and the bias gradients (column
    sums of the unrounded dlogits / dgates) stay in `dtype`.
    -> (loss, nll (B, T), {name: gradient})."""
    rd = lambda t: t.float().to(torch.bfloat16).to(dtype)  # noqa: E731
    p = {k: v.detach().to(dtype) for k, v in sd.items()}
    x = F.pad(text, [1, 0], "constant", V - 1)
    t = F.pad(text, [0, 1], "constant", 0)
    for i, n in enumerate(lens.tolist()):
        t[i, n] = V - 1
    B, T = x.shape
    L = sum(1 for k in p if k.startswith("rnn.weight_ih_l"))
    H = p["rnn.weight_hh_l0"].shape[1]
    tok = x.t().reshape(-1)  # time-major rows
    seq = p["encoder.weight"][tok]  # (T*B, ninp)
    saved = []
    for k in range(L):
        w_ih, w_hh = rd(p[f"rnn.weight_ih_l{k}"]), rd(p[f"rnn.weight_hh_l{k}"])
        xc = rd(seq)
        xproj = (xc @ w_ih.t() + (p[f"rnn.bias_ih_l{k}"] + p[f"rnn.bias_hh_l{k}"])).view(T, B, 4 * H)
        h, c = torch.zeros(B, H, dtype=dtype), torch.zeros(B, H, dtype=dtype)
        hprev, cs, gates, outs = [], [c], [], []
        for s in range(T):
            hb = rd(h)
            hprev.append(hb)
            gi, gf, gg, go = (xproj[s] + hb @ w_hh.t()).chunk(4, dim=1)
            gi, gf, gg, go = torch.sigmoid(gi), torch.sigmoid(gf), torch.tanh(gg), torch.sigmoid(go)
            c = gf * c + gi * gg
            h = go * torch.tanh(c)
            cs.append(c)
            gates.append((gi, gf, gg, go))
            outs.append(h)
        saved.append((xc, w_ih, w_hh, torch.cat(hprev), cs, gates))
        seq = torch.cat(outs)  # (T*B, H)
    xd, wd = rd(seq), rd(p["decoder.weight"])
    logits = xd @ wd.t() + p["decoder.bias"]
    tgt = t.t().reshape(-1)
    valid = (torch.arange(T).unsqueeze(1) < (lens + 1).unsqueeze(0)).reshape(-1)  # (T, B) time-major
    ntok = int((lens + 1).sum())
    logp = torch.log_softmax(logits, dim=1)
    nll = -logp.gather(1, tgt.view(-1, 1)).view(-1) * valid
    loss = nll.sum() / ntok
    # ---- backward
    g = {}
    dlog = torch.softmax(logits, dim=1)
    dlog[torch.arange(T * B), tgt] -= 1.0
    dlog = dlog * valid.view(-1, 1).to(dtype) / ntok
    dyc = rd(dlog)
    g["decoder.weight"] = dyc.t() @ xd
    g["decoder.bias"] = dlog.sum(0)
    dy = dyc @ wd
    for k in range(L - 1, -1, -1):
        xc, w_ih, w_hh, hprev, cs, gates = saved[k]
        dy = dy.view(T, B, H)
        dg = [None] * T
        dc = torch.zeros(B, H, dtype=dtype)
        for s in range(T - 1, -1, -1):
            dh = dy[s] if s == T - 1 else dy[s] + rd(dg[s + 1]) @ w_hh
            gi, gf, gg, go = gates[s]
            tc = torch.tanh(cs[s + 1])
            d_o = dh * tc * go * (1 - go)
            dcc = dc + dh * go * (1 - tc * tc)
            d_i = dcc * gg * gi * (1 - gi)
            d_f = dcc * cs[s] * gf * (1 - gf)
            d_g = dcc * gi * (1 - gg * gg)
            dc = dcc * gf
            dg[s] = torch.cat([d_i, d_f, d_g, d_o], dim=1)
        dg = torch.cat(dg)  # (T*B, 4H)
        dgm = rd(dg)
        g[f"rnn.weight_ih_l{k}"] = dgm.t() @ xc
        g[f"rnn.weight_hh_l{k}"] = dgm.t() @ hprev
        g[f"rnn.bias_ih_l{k}"] = g[f"rnn.bias_hh_l{k}"] = dg.sum(0)
        dy = dgm @ w_ih
    gE = torch.zeros_like(p["encoder.weight"])
    gE.index_add_(0, tok, dy)
    gE[0] = 0  # padding_idx
    g["encoder.weight"] = gE
    return loss, nll.view(T, B).t(), g
