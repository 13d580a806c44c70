"""Loader of the SequentialRNNLM fixtures written by tests/capture_rnn_lm_goldens.py."""
import os

import numpy as np
import torch

from goldens import GOLDEN, load, section

SMALL = ("rnn_lm_tiny", "rnn_lm_nhid")
SIZED = ("rnn_lm_650", "rnn_lm_2048")
RECIPES = ("librispeech_train_lm_adam", "aishell_train_lm", "laborotv_train_lm")


def weights(d):
    return {k: torch.from_numpy(v) for k, v in section(d, "w").items()}


def load_lm(name, cls):
    """-> (cfg, d, model on the CPU with the fixture's weights): stored for the small fixtures,
    regenerated from cfg.seed and checked against the stored per-tensor f64 sums for the sized."""
    cfg, d = load(name)
    if name in SMALL:
        lm = cls(**cfg["lm_conf"])
        lm.load_state_dict(weights(d))
        return cfg, d, lm
    torch.manual_seed(cfg["seed"])
    lm = cls(**cfg["lm_conf"])
    sd, sums = lm.state_dict(), section(d, "wsum")
    assert list(sd) == list(sums), "state_dict layout differs from the reference's"
    for k, v in sums.items():
        np.testing.assert_allclose(sd[k].double().sum().item(), float(v), rtol=1e-12, atol=1e-12, err_msg=k)
    return cfg, d, lm


def recipe(key):
    """The recipe YAML copied beside rnn_lm_recipes.npz -> its dict."""
    import yaml
    with open(os.path.join(GOLDEN, f"rnn_lm_{key}.yaml")) as f:
        return yaml.safe_load(f)


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def restate_forward(sd, ids, hidden=None, dtype=torch.float64, bf16=False):
    """seq_rnn_lm.py forward restated with plain tensor arithmetic on the CPU in `dtype`
    (Embedding, the LSTM layers step by step, the output Linear).  bf16: the LSTM and decoder
    weights and, at every use, the x / h operands of the products are rounded to bf16 as the HIP
    path rounds them (biases, the cell state, the gates and the sums stay in `dtype`).
    -> (logits (B, T, V), (h, c) each (L, B, H))."""
    rd = (lambda t: bf16_round(t.float()).to(dtype)) if bf16 else (lambda t: t.to(dtype))
    L = sum(1 for k in sd if k.startswith("rnn.weight_ih_l"))
    emb = sd["encoder.weight"].to(dtype)
    B, T = ids.shape
    H = sd["rnn.weight_hh_l0"].shape[1]
    if hidden is None:
        h = [torch.zeros(B, H, dtype=dtype) for _ in range(L)]
        c = [torch.zeros(B, H, dtype=dtype) for _ in range(L)]
    else:
        h = [hidden[0][k].to(dtype) for k in range(L)]
        c = [hidden[1][k].to(dtype) for k in range(L)]
    outs = []
    for t in range(T):
        x = emb[ids[:, t]]
        for k in range(L):
            w_ih, w_hh = rd(sd[f"rnn.weight_ih_l{k}"]), rd(sd[f"rnn.weight_hh_l{k}"])
            g = rd(x) @ w_ih.t() + rd(h[k]) @ w_hh.t() \
                + sd[f"rnn.bias_ih_l{k}"].to(dtype) + sd[f"rnn.bias_hh_l{k}"].to(dtype)
            gi, gf, gg, go = g.chunk(4, dim=1)
            c[k] = torch.sigmoid(gf) * c[k] + torch.sigmoid(gi) * torch.tanh(gg)
            h[k] = torch.sigmoid(go) * torch.tanh(c[k])
            x = h[k]
        outs.append(rd(x) @ rd(sd["decoder.weight"]).t() + sd["decoder.bias"].to(dtype))
    return torch.stack(outs, dim=1), (torch.stack(h), torch.stack(c))
