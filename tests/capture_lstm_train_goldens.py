"""Capture the LM-training fixtures from the REFERENCE implementation
(espnet2/lm/espnet_model.py ESPnetLanguageModel over espnet2/lm/seq_rnn_lm.py SequentialRNNLM,
dropout 0).  Test infrastructure: not collected by pytest, never imported by the package.

It reuses oracle/make_goldens.py (reference import path and stubs) and writes, readable by
tests/goldens.py and tests/lstm_train_goldens.py:

    lstm_train_tiny.npz  unit 26, 2 layers over the tiny_hybrid vocabulary, a ragged batch of 5
                         sentences, one of them with id 0 (ignore_id) inside; weights stored (w.*)
    lstm_train_nhid.npz  unit 24, nhid 40, 3 layers, ONE sentence (B = 1); weights stored
    lstm_train_650.npz   unit 650 x 2 layers, vocabulary 120, a ragged batch of 3; weights NOT
                         stored: regenerated from cfg.seed and checked against wsum.*; of every
                         gradient a strided sample of at most 4096 elements (gsamp.*, stride in
                         cfg.gstride) with its f64 sum and L2 norm (gsum.*, gnorm.*), since the
                         whole gradient (28 MB) cannot be a fixture

each with in.text / in.text_lengths, out.nll / out.loss / out.ntokens, the gradient of every
parameter after one backward (grad.* or the sample), and adam.losses: the losses of 5 steps of
torch.optim.Adam(lr 1e-3) with clip_grad_norm_(5.0) on that batch.

Yardsticks.  The same module is run in float64; err.<array> is max |f32 - f64| of the
reference itself for every recorded array, and the tests allow 4 x that (MARGIN, what
tests/capture_rnn_lm_goldens.py uses) or 4 ulps of f32 at the array's magnitude, whichever is
larger.  The tolerance scales with the reference's own error, so no sequence has to be
shortened for the reference to stay within a quarter of it: it always is.
bf16: bf.nll / bf.loss / bf.grad.* come from the training step restated in float64 with the
operands of every matrix product, forward AND backward, rounded to bf16 where the HIP path rounds
them (tests/lstm_train_goldens.py restate_bf16: the backward is written out, not autograd's, so
that dlogits, dgates and the saved activations are rounded as operands of the gradient products);
bf.err.* is the deviation of the same restatement run in f32, and the tests hold loss, nll and
every gradient element to tolerance(ref, bf.err) exactly as in f32.

Run:  PYTHONDONTWRITEBYTECODE=1 python -B tests/capture_lstm_train_goldens.py
"""
from __future__ import annotations

import copy
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, HERE]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import make_goldens as mg  # noqa: E402  (puts the reference and its stubs on sys.path)
from lstm_train_goldens import restate_bf16  # noqa: E402

MARGIN = 4
GSAMPLE = 4096
ADAM_STEPS, ADAM_LR, GRAD_CLIP = 5, 1e-3, 5.0


def _save(name, rec):
    path = os.path.join(mg.OUT, f"{name}.npz")
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    assert size < 2 ** 20, (name, size)
    return size


def _batch(V, lengths, gen, zero_inside=False):
    """Sentences of ids in [1, V - 1) (neither the pad id nor <sos/eos>), padded with 0."""
    B, L = len(lengths), max(lengths)
    text = torch.zeros(B, L, dtype=torch.int64)
    for i, n in enumerate(lengths):
        text[i, :n] = torch.randint(1, V - 1, (n,), generator=gen)
    if zero_inside:
        text[0, lengths[0] // 2] = 0  # ignore_id inside a sentence: scored, as the length mask says
    return text, torch.tensor(lengths, dtype=torch.int64)


def _one_pass(model, text, lens):
    model.zero_grad()
    loss, _, ntok = model(text, lens)
    loss.backward()
    with torch.no_grad():
        nll, _ = model.nll(text, lens)
    return loss.detach(), nll.detach(), ntok, {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def _adam(model, text, lens):
    model = copy.deepcopy(model)
    opt = torch.optim.Adam(model.parameters(), lr=ADAM_LR)
    losses = []
    for _ in range(ADAM_STEPS):
        opt.zero_grad()
        loss = model(text, lens)[0]
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), GRAD_CLIP)
        opt.step()
        losses.append(loss.detach().double())
    return torch.stack(losses)


def _restated(sd, text, lens, V, dtype):
    """loss / nll / gradients of the bf16-rounded restatement in `dtype` (forward and backward
    written out, tests/lstm_train_goldens.py restate_bf16)."""
    return restate_bf16(sd, text.clone(), lens, V, dtype)


def _err(a32, a64):
    return np.array(float((a32.double() - a64.double()).abs().max()))


def capture(name, lm_conf, lengths, seed, store_weights, zero_inside=False):
    from espnet2.lm.espnet_model import ESPnetLanguageModel
    from espnet2.lm.seq_rnn_lm import SequentialRNNLM
    V = lm_conf["vocab_size"]
    torch.manual_seed(seed)
    lm = SequentialRNNLM(**lm_conf)
    model = ESPnetLanguageModel(lm, V)
    model.train()
    model64 = copy.deepcopy(model).double()
    gen = torch.Generator().manual_seed(11)
    text, lens = _batch(V, lengths, gen, zero_inside)
    rec = {"in.text": text.numpy(), "in.text_lengths": lens.numpy()}
    if store_weights:
        rec.update({f"w.{k}": mg.np32(v) for k, v in lm.state_dict().items()})
    else:
        rec.update({f"wsum.{k}": np.array(v.double().sum().item()) for k, v in lm.state_dict().items()})
    loss, nll, ntok, g = _one_pass(model, text, lens)
    loss64, nll64, _, g64 = _one_pass(model64, text, lens)
    rec["out.loss"], rec["out.nll"], rec["out.ntokens"] = mg.np32(loss), mg.np32(nll), np.array(int(ntok))
    rec["err.loss"], rec["err.nll"] = _err(loss, loss64), _err(nll, nll64)
    bl64, bn64, bg64 = _restated(lm.state_dict(), text, lens, V, torch.float64)
    bl32, bn32, bg32 = _restated(lm.state_dict(), text, lens, V, torch.float32)
    rec["bf.loss"], rec["bf.nll"] = np.array(float(bl64)), bn64.numpy()
    rec["bf.err.loss"], rec["bf.err.nll"] = _err(bl32, bl64), _err(bn32, bn64)
    gstride = {}
    for k in g:
        short = k[3:]  # without the model's "lm." prefix
        rec[f"err.grad.{short}"] = _err(g[k], g64[k])
        rec[f"bf.err.grad.{short}"] = _err(bg32[short], bg64[short])
        if store_weights:
            rec[f"grad.{short}"] = mg.np32(g[k])
            rec[f"bf.grad.{short}"] = bg64[short].numpy()
        else:
            flat, flat_bf = g[k].reshape(-1), bg64[short].reshape(-1)
            s = max(1, -(-flat.numel() // GSAMPLE))
            gstride[short] = s
            rec[f"gsamp.{short}"] = mg.np32(flat[::s])
            rec[f"gsum.{short}"] = np.array(float(g64[k].sum()))
            rec[f"gnorm.{short}"] = np.array(float(g64[k].norm()))
            rec[f"bf.gsamp.{short}"] = flat_bf[::s].numpy()
            rec[f"bf.gnorm.{short}"] = np.array(float(bg64[short].norm()))
    a32, a64 = _adam(model, text, lens), _adam(model64, text, lens)
    rec["adam.losses"] = a64.numpy()
    rec["err.adam"] = _err(a32, a64)
    rec["cfg"] = np.array(json.dumps({"lm_conf": lm_conf, "seed": seed, "margin": MARGIN, "gstride": gstride,
                                      "adam": {"steps": ADAM_STEPS, "lr": ADAM_LR, "grad_clip": GRAD_CLIP}}))
    print(f"{name}: loss {float(loss):.6f} (f32-f64 {float(rec['err.loss']):.1e}), nll err "
          f"{float(rec['err.nll']):.1e}, adam err {float(rec['err.adam']):.1e}, bf16 loss "
          f"{float(bl64):.6f} (err {float(rec['bf.err.loss']):.1e}), {_save(name, rec)} bytes")


if __name__ == "__main__":
    z = np.load(os.path.join(mg.OUT, "tiny_hybrid.npz"))
    V = json.loads(str(z["cfg"]))["vocab_size"]
    capture("lstm_train_tiny", dict(vocab_size=V, unit=26, nhid=None, nlayers=2), [7, 4, 6, 1, 3], 3, True,
            zero_inside=True)
    capture("lstm_train_nhid", dict(vocab_size=V, unit=24, nhid=40, nlayers=3), [6], 5, True)
    capture("lstm_train_650", dict(vocab_size=120, unit=650, nlayers=2), [5, 3, 4], 0, False)
