"""Capture the intermediate-CTC / self-conditioned-CTC fixtures from the REFERENCE
implementation.  Test infrastructure: not collected by pytest, never imported by the package.

It reuses oracle/make_goldens.py (reference import path and stubs, model builder, batch and
norm perturbation) and writes the same key layout (cfg, w.*, in.*, out.*, stat.*, mid.*, g.*,
buf_after.*), plus

    mid.interctc{l}   the tap's normalised output y_l (conformer_encoder.py:354-357)
    out.next_rand     torch.rand(1) drawn right after the forward: the encoder with taps loops
                      over its layers itself, so MultiSequential's layer-drop uniform_ draw
                      (repeat.py:27) does not happen, and the host generator shows it

A fixture is written as numbered parts, <name>.0.npz, <name>.1.npz, ..., each below the
repository's 1 MiB limit for a committed file and each readable by tests/goldens.py;
tests/interctc_goldens.py merges them back in order.  interctc_recipes.npz holds the
reference's parameter counts of the two librispeech_100 recipe configurations
(train_conformer_interctc.yaml, train_conformer_scctc.yaml, copied beside it).

Run:  PYTHONDONTWRITEBYTECODE=1 python -B tests/capture_interctc_goldens.py
"""
from __future__ import annotations

import io
import json
import os
import shutil
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import make_goldens as mg  # noqa: E402  (puts the reference and its stubs on sys.path)

PART_BYTES = 900_000  # compressed size bound of one part (float data barely compresses)
RECIPES = ("train_conformer_interctc.yaml", "train_conformer_scctc.yaml")
RECIPE_DIR = os.path.join(mg.REF, "egs2", "librispeech_100", "asr1", "conf", "tuning")


def _enc(nb, taps, cond):
    return dict(mg.conformer_conf(64, 4, 128, nb, k=15), interctc_layer_idx=taps, interctc_use_conditioning=cond)


CONFIGS = {
    # self-conditioned, hybrid: two taps, ragged lengths (padded rows in every tap)
    "interctc_sc_hybrid": dict(
        encoder="conformer", input_size=80, vocab_size=50, encoder_conf=_enc(4, [1, 3], True),
        decoder="transformer", decoder_conf=mg.decoder_conf(4, 128, 1),
        model_conf=dict(ctc_weight=0.3, interctc_weight=0.5, lsm_weight=0.1, length_normalized_loss=False),
        speech_lengths=[120, 97, 64, 33], text_lengths=[12, 9, 7, 3],
    ),
    # self-conditioned, CTC only (the scctc recipe's weights; decoder dropped), equal lengths:
    # no padded row at all
    "interctc_sc_ctc": dict(
        encoder="conformer", input_size=80, vocab_size=50, encoder_conf=_enc(3, [2], True),
        decoder="transformer", decoder_conf=mg.decoder_conf(4, 128, 1),
        model_conf=dict(ctc_weight=1.0, interctc_weight=0.66, lsm_weight=0.1, length_normalized_loss=False),
        speech_lengths=[100, 100, 100], text_lengths=[10, 4, 8],
    ),
    # plain intermediate CTC (no conditioning), hybrid
    "interctc_plain": dict(
        encoder="conformer", input_size=80, vocab_size=50, encoder_conf=_enc(4, [1, 3], False),
        decoder="transformer", decoder_conf=mg.decoder_conf(4, 128, 1),
        model_conf=dict(ctc_weight=0.3, interctc_weight=0.5, lsm_weight=0.1, length_normalized_loss=False),
        speech_lengths=[120, 97, 64, 33], text_lengths=[12, 9, 7, 3],
    ),
}


def _npz_bytes(rec):
    buf = io.BytesIO()
    np.savez_compressed(buf, **rec)
    return buf.getvalue()


def write_parts(name, rec):
    """rec (ordered) -> <name>.<i>.npz, keys in order, each part below PART_BYTES."""
    for f in os.listdir(mg.OUT):
        if f.startswith(name + ".") and f.endswith(".npz"):
            os.remove(os.path.join(mg.OUT, f))
    parts, cur = [], {}
    for k, v in rec.items():
        trial = dict(cur)
        trial[k] = v
        if cur and len(_npz_bytes(trial)) > PART_BYTES:
            parts.append(cur)
            cur = {k: v}
        else:
            cur = trial
    parts.append(cur)
    sizes = []
    for i, part in enumerate(parts):
        data = _npz_bytes(part)
        assert len(data) < 2 ** 20, (name, i, len(data))
        with open(os.path.join(mg.OUT, f"{name}.{i}.npz"), "wb") as f:
            f.write(data)
        sizes.append(len(data))
    return sizes


def capture(name, cfg, seed=0):
    torch.manual_seed(seed)
    model = mg.build_reference_model(cfg)
    mg.perturb_norms(model, torch.Generator().manual_seed(1000 + seed))
    batch = mg.make_batch(cfg, torch.Generator().manual_seed(1))
    model.train()
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    enc_out = {}

    def enc_hook(mod, inp, out):
        enc_out["x"], enc_out["lens"] = out[0], out[1]

    hook = model.encoder.register_forward_hook(enc_hook)
    inputs = {k: v.clone() for k, v in batch.items()}
    torch.manual_seed(4242)  # the host generator the forward would draw its layer-drop numbers from
    loss, stats, weight = model(**batch)
    next_rand = torch.rand(1)
    loss.backward()
    hook.remove()
    (x, inter), lens = enc_out["x"], enc_out["lens"]

    rec = {"cfg": np.array(json.dumps(cfg))}
    for k, v in sd0.items():
        rec["w." + k] = mg.np32(v)
    for k, v in inputs.items():
        rec["in." + k] = v.numpy()
    rec["out.loss"] = mg.np32(loss)
    for k, v in stats.items():
        if v is not None:
            rec["stat." + k] = mg.np32(v)
    rec["out.weight"] = weight.numpy()
    rec["out.encoder_out"] = mg.np32(x)
    rec["out.encoder_out_lens"] = lens.numpy()
    rec["out.next_rand"] = next_rand.numpy()
    rec["out.num_params"] = np.array(sum(p.numel() for p in model.parameters()))
    for layer_idx, y in inter:
        rec[f"mid.interctc{layer_idx}"] = mg.np32(y)
    for k, p in model.named_parameters():
        if p.grad is not None:
            rec["g." + k] = mg.np32(p.grad)
    for k, v in model.state_dict().items():
        if "running" in k or "num_batches" in k:
            rec["buf_after." + k] = mg.np32(v)
    sizes = write_parts(name, rec)
    print(f"{name}: loss={loss.item():.6f} "
          f"stats={ {k: round(float(v), 4) for k, v in stats.items() if v is not None} } parts={sizes}")


def capture_recipes():
    """The two recipe YAMLs (settings only) and the reference model's parameter count for each:
    input_size 80 (no frontend), a 5000-token list, the decoder dropped (ctc_weight 1.0)."""
    import yaml
    rec = {}
    for fn in RECIPES:
        src = os.path.join(RECIPE_DIR, fn)
        shutil.copyfile(src, os.path.join(mg.OUT, fn))
        with open(src) as f:
            y = yaml.safe_load(f)
        assert y["encoder"] == "conformer" and y["model_conf"]["ctc_weight"] == 1.0
        cfg = dict(encoder="conformer", input_size=80, vocab_size=5000, encoder_conf=y["encoder_conf"],
                   model_conf=y["model_conf"])
        torch.manual_seed(0)
        model = mg.build_reference_model(cfg)
        rec["nparams." + fn[:-len(".yaml")]] = np.array(sum(p.numel() for p in model.parameters()))
        rec["nkeys." + fn[:-len(".yaml")]] = np.array(len(model.state_dict()))
        print(fn, int(rec["nparams." + fn[:-len(".yaml")]]))
    np.savez_compressed(os.path.join(mg.OUT, "interctc_recipes.npz"), **rec)


if __name__ == "__main__":
    for name, cfg in CONFIGS.items():
        capture(name, cfg)
    capture_recipes()
