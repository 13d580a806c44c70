"""Capture the E-Branchformer fixtures from the REFERENCE implementation
(espnet2/asr/encoder/e_branchformer_encoder.py).  Test infrastructure: not collected by pytest,
never imported by the package.

oracle/make_goldens.build_reference_model knows the Conformer and the Transformer encoder only,
so the reference ESPnetASRModel is built here around the reference EBranchformerEncoder; the
reference import path and stubs, make_batch, perturb_norms, np32 and decoder_conf come from
oracle/make_goldens.py.  The key layout is tests/goldens.py's (cfg, w.*, in.*, out.*, stat.*,
g.*), plus out.next_rand (torch.rand(1) drawn right after the forward: repeat() builds a
MultiSequential, whose layer-drop uniform_ draw advances the host generator once per forward)
and out.num_params.  Everything runs with dropout 0.

A fixture is written as numbered parts <name>.0.npz, <name>.1.npz, ..., each below the
repository's 1 MiB limit for a committed file; tests/ebranchformer_goldens.py merges them.
ebf_recipes.npz holds the reference's parameter and state_dict key counts of the two
librispeech_100 E-Branchformer recipes (input_size 80, 5000 tokens), whose YAMLs (settings
only) are copied beside it.

Run:  PYTHONDONTWRITEBYTECODE=1 python -B tests/capture_ebranchformer_goldens.py
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

PART_BYTES = 900_000
RECIPES = ("train_asr_e_branchformer_size256_mlp1024_linear1024_e12_mactrue_edrop0.0_ddrop0.0.yaml",
           "train_asr_ctc_e_branchformer_e12_mlp1024_linear1024.yaml")
RECIPE_DIR = os.path.join(mg.REF, "egs2", "librispeech_100", "asr1", "conf", "tuning")


def ebf_conf(d, h, units, ck, mk, ff, nb, macaron):
    return dict(
        output_size=d, attention_heads=h, attention_layer_type="rel_selfattn", pos_enc_layer_type="rel_pos",
        rel_pos_type="latest", cgmlp_linear_units=units, cgmlp_conv_kernel=ck, use_linear_after_conv=False,
        gate_activation="identity", num_blocks=nb, dropout_rate=0.0, positional_dropout_rate=0.0,
        attention_dropout_rate=0.0, input_layer="conv2d", layer_drop_rate=0.0, linear_units=ff,
        positionwise_layer_type="linear", use_ffn=True, macaron_ffn=macaron, ffn_activation_type="swish",
        merge_conv_kernel=mk,
    )


CONFIGS = {
    # hybrid, macaron, ragged lengths (T' = 29); the two kernel sizes differ so that a swap shows
    "ebf_hybrid": dict(
        encoder="e_branchformer", input_size=80, vocab_size=50,
        encoder_conf=ebf_conf(64, 4, 128, 15, 7, 128, 3, True),
        decoder="transformer", decoder_conf=mg.decoder_conf(4, 128, 1),
        model_conf=dict(ctc_weight=0.3, lsm_weight=0.1, length_normalized_loss=False),
        speech_lengths=[120, 97, 64, 33], text_lengths=[12, 9, 7, 3],
    ),
    # CTC only, no macaron FFN, both kernels 31 over T' = 24 frames (every tap window runs off
    # both ends), 72 gate channels (not a multiple of the kernels' 64-channel tile)
    "ebf_ctc_k31": dict(
        encoder="e_branchformer", input_size=80, vocab_size=50,
        encoder_conf=ebf_conf(64, 4, 144, 31, 31, 128, 2, False),
        decoder="transformer", decoder_conf=mg.decoder_conf(4, 128, 1),
        model_conf=dict(ctc_weight=1.0, lsm_weight=0.1, length_normalized_loss=False),
        speech_lengths=[100, 100, 100], text_lengths=[10, 4, 8],
    ),
}


def build_reference_model(cfg):
    from espnet2.asr.ctc import CTC
    from espnet2.asr.decoder.transformer_decoder import TransformerDecoder
    from espnet2.asr.encoder.e_branchformer_encoder import EBranchformerEncoder
    from espnet2.asr.espnet_model import ESPnetASRModel
    from espnet2.layers.utterance_mvn import UtteranceMVN

    V = cfg["vocab_size"]
    encoder = EBranchformerEncoder(input_size=cfg["input_size"], **cfg["encoder_conf"])
    decoder = None
    if cfg.get("decoder"):
        decoder = TransformerDecoder(vocab_size=V, encoder_output_size=encoder.output_size(), **cfg["decoder_conf"])
    ctc = CTC(odim=V, encoder_output_size=encoder.output_size(), **cfg.get("ctc_conf", {}))
    return ESPnetASRModel(vocab_size=V, token_list=mg.token_list(V), frontend=None, specaug=None,
                          normalize=UtteranceMVN(), preencoder=None, encoder=encoder, postencoder=None,
                          decoder=decoder, ctc=ctc, joint_network=None, **cfg["model_conf"])


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
    model = build_reference_model(cfg)
    mg.perturb_norms(model, torch.Generator().manual_seed(1000 + seed))
    batch = mg.make_batch(cfg, torch.Generator().manual_seed(1))
    model.train()
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    enc_out = {}

    def enc_hook(mod, inp, out):
        enc_out["x"], enc_out["lens"] = out[0], out[1]

    hook = model.encoder.register_forward_hook(enc_hook)
    inputs = {k: v.clone() for k, v in batch.items()}
    torch.manual_seed(4242)  # the host generator the forward draws its layer-drop numbers from
    loss, stats, weight = model(**batch)
    next_rand = torch.rand(1)
    loss.backward()
    hook.remove()

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
    rec["out.encoder_out"] = mg.np32(enc_out["x"])
    rec["out.encoder_out_lens"] = enc_out["lens"].numpy()
    rec["out.next_rand"] = next_rand.numpy()
    rec["out.num_params"] = np.array(sum(p.numel() for p in model.parameters()))
    for k, p in model.named_parameters():
        if p.grad is not None:
            rec["g." + k] = mg.np32(p.grad)
    sizes = write_parts(name, rec)
    print(f"{name}: loss={loss.item():.6f} "
          f"stats={ {k: round(float(v), 4) for k, v in stats.items() if v is not None} } parts={sizes}")


def capture_recipes():
    """The two recipe YAMLs (settings only) and the reference model's parameter and state_dict
    key counts for each: input_size 80 (no frontend), a 5000-token list."""
    import yaml
    rec = {}
    for fn in RECIPES:
        src = os.path.join(RECIPE_DIR, fn)
        shutil.copyfile(src, os.path.join(mg.OUT, fn))
        with open(src) as f:
            y = yaml.safe_load(f)
        assert y["encoder"] == "e_branchformer"
        cfg = dict(input_size=80, vocab_size=5000, encoder_conf=y["encoder_conf"],
                   decoder=y.get("decoder"), decoder_conf=y.get("decoder_conf", {}), model_conf=y["model_conf"])
        if y["model_conf"].get("ctc_weight") == 1.0:
            cfg["decoder"] = None  # as ASRTask: the CTC-only recipe names no decoder
        torch.manual_seed(0)
        model = build_reference_model(cfg)
        key = fn[:-len(".yaml")]
        rec["nparams." + key] = np.array(sum(p.numel() for p in model.parameters()))
        rec["nkeys." + key] = np.array(len(model.state_dict()))
        print(fn, int(rec["nparams." + key]), int(rec["nkeys." + key]))
    np.savez_compressed(os.path.join(mg.OUT, "ebf_recipes.npz"), **rec)


if __name__ == "__main__":
    for name, cfg in CONFIGS.items():
        capture(name, cfg)
    capture_recipes()
