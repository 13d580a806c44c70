"""Capture the legacy rel-pos fixtures (rel_pos_type: legacy, the Conformer's default) from
the REFERENCE implementation.  Test infrastructure: not collected by pytest, never imported
by the package.

oracle/make_goldens.build_reference_model builds a legacy Conformer from any encoder_conf that
leaves rel_pos_type out; make_batch, perturb_norms and np32 come from there too.  The model
fixtures keep tests/goldens.py's key layout (cfg, w.*, in.*, out.*, stat.*, g.*) and are
written as numbered parts <name>.0.npz, <name>.1.npz, ..., each below the repository's 1 MiB
limit for a committed file; tests/legacy_relpos_goldens.py merges them.  Everything runs with
dropout 0.

  legacy_shift.npz    random (B, H, T, T) f64 matrices and the reference's legacy rel_shift of
                      them for T in {1, 2, 3, 5, 8, 17} (the index law of
                      tests/legacy_relpos_goldens.py is checked bit-for-bit against it here,
                      before anything is stored), and the reference's pos_emb for
                      (max_len 16, T 10) and (max_len 16, T 20 then T 10)
  legacy_tiny         hybrid, d 64, 4 heads (head dim 16), 2 blocks, ragged lengths
  legacy_dk64         hybrid, d 128, 2 heads (head dim 64), 2 blocks, T' = 66 and 49; also the
                      encoder output of an eval-mode forward
  legacy_recipes.npz  parameter and state_dict key counts of
                      train_asr_conformer7_n_fft512_hop_length256.yaml (input size 80, 5000
                      tokens); the YAML (settings only) is copied beside it

Run:  PYTHONDONTWRITEBYTECODE=1 python -B tests/capture_legacy_relpos_goldens.py
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
sys.path[:0] = [REPO, HERE]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import make_goldens as mg  # noqa: E402  (puts the reference and its stubs on sys.path)
import legacy_relpos_goldens as lg  # noqa: E402

PART_BYTES = 900_000
RECIPE_DIR = os.path.join(mg.REF, "egs2", "librispeech", "asr1", "conf", "tuning")


def legacy_conf(d, h, ff, nb, k):
    c = mg.conformer_conf(d, h, ff, nb, k=k)
    del c["rel_pos_type"]  # the reference's default: legacy
    return c


CONFIGS = {
    "legacy_tiny": dict(
        encoder="conformer", input_size=80, vocab_size=50,
        encoder_conf=legacy_conf(64, 4, 128, 2, 15),
        decoder="transformer", decoder_conf=mg.decoder_conf(4, 128, 1),
        model_conf=dict(ctc_weight=0.3, lsm_weight=0.1, length_normalized_loss=False),
        speech_lengths=[120, 97, 64, 33], text_lengths=[12, 9, 7, 3],
    ),
    # T' = 66 (two 64-query tiles) and 49 (less than one).  input_size 48 keeps embed.out.0.weight
    # (d, d*F'') below the 1 MiB file limit, and at this size and these lengths the reference's own
    # fp32 gradients are within 0.26x of the fp32 parity tolerance of tests/test_model_gpu.py from
    # its float64 gradients (at input_size 20 and lengths 280/200 the subsampling layers' were
    # 2.1x away: the fixture would have been its own rounding noise)
    "legacy_dk64": dict(
        encoder="conformer", input_size=48, vocab_size=50,
        encoder_conf=legacy_conf(128, 2, 128, 2, 15),
        decoder="transformer", decoder_conf=mg.decoder_conf(2, 128, 1),
        model_conf=dict(ctc_weight=0.3, lsm_weight=0.1, length_normalized_loss=False),
        speech_lengths=[270, 200], text_lengths=[20, 14],
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


def capture(name, cfg, seed=0, eval_out=False):
    from espnet.nets.pytorch_backend.transformer.attention import LegacyRelPositionMultiHeadedAttention
    from espnet.nets.pytorch_backend.transformer.embedding import LegacyRelPositionalEncoding
    torch.manual_seed(seed)
    model = mg.build_reference_model(cfg)
    assert isinstance(model.encoder.embed.out[1], LegacyRelPositionalEncoding)
    assert isinstance(model.encoder.encoders[0].self_attn, LegacyRelPositionMultiHeadedAttention)
    mg.perturb_norms(model, torch.Generator().manual_seed(1000 + seed))
    batch = mg.make_batch(cfg, torch.Generator().manual_seed(1))
    model.train()
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    enc_out = {}

    def enc_hook(mod, inp, out):
        enc_out["x"], enc_out["lens"] = out[0], out[1]

    hook = model.encoder.register_forward_hook(enc_hook)
    inputs = {k: v.clone() for k, v in batch.items()}
    loss, stats, weight = model(**batch)
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
    with torch.no_grad():
        rec["out.ctc_argmax"] = model.ctc.argmax(enc_out["x"]).numpy()
        rec["out.ctc_logits"] = mg.np32(model.ctc.ctc_lo(enc_out["x"]))
    rec["out.num_params"] = np.array(sum(p.numel() for p in model.parameters()))
    for k, p in model.named_parameters():
        if p.grad is not None:
            rec["g." + k] = mg.np32(p.grad)
    for k, v in model.state_dict().items():
        if "running" in k or "num_batches" in k:
            rec["buf_after." + k] = mg.np32(v)
    if eval_out:
        # eval-mode encode() from the INITIAL state (the BatchNorm running statistics of sd0)
        model.load_state_dict(sd0)
        model.eval()
        with torch.no_grad():
            ev, evl = model.encode(inputs["speech"].clone(), inputs["speech_lengths"].clone())
        rec["out.encoder_out_eval"] = mg.np32(ev)
        rec["out.encoder_out_eval_lens"] = evl.numpy()
    sizes = write_parts(name, rec)
    print(f"{name}: loss={loss.item():.6f} "
          f"stats={ {k: round(float(v), 4) for k, v in stats.items() if v is not None} } parts={sizes}")


def capture_shift():
    from espnet.nets.pytorch_backend.transformer.attention import LegacyRelPositionMultiHeadedAttention
    from espnet.nets.pytorch_backend.transformer.embedding import LegacyRelPositionalEncoding
    att = LegacyRelPositionMultiHeadedAttention(2, 8, 0.0)
    g = torch.Generator().manual_seed(5)
    rec = {}
    for T in lg.SHIFT_T:
        x = torch.randn(2, 3, T, T, generator=g, dtype=torch.float64)
        y = att.rel_shift(x)
        assert torch.equal(lg.legacy_shift(x), y), T  # the index law, bit for bit
        # ... and the band form the kernels use, with exactly representable small integers
        q = torch.randint(-4, 5, (2, 3, T, 4), generator=g).double()
        p = torch.randint(-4, 5, (T, 4), generator=g).double()
        assert torch.equal(lg.legacy_band(q, lg.pext(p)), att.rel_shift(q @ p.t())), T
        rec[f"x.{T}"] = x.numpy()
        rec[f"y.{T}"] = y.numpy()
    d = 8
    pe = LegacyRelPositionalEncoding(d, 0.0, max_len=16)
    pe.eval()
    rec["pos.16.10"] = pe(torch.zeros(1, 10, d))[1][0].numpy()
    pe = LegacyRelPositionalEncoding(d, 0.0, max_len=16)
    pe.eval()
    rec["pos.16.20"] = pe(torch.zeros(1, 20, d))[1][0].numpy()
    rec["pos.16.20.10"] = pe(torch.zeros(1, 10, d))[1][0].numpy()
    rec["cfg"] = np.array(json.dumps(dict(T=list(lg.SHIFT_T), d_model=d, max_len=16)))
    np.savez_compressed(os.path.join(mg.OUT, "legacy_shift.npz"), **rec)
    print("legacy_shift: index law and band form equal the reference's rel_shift for T in", lg.SHIFT_T)


def capture_recipe():
    import yaml
    fn = lg.RECIPE + ".yaml"
    src = os.path.join(RECIPE_DIR, fn)
    shutil.copyfile(src, os.path.join(mg.OUT, fn))
    with open(src) as f:
        y = yaml.safe_load(f)
    assert y["encoder"] == "conformer" and "rel_pos_type" not in y["encoder_conf"]
    cfg = dict(encoder="conformer", input_size=80, vocab_size=5000, encoder_conf=y["encoder_conf"],
               decoder=y["decoder"], decoder_conf=y["decoder_conf"], model_conf=y["model_conf"])
    torch.manual_seed(0)
    model = mg.build_reference_model(cfg)
    rec = {"nparams." + lg.RECIPE: np.array(sum(p.numel() for p in model.parameters())),
           "nkeys." + lg.RECIPE: np.array(len(model.state_dict()))}
    print(fn, int(rec["nparams." + lg.RECIPE]), int(rec["nkeys." + lg.RECIPE]))
    np.savez_compressed(os.path.join(mg.OUT, "legacy_recipes.npz"), **rec)


if __name__ == "__main__":
    capture_shift()
    capture("legacy_tiny", CONFIGS["legacy_tiny"])
    capture("legacy_dk64", CONFIGS["legacy_dk64"], eval_out=True)
    capture_recipe()
