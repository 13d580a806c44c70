"""Capture the SequentialRNNLM fixtures from the REFERENCE implementation
(espnet2/lm/seq_rnn_lm.py).  Test infrastructure: not collected by pytest, never imported by
the package.

It reuses oracle/make_goldens.py (reference import path and stubs, the tiny hybrid model) and
writes, readable by tests/goldens.py and tests/rnn_lm_goldens.py:

    rnn_lm_tiny.npz   unit 26, 2 layers over the tiny_hybrid vocabulary: weights (w.*), forward
                      logits and final (h, c) of in.ids, a chain of 5 batch_score steps on 4
                      prefixes (chain.{k}.logp/h/c), the reference BeamSearch n-best with LM
                      fusion (c{case}.u{utt}.h{rank}.*) and the BatchBeamSearch n-best (b{case}...)
    rnn_lm_nhid.npz   unit 24, nhid 40, 3 layers: weights, logits, a 2-step batch_score chain
    rnn_lm_650.npz    unit 650 x 2 layers, vocabulary 120   } weights NOT stored: regenerated from
    rnn_lm_2048.npz   unit 2048 x 1 layer, vocabulary 64    } cfg.seed, checked against wsum.*
                      logits of in.ids and one batch_score at n = 17 from the states in.bs_h/c
    rnn_lm_recipes.npz  parameter and state_dict key counts of the lm_conf of three recipes, whose
                      YAMLs (settings only) are copied beside it as rnn_lm_<recipe>_<file>.yaml

The tiny seed is advanced until every two adjacent n-best scores of every search differ by at
least 1e-2, ten times the tests' score tolerance, so a rounding-level difference cannot reorder
the reference's own list.  The sized captures check on the CPU that the reference's f32 result
is within 2.5e-5 (a quarter of the tests' tolerance) of the same module run in float64, and
shorten the sequence until it is.

Run:  PYTHONDONTWRITEBYTECODE=1 python -B tests/capture_rnn_lm_goldens.py
"""
from __future__ import annotations

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

RECIPES = {"librispeech_train_lm_adam": ("librispeech", "tuning/train_lm_adam.yaml"),
           "aishell_train_lm": ("aishell", "train_lm.yaml"),
           "laborotv_train_lm": ("laborotv", "train_lm.yaml")}
RECIPE_VOCAB = 5000
MIN_GAP = 1e-2  # between adjacent n-best scores
F64_TOL = 2.5e-5
CASES = [(3, 0.0, 0.0, 0.3, 0.3), (4, 0.5, 0.0, 0.5, 0.5)]  # capture_lm's: beam, lb, maxlenratio, ctc w, lm w


def _save(name, rec):
    path = os.path.join(mg.OUT, f"{name}.npz")
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    assert size < 2 ** 20, (name, size)
    return size


def _chain(lm, ys, steps):
    """steps batch_score calls on growing prefixes ys[:, :k + 1], each fed the previous states."""
    rec, states = {}, [None] * ys.shape[0]
    for k in range(steps):
        logp, states = lm.batch_score(ys[:, :k + 1], states, None)
        rec[f"chain.{k}.logp"] = mg.np32(logp)
        rec[f"chain.{k}.h"] = mg.np32(torch.stack([h for h, _ in states], dim=1))
        rec[f"chain.{k}.c"] = mg.np32(torch.stack([c for _, c in states], dim=1))
    return rec


def _small(lm_conf, seed, V, sos, steps):
    from espnet2.lm.seq_rnn_lm import SequentialRNNLM
    torch.manual_seed(seed)
    lm = SequentialRNNLM(**lm_conf)
    lm.eval()
    gen = torch.Generator().manual_seed(4)
    rec = {f"w.{k}": mg.np32(v) for k, v in lm.state_dict().items()}
    ids = torch.randint(2, V - 1, (3, 7), generator=gen)
    ys = torch.cat([torch.full((4, 1), sos), torch.randint(2, V - 1, (4, steps - 1), generator=gen)], dim=1)
    with torch.no_grad():
        logits, (h, c) = lm(ids, None)
        rec.update(_chain(lm, ys, steps))
    rec["in.ids"] = ids.numpy().astype(np.int64)
    rec["in.ys"] = ys.numpy().astype(np.int64)
    rec["out.logits"], rec["out.h"], rec["out.c"] = mg.np32(logits), mg.np32(h), mg.np32(c)
    return lm, rec


def _searches(model, lm, z, cls, tag):
    from espnet.nets.scorers.ctc import CTCPrefixScorer
    from espnet.nets.scorers.length_bonus import LengthBonus
    speech, lens = torch.from_numpy(z["in.speech"]), torch.from_numpy(z["in.speech_lengths"])
    V = model.vocab_size
    out, meta, gap = {}, [], float("inf")
    with torch.no_grad():
        for ci, (beam, lb, mlr, cw, lw) in enumerate(CASES):
            bs = cls(scorers={"decoder": model.decoder, "ctc": CTCPrefixScorer(model.ctc, model.eos), "lm": lm,
                              "length_bonus": LengthBonus(V)},
                     weights={"decoder": 1.0 - cw, "ctc": cw, "lm": lw, "length_bonus": lb}, beam_size=beam,
                     vocab_size=V, sos=model.sos, eos=model.eos, token_list=None, pre_beam_score_key="full")
            for u in range(speech.shape[0]):
                le = int(lens[u])
                enc, _ = model.encode(speech[u:u + 1, :le], lens[u:u + 1])
                nbest = bs(x=enc[0], maxlenratio=mlr, minlenratio=0.0)
                sc = [float(h.score) for h in nbest]
                gap = min([gap] + [a - b for a, b in zip(sc, sc[1:])])
                for r, h in enumerate(nbest):
                    key = f"{tag}{ci}.u{u}.h{r}"
                    out[key + ".yseq"] = h.yseq.numpy().astype(np.int64)
                    out[key + ".score"] = np.float64(float(h.score))
                    out[key + ".lm"] = np.float64(float(h.scores["lm"]))
                meta.append({"case": ci, "utt": u, "n": len(nbest)})
    return out, meta, gap


def capture_tiny(name="rnn_lm_tiny", cfg_name="tiny_hybrid"):
    from espnet.nets.batch_beam_search import BatchBeamSearch
    from espnet.nets.beam_search import BeamSearch
    z = np.load(os.path.join(mg.OUT, cfg_name + ".npz"))
    cfg = json.loads(str(z["cfg"]))
    model = mg.build_reference_model(cfg)
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")})
    model.eval()
    V = model.vocab_size
    lm_conf = dict(vocab_size=V, unit=26, nhid=None, nlayers=2)
    for seed in range(3, 64):
        lm, rec = _small(lm_conf, seed, V, model.sos, steps=5)
        o1, m1, g1 = _searches(model, lm, z, BeamSearch, "c")
        o2, m2, g2 = _searches(model, lm, z, BatchBeamSearch, "b")
        if min(g1, g2) >= MIN_GAP:
            break
        print(f"{name}: seed {seed} rejected (adjacent n-best scores {min(g1, g2):.2e} apart)")
    else:
        raise RuntimeError("no seed separates the n-best scores")
    rec.update(o1)
    rec.update(o2)
    rec["cfg"] = np.array(json.dumps({"lm_conf": lm_conf, "seed": seed, "cases": CASES, "nbest": m1,
                                      "nbest_batch": m2, "model": cfg_name, "min_gap": min(g1, g2)}))
    print(f"{name}: seed {seed}, min n-best gap {min(g1, g2):.3f}, {_save(name, rec)} bytes")


def capture_nhid(name="rnn_lm_nhid", cfg_name="tiny_hybrid"):
    z = np.load(os.path.join(mg.OUT, cfg_name + ".npz"))
    V = json.loads(str(z["cfg"]))["vocab_size"]
    lm_conf = dict(vocab_size=V, unit=24, nhid=40, nlayers=3)
    _, rec = _small(lm_conf, 5, V, V - 1, steps=2)
    rec["cfg"] = np.array(json.dumps({"lm_conf": lm_conf, "seed": 5}))
    print(f"{name}: {_save(name, rec)} bytes")


def _close64(a32, a64):
    return bool((a32.double() - a64).abs().le(F64_TOL + F64_TOL * a64.abs()).all())


def capture_sized(name, lm_conf, seed=0, n=17):
    """Weights from torch.manual_seed(seed) (the build's class constructs the same modules in the
    same order, so it initialises bit-identically); only per-tensor f64 sums are stored."""
    import copy
    from espnet2.lm.seq_rnn_lm import SequentialRNNLM
    V = lm_conf["vocab_size"]
    torch.manual_seed(seed)
    lm = SequentialRNNLM(**lm_conf)
    lm.eval()
    lm64 = copy.deepcopy(lm).double()
    gen = torch.Generator().manual_seed(4)
    rec = {f"wsum.{k}": np.array(v.double().sum().item()) for k, v in lm.state_dict().items()}
    T = 6
    ids = torch.randint(1, V, (2, T), generator=gen)
    pre = torch.randint(1, V, (n, 4), generator=gen)
    with torch.no_grad():
        while True:
            logits, (h, c) = lm(ids[:, :T], None)
            l64, (h64, c64) = lm64(ids[:, :T], None)
            if _close64(logits, l64) and _close64(h, h64) and _close64(c, c64):
                break
            T -= 1
            assert T >= 1, "f32 reference is not within F64_TOL of float64 even for one token"
        _, (bh, bc) = lm(pre[:, :3], None)
        st = [(bh[:, i], bc[:, i]) for i in range(n)]
        logp, st2 = lm.batch_score(pre, st, None)
        lp64, st64 = lm64.batch_score(pre, [(a.double(), b.double()) for a, b in st], None)
        h2, c2 = torch.stack([a for a, _ in st2], 1), torch.stack([b for _, b in st2], 1)
        assert _close64(logp, lp64) and _close64(h2, torch.stack([a for a, _ in st64], 1)) \
            and _close64(c2, torch.stack([b for _, b in st64], 1)), "batch_score f32 vs float64"
    rec["in.ids"] = ids[:, :T].numpy().astype(np.int64)
    rec["in.ys"] = pre.numpy().astype(np.int64)
    rec["in.bs_h"], rec["in.bs_c"] = mg.np32(bh), mg.np32(bc)
    rec["out.logits"], rec["out.h"], rec["out.c"] = mg.np32(logits), mg.np32(h), mg.np32(c)
    rec["out.bs_logp"], rec["out.bs_h"], rec["out.bs_c"] = mg.np32(logp), mg.np32(h2), mg.np32(c2)
    rec["cfg"] = np.array(json.dumps({"lm_conf": lm_conf, "seed": seed}))
    print(f"{name}: T={T}, max |f32 - f64| logits {float((logits.double() - l64).abs().max()):.2e}, "
          f"{_save(name, rec)} bytes")


def capture_recipes(name="rnn_lm_recipes"):
    """The three recipe YAMLs (settings only) and, for each lm_conf, the reference model's
    parameter and state_dict key counts on the meta device (nothing large is allocated)."""
    import yaml
    from espnet2.lm.seq_rnn_lm import SequentialRNNLM
    rec = {}
    for key, (corpus, fn) in RECIPES.items():
        src = os.path.join(mg.REF, "egs2", corpus, "asr1", "conf", fn)
        shutil.copyfile(src, os.path.join(mg.OUT, f"rnn_lm_{key}.yaml"))
        os.chmod(os.path.join(mg.OUT, f"rnn_lm_{key}.yaml"), 0o644)
        with open(src) as f:
            y = yaml.safe_load(f)
        assert y.get("lm", "seq_rnn") == "seq_rnn"
        with torch.device("meta"):
            lm = SequentialRNNLM(vocab_size=RECIPE_VOCAB, **y["lm_conf"])
        rec["nparams." + key] = np.array(sum(p.numel() for p in lm.parameters()))
        rec["nkeys." + key] = np.array(len(lm.state_dict()))
        print(key, int(rec["nparams." + key]), int(rec["nkeys." + key]))
    rec["cfg"] = np.array(json.dumps({"vocab_size": RECIPE_VOCAB, "recipes": list(RECIPES)}))
    _save(name, rec)


if __name__ == "__main__":
    capture_tiny()
    capture_nhid()
    capture_sized("rnn_lm_650", dict(vocab_size=120, unit=650, nlayers=2))
    capture_sized("rnn_lm_2048", dict(vocab_size=64, unit=2048, nlayers=1))
    capture_recipes()
