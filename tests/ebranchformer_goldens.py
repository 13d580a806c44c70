"""Readers of the E-Branchformer fixtures (tests/capture_ebranchformer_goldens.py): a fixture is
a run of numbered parts <name>.0.npz, <name>.1.npz, ... in tests/goldens.py's key layout, each
small enough to commit; load() merges them in order (the w.* keys keep the state_dict order)."""
import os

import torch

from goldens import GOLDEN, load as load_one, section

FIXTURES = ("ebf_hybrid", "ebf_ctc_k31")
RECIPES = ("train_asr_e_branchformer_size256_mlp1024_linear1024_e12_mactrue_edrop0.0_ddrop0.0",
           "train_asr_ctc_e_branchformer_e12_mlp1024_linear1024")
_CACHE = {}


def load(name):
    if name not in _CACHE:
        cfg, d, i = None, {}, 0
        while os.path.exists(os.path.join(GOLDEN, f"{name}.{i}.npz")):
            c, part = load_one(f"{name}.{i}")
            cfg = cfg if c is None else c
            d.update(part)
            i += 1
        assert i > 0 and cfg is not None, name
        _CACHE[name] = (cfg, d)
    cfg, d = _CACHE[name]
    return dict(cfg), d


def build_loaded(name, **enc):
    """The fixture's model on the CPU with the fixture's weights (strict load); `enc` overrides
    encoder options (dropout rates)."""
    from test_model_build import build
    cfg, d = load(name)
    if enc:
        cfg["encoder_conf"] = dict(cfg["encoder_conf"], **enc)
    torch.manual_seed(0)
    m = build(cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in section(d, "w").items()}, strict=True)
    return cfg, d, m
