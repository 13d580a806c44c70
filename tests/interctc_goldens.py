"""Readers of the intermediate-CTC fixtures (tests/capture_interctc_goldens.py): a fixture is a
run of numbered parts <name>.0.npz, <name>.1.npz, ... in tests/goldens.py's key layout, each
small enough to commit; load() merges them in order (the w.* keys keep the state_dict order)."""
import os

import torch

from goldens import GOLDEN, load as load_one, section

FIXTURES = ("interctc_sc_hybrid", "interctc_sc_ctc", "interctc_plain")


def load(name):
    cfg, d, i = None, {}, 0
    while os.path.exists(os.path.join(GOLDEN, f"{name}.{i}.npz")):
        c, part = load_one(f"{name}.{i}")
        cfg = cfg if c is None else c
        d.update(part)
        i += 1
    assert i > 0 and cfg is not None, name
    return cfg, d


def build_loaded(name):
    """The fixture's model on the CPU with the fixture's weights (strict load)."""
    from test_model_build import build
    cfg, d = load(name)
    torch.manual_seed(0)
    m = build(cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in section(d, "w").items()}, strict=True)
    return cfg, d, m
