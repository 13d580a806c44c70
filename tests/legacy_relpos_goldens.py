"""Readers of the legacy rel-pos fixtures (tests/capture_legacy_relpos_goldens.py) and the
legacy rel_shift restated as an index law, shared by the capture script (which checks it
bit-for-bit against the reference before storing anything) and the tests.

A model fixture is a run of numbered parts <name>.0.npz, <name>.1.npz, ... in tests/goldens.py's
key layout, each small enough to commit; load() merges them in order."""
import os

import torch

from goldens import GOLDEN, load as load_one, section

FIXTURES = ("legacy_tiny", "legacy_dk64")
RECIPE = "train_asr_conformer7_n_fft512_hop_length256"
SHIFT_T = (1, 2, 3, 5, 8, 17)
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


# ------------------------------------------------------------------------------ the index law
def legacy_shift(bdq):
    """LegacyRelPositionMultiHeadedAttention.rel_shift of a (..., T, T) matrix BDq[r, k]:
        out[i, j] = BDq[i,   T-1-i+j]   j <= i
        out[i, j] = 0                   j == i+1
        out[i, j] = BDq[i+1, j-i-2]     j >= i+2"""
    T = bdq.shape[-1]
    i = torch.arange(T).view(T, 1).expand(T, T)
    j = torch.arange(T).view(1, T).expand(T, T)
    low = j <= i
    up = j >= i + 2
    row = torch.where(low, i, (i + 1).clamp(max=T - 1))
    col = torch.where(low, T - 1 - i + j, (j - i - 2).clamp(min=0))
    out = bdq[..., row, col]
    return torch.where(low | up, out, torch.zeros((), dtype=bdq.dtype))


def pext(p):
    """The extended table of 2T-1 rows from p (T, d): p, one zero row, p[:T-2]."""
    T = p.shape[0]
    if T == 1:
        return p.clone()
    return torch.cat([p, torch.zeros_like(p[:1]), p[:T - 2]], 0)


def pext_fold(dpx):
    """Adjoint of pext: (2T-1, d) -> (T, d), dp[k] = dPext[k] + dPext[T+1+k] for k <= T-3."""
    T = (dpx.shape[0] + 1) // 2
    dp = dpx[:T].clone()
    if T >= 3:
        dp[:T - 2] += dpx[T + 1:]
    return dp


def legacy_band(qv, px):
    """The shifted term through the band form the kernels use: BD[r, k] = (q_r + v)·Pext[k] over
    2T-1 columns, out[i, j] = BD[i + (j > i), T-1-i+j].  qv (..., T, dk), px (2T-1, dk)."""
    T = qv.shape[-2]
    bd = qv @ px.transpose(-1, -2)
    i = torch.arange(T).view(T, 1).expand(T, T)
    j = torch.arange(T).view(1, T).expand(T, T)
    row = (i + (j > i).long()).clamp(max=T - 1)
    return bd[..., row, T - 1 - i + j]
