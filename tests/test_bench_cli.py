"""bench.py's command line: a plain run times the steps and prints the result line only;
--full adds the roofline, the DP rehearsal and the CPU baseline; --dump-outputs DIR writes
the last timed step's outputs as float arrays."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("roofline", "dp_rehearsal", "cpu_baseline", "speedup_vs_cpu")


def _step_out():
    g = torch.Generator().manual_seed(3)
    stats = dict(loss=torch.randn(1, generator=g), loss_ctc=torch.randn(1, generator=g),
                 acc=torch.rand(1, generator=g).to(torch.bfloat16), cer=None, wer=None)
    return (stats["loss"].clone(), stats, torch.tensor(32), torch.rand((), generator=g).double())


def test_dump_outputs_writes_float_arrays(tmp_path):
    import bench
    g = torch.Generator().manual_seed(5)
    n = 3 * bench.DUMP_PARAM_SAMPLE + 17
    model = types.SimpleNamespace(arena=types.SimpleNamespace(data=torch.randn(n, generator=g)))
    out = _step_out()
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, out, model)
    bench.dump_outputs(b, out, model)
    names = sorted(os.listdir(a))
    assert names == ["grad_norm.npy", "loss.npy", "params_sample.npy", "stats_acc.npy", "stats_loss.npy",
                     "stats_loss_ctc.npy", "weight.npy"]
    total = 0
    for f in names:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype in (np.float32, np.float64), (f, x.dtype)
        assert x.shape == y.shape and np.array_equal(x, y), f  # the sample is fixed
        total += x.nbytes
    assert total <= bench.DUMP_LIMIT
    assert np.load(os.path.join(a, "grad_norm.npy")).dtype == np.float64
    assert np.load(os.path.join(a, "loss.npy")) == pytest.approx(out[0].numpy())
    assert np.load(os.path.join(a, "weight.npy")) == 32.0
    assert np.load(os.path.join(a, "stats_acc.npy")) == out[1]["acc"].float().numpy()
    p = np.load(os.path.join(a, "params_sample.npy"))
    assert p.shape == (bench.DUMP_PARAM_SAMPLE,)
    assert np.isin(p, model.arena.data.numpy()).all()


def test_dump_outputs_refuses_more_than_the_limit(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT", 1024)
    model = types.SimpleNamespace(arena=types.SimpleNamespace(data=torch.zeros(4096)))
    with pytest.raises(RuntimeError, match="dump-outputs"):
        bench.dump_outputs(str(tmp_path / "d"), _step_out(), model)


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_dumps(tmp_path):
    """The smallest configuration (C2), two timed steps: the result line holds the headline
    fields and nothing that belongs to --full; the dump holds float arrays."""
    d = str(tmp_path / "out")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--config", "c2", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", d], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 2 and out["unit"] == "utterances/s" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(16 * 1e3 / out["ms_per_step"], rel=1e-3)
    assert not [k for k in FULL_ONLY if k in out]
    files = sorted(os.listdir(d))
    assert {"loss.npy", "grad_norm.npy", "weight.npy", "params_sample.npy"} <= set(files)
    for f in files:
        x = np.load(os.path.join(d, f))
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), f
    assert float(np.load(os.path.join(d, "loss.npy")).reshape(-1)[0]) == pytest.approx(out["loss"], abs=1e-3)
