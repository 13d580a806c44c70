"""layers.common.STREAM_ATTN_CORES = "bf16" (EA_STREAM_ATTN_TRAIN=bf16): bf16 models on the bf16-MFMA streaming
attention (csrc/attn_stream_bf16.hip), with the models, batches and bounds of tests/test_stream_attn_train_gpu.py.
Width 64 with 2 encoder heads (head dim 32; the decoder keeps 4 heads, head dim 16: a head dim padded to the MFMA
contraction step), bf16, T' = 70.
Step: loss and every parameter gradient against the float64 oracle, |on - ref| <= 4 x |off - ref| with `off` the
same step on the unfused path (that test's own body, run under the new switch value).
encode() at T' = 2049 against the f32-MFMA streaming kernel (the `=1` path): both read the same bf16 operands and
differ by the rounding of P to bf16 and of O once, which the block's later bf16 stages (linear_out, the feed-forward
and convolution modules) can carry by an ulp each: 4 bf16 ulps, 2^-6, of the unit-scale encoder output.
Captured: three steps with attention dropout 0.1 through train/graph.py, losses bit-equal to the eager ones."""
import numpy as np
import pytest
import torch

import test_stream_attn_train_gpu as S
from test_longform_encode_gpu import T

pytestmark = pytest.mark.gpu


@pytest.fixture
def bf16_cores(monkeypatch):
    from espnet_amd.layers import common
    monkeypatch.setattr(S, "HEADS", 2)
    monkeypatch.setattr(common, "STREAM_ATTN_CORES", "bf16")
    calls = []
    entry = common._stream_entry
    monkeypatch.setattr(common, "_stream_entry", lambda name, cores, q: calls.append((name, cores)) or entry(name, cores, q))
    return calls


@pytest.mark.parametrize("kind,pa", [("latest", 0.0), ("latest", 0.1), ("transformer", 0.1)])
def test_bf16_step_matches_f64_oracle(kind, pa, bf16_cores, monkeypatch):
    S.test_small_model_step_matches_f64_oracle(kind, 64, True, pa, monkeypatch)
    assert sorted(bf16_cores) == sorted([("fwd_train", "bf16"), ("bwd", "bf16")] * 3)  # encoder, decoder self / source


def test_encode_2049_frames_matches_f32_cores(bf16_cores, monkeypatch):
    from espnet_amd.layers import common
    monkeypatch.setattr(common, "STREAM_ATTN_TRAIN", True)
    m = S.models("latest", 64, True)[0]
    b = S.batch(T)
    with torch.no_grad():
        new = m.encode(b[0], b[1])[0].float().cpu().numpy()
        monkeypatch.setattr(common, "STREAM_ATTN_CORES", "f32")
        old = m.encode(b[0], b[1])[0].float().cpu().numpy()
    assert bf16_cores == [("fwd", "bf16"), ("fwd", "f32")]
    print(f"encode 2049 bf16 cores against f32 cores: max |diff| {np.abs(new - old).max():.3g}")
    np.testing.assert_allclose(new, old, atol=2.0 ** -6, rtol=2.0 ** -6)


def test_captured_bf16_steps_equal_eager_steps(bf16_cores, monkeypatch):
    from espnet_amd.layers import common
    from espnet_amd.optim.adam import ArenaAdam
    from espnet_amd.train.graph import CapturedTrainStep
    from espnet_amd.train.trainer import Trainer
    monkeypatch.setattr(common, "STREAM_ATTN_TRAIN", True)
    batch = dict(zip(("speech", "speech_lengths", "text", "text_lengths"), S.batch(287)))

    def setup():
        m = S.models("latest", 64, True, 0.1)[0]
        m.train()
        return m, ArenaAdam(m, lr=0.002, weight_decay=1e-6)

    m1, o1 = setup()
    eager = [float(Trainer.train_one_step(m1, batch, o1, None, grad_clip=5.0)[0]) for _ in range(3)]
    m2, o2 = setup()
    run = CapturedTrainStep(m2, o2, None, grad_clip=5.0, warmup=1)
    graph = [float(run(batch)[0]) for _ in range(3)]
    torch.cuda.synchronize()
    assert run.mode == "graph" and ("bwd", "bf16") in bf16_cores
    assert eager == graph and len(set(eager)) == 3
    assert torch.equal(m1.arena.grad, m2.arena.grad)
