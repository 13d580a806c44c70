"""layers.common.STREAM_ATTN_TRAIN (EA_STREAM_ATTN_TRAIN=1): one training step on the streaming attention
forward + backward against the same step on the default (unfused) path.
Small models: the one-block models of tests/test_longform_encode_gpu.py (Conformer latest / legacy, Transformer
encoder, each with the Transformer decoder) at T' = 70 (two key tiles, one ragged), in f32 at width 64 (head dim
16: the arena keeps a LayerNorm's weight and bias adjacent from there on) with attention dropout 0 and 0.1, and
once in bf16 at width 128 (head dim 32); every other dropout is 0.  Reference: the float64 oracle under torch
autograd; for dropout its attention masks are those of the default path's forward (Pd != 0 where P > 0, in call
order), which the shared keep law makes the new path's too.  The legacy restatement of the long-form test has no
dropout, so legacy runs at 0 only.  E-Branchformer (the ebf_hybrid fixture, f32) has no float64 oracle: its
reference is the fixture's gradients, the reference implementation's own f32 step.
Bound, for the loss and for every parameter by itself: |on - ref| (max over the tensor) <= 4 x |off - ref|,
absolute, so a gradient that is zero in exact arithmetic is held to the default path's own noise.  Measured and
printed.  Eager == captured: three steps with dropout 0.1 through train/graph.py, bit-equal.
T' = 2049: the step the default path refuses runs, with finite loss and gradients, and its encoder output equals
the no_grad encode() of the same model (the inference kernel) to that test's 1e-4.
Measured on MI355X, the parameter closest to its bound, on / off: latest 1.11e-06 / 5.98e-07, legacy 5.12e-08 /
2.28e-08, transformer 8.28e-08 / 3.79e-08; p 0.1: latest 3.95e-10 / 1.6e-10 (a key bias, zero in exact arithmetic),
transformer 6.73e-08 / 2.73e-08; bf16 width 128: 8.4e-04 / 6.04e-04; ebf_hybrid 3.78e-10 / 1.91e-10 (a key bias).
Loss errors on and off are equal in f32; bf16: 1.74e-03 / 1.06e-03."""
import numpy as np
import pytest
import torch

import test_longform_encode_gpu as longform
from test_longform_encode_gpu import F, HEADS, T, V, _legacy_rel_mha

pytestmark = pytest.mark.gpu


def models(kind, width=64, amp=False, pa=0.0):
    """longform._models at another width / compute dtype / attention dropout rate"""
    from oracle.asr_oracle import OracleASR
    from test_model_build import build
    from goldens import perturb_norms
    enc = dict(output_size=width, attention_heads=HEADS, linear_units=64, num_blocks=1, attention_dropout_rate=pa,
               input_layer="conv2d", normalize_before=True, **longform.ZERO)
    if kind != "transformer":
        enc.update(longform.CONFORMER, rel_pos_type=kind)
    dec = dict(longform.DEC, self_attention_dropout_rate=pa, src_attention_dropout_rate=pa)
    cfg = dict(encoder="transformer" if kind == "transformer" else "conformer", input_size=F, vocab_size=V,
               encoder_conf=enc, decoder="transformer", decoder_conf=dec,
               model_conf=dict(ctc_weight=0.3, lsm_weight=0.1, length_normalized_loss=False))
    torch.manual_seed(5)
    m = build(cfg)
    perturb_norms(m, torch.Generator().manual_seed(6))
    ora = OracleASR(cfg, {k: v.clone() for k, v in m.state_dict().items()}, dtype=torch.float64)
    return m.prepare("cuda", amp=amp, seed=3), ora


def batch(frames):
    g = torch.Generator().manual_seed(9)
    return (torch.randn(2, frames, F, generator=g), torch.tensor([frames, frames * 3 // 5]),
            torch.randint(1, V - 1, (2, 3), generator=g), torch.tensor([3, 2]))


def step(m, inputs):
    m.train()
    loss = m(*inputs)[0] if isinstance(inputs, tuple) else m(**inputs)[0]
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), {k: p.grad.double().cpu() for k, p in m.named_parameters()}


def check(name, on, off, ref):
    """on / off / ref: (loss, {parameter: gradient}); the 4 x bound on the loss and on every parameter"""
    err = lambda r, k: float((r[1][k] - ref[1][k]).abs().max())  # noqa: E731
    worst = max(ref[1], key=lambda k: err(on, k) / max(err(off, k), 1e-300))
    print(f"{name}: loss err on / off {abs(on[0] - ref[0]):.3g} / {abs(off[0] - ref[0]):.3g}; worst parameter {worst} "
          f"on / off {err(on, worst):.3g} / {err(off, worst):.3g} (largest |ref| "
          f"{float(ref[1][worst].abs().max()):.3g})")
    assert abs(on[0] - ref[0]) <= 4 * abs(off[0] - ref[0])
    for k in ref[1]:
        assert err(on, k) <= 4 * err(off, k), (k, err(on, k), err(off, k))


@pytest.mark.parametrize("kind,width,amp,pa", [(k, 64, False, 0.0) for k in ("latest", "legacy", "transformer")] +
                         [(k, 64, False, 0.1) for k in ("latest", "transformer")] + [("latest", 128, True, 0.0)])
def test_small_model_step_matches_f64_oracle(kind, width, amp, pa, monkeypatch):
    from espnet_amd.layers import common, decoder, sublayers
    from oracle import asr_oracle as O
    if kind == "legacy":
        monkeypatch.setattr(O, "rel_mha", _legacy_rel_mha)
    masks = []

    def recording_attn_fwd(*a, **kw):  # the default path's attention, keeping its dropout mask
        O_, P, Pd, ldT = common.attn_fwd(*a, **kw)
        masks.append(((Pd.float() != 0) | ~(P > 0)).view(kw["B"], kw["H"], kw["T1"], ldT)[..., :kw["T2"]].cpu())
        return O_, P, Pd, ldT

    for mod in (decoder, sublayers):
        monkeypatch.setattr(mod, "attn_fwd", recording_attn_fwd)
    b = batch(287)  # ((287 - 1) // 2 - 1) // 2 = 70
    m, ora = models(kind, width, amp, pa)
    off = step(m, b)
    assert len(masks) == 3  # encoder block, decoder self- and source attention, the oracle's order
    it = iter(masks)
    monkeypatch.setattr(O, "drop", lambda x, p, training: x if not p else x * next(it).to(x.dtype) / (1 - p))
    loss = ora(*b)[0]
    loss.backward()
    ref = (loss.item(), {k: r.grad for k, r in ora.params.items() if r.grad is not None})
    monkeypatch.setattr(common, "STREAM_ATTN_TRAIN", True)
    on = step(models(kind, width, amp, pa)[0], b)
    assert len(masks) == 3  # the switch took every attention off the default path
    check(f"{kind} width {width} {'bf16' if amp else 'f32'} p={pa}", on, off, ref)


def test_ebranchformer_step_matches_reference_fixture(monkeypatch):
    from ebranchformer_goldens import build_loaded
    from espnet_amd.layers import common
    from goldens import section
    runs = []
    for on in (False, True):
        monkeypatch.setattr(common, "STREAM_ATTN_TRAIN", on)
        cfg, d, m = build_loaded("ebf_hybrid")
        m.prepare("cuda", amp=False)
        torch.manual_seed(4242)
        runs.append(step(m, {k: torch.from_numpy(v) for k, v in section(d, "in").items()}))
    ref = (float(d["out.loss"]), {k: torch.from_numpy(g).double() for k, g in section(d, "g").items()})
    check("ebf_hybrid f32", runs[1], runs[0], ref)


def test_captured_steps_equal_eager_steps_with_dropout(monkeypatch):
    """tests/test_ebranchformer_model_gpu.py's eager == captured test in f32 (every attention streaming) with
    the switch on: bit-equal losses, gradients and weights over warm-up, capture and replay."""
    import test_dp_ragged_gpu as R
    from ebranchformer_goldens import build_loaded
    from espnet_amd.layers import common
    from espnet_amd.optim.adam import ArenaAdam
    from espnet_amd.schedulers.warmup_lr import WarmupLR
    from espnet_amd.train.graph import CapturedTrainStep
    from espnet_amd.train.trainer import Trainer
    monkeypatch.setattr(common, "STREAM_ATTN_TRAIN", True)
    torch.cuda.set_device(0)

    def setup():
        m = build_loaded("ebf_hybrid", dropout_rate=0.1, positional_dropout_rate=0.1, attention_dropout_rate=0.1)[2]
        m.prepare("cuda:0", amp=False, seed=77)
        m.train()
        opt = ArenaAdam(m, lr=0.002, weight_decay=1e-6)
        return m, opt, WarmupLR(opt, warmup_steps=15000)

    batches = [R._global_batches(1, seed=11 + i)[0] for i in range(3)]  # one input shape
    m1, o1, s1 = setup()
    torch.manual_seed(99)
    eager = [float(Trainer.train_one_step(m1, b, o1, s1, grad_clip=5.0)[0]) for b in batches]
    m2, o2, s2 = setup()
    run = CapturedTrainStep(m2, o2, s2, grad_clip=5.0, warmup=1)
    torch.manual_seed(99)
    graph = [float(run(b)[0]) for b in batches]
    torch.cuda.synchronize()
    assert len(run.graphs) == 1 and run.mode == "graph"
    assert eager == graph and len(set(eager)) == len(eager)
    assert torch.equal(m1.arena.grad, m2.arena.grad)
    for (k, p1), p2 in zip(m1.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(p1, p2), k


@pytest.mark.parametrize("kind", ["latest", "legacy", "transformer"])
def test_step_at_2049_frames(kind, monkeypatch):
    from espnet_amd.layers import common
    m, _ = models(kind)
    b = batch(T)
    m.train()
    with pytest.raises(NotImplementedError, match="2048 keys.*inference is served"):  # switch off: as before
        m(*b)
    monkeypatch.setattr(common, "STREAM_ATTN_TRAIN", True)
    with torch.no_grad():
        enc = m.encode(b[0], b[1])[0]
    loss = m(*b)[0]
    loss.backward()
    assert torch.isfinite(loss)
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())
    np.testing.assert_allclose(m._last_encoder_out[0].detach().cpu().numpy(), enc.cpu().numpy(), atol=1e-4, rtol=1e-4)
