"""E-Branchformer, whole model on the MI355X against the reference fixtures
(tests/capture_ebranchformer_goldens.py): loss, every stat, encoder output and lengths, every
parameter gradient, and the host RNG position after the step (one MultiSequential layer-drop draw
per forward); bf16 AMP closeness; no state carried between steps; eval encode and CTC greedy;
checkpoint round trip; eager step == captured-step replay with dropout on."""
import numpy as np
import pytest
import torch

from ebranchformer_goldens import FIXTURES, build_loaded
from goldens import assert_grad_close, is_null_grad, section

pytestmark = pytest.mark.gpu

STEPS = 3


def run(name, amp=False, train=True, backward=True):
    cfg, d, m = build_loaded(name)
    m.prepare("cuda", amp=amp)
    m.train(train)
    inp = {k: torch.from_numpy(v) for k, v in section(d, "in").items()}
    torch.manual_seed(4242)  # as the capture: the host generator the layer-drop draw advances
    if train:
        loss, stats, weight = m(**inp)
    else:
        with torch.no_grad():
            loss, stats, weight = m(**inp)
    next_rand = torch.rand(1)
    if train and backward:
        loss.backward()
    torch.cuda.synchronize()
    return cfg, d, m, loss, stats, weight, next_rand


@pytest.mark.parametrize("name", FIXTURES)
def test_ebranchformer_fp32_parity(name):
    cfg, d, m, loss, stats, weight, next_rand = run(name)
    print(f"{name} loss: {loss.item():.6f} (reference {d['out.loss'].item():.6f})")
    np.testing.assert_allclose(loss.item(), d["out.loss"], rtol=2e-6, atol=1e-4)
    assert weight.item() == d["out.weight"]
    for k, v in section(d, "stat").items():
        print(f"{name} {k}: {stats[k].item():.6f} (reference {v.item():.6f})")
        np.testing.assert_allclose(stats[k].item(), v, rtol=2e-6, atol=1e-4, err_msg=k)
    assert torch.equal(next_rand, torch.from_numpy(d["out.next_rand"]))
    enc, olens = m._last_encoder_out
    np.testing.assert_array_equal(olens.cpu().numpy(), d["out.encoder_out_lens"])
    np.testing.assert_allclose(enc.detach().cpu().numpy(), d["out.encoder_out"], atol=1e-4, rtol=1e-4)
    params = dict(m.named_parameters())
    grads = section(d, "g")
    assert set(grads) == set(params)
    e0 = "encoder.encoders.0."
    for k in ("cgmlp.csgu.norm.weight", "cgmlp.csgu.norm.bias", "cgmlp.csgu.conv.weight", "cgmlp.csgu.conv.bias",
              "cgmlp.channel_proj1.0.weight", "depthwise_conv_fusion.weight", "depthwise_conv_fusion.bias",
              "merge_proj.weight", "attn.pos_bias_u", "norm_mlp.weight"):
        assert e0 + k in grads, k
    for k, g in grads.items():
        assert_grad_close(params[k].grad.cpu().numpy(), g, k, rtol=2e-4, scale_tol=1e-5, atol=2e-5)


@pytest.mark.parametrize("name", FIXTURES)
def test_ebranchformer_bf16_amp_close(name):
    """As test_model_bf16_amp_close: per-tensor relative L2 distance from the reference's fp32
    gradient below 6e-2."""
    cfg, d, m, loss, stats, weight, _ = run(name, amp=True)
    print(f"{name} bf16 loss: {loss.item():.6f} (reference {d['out.loss'].item():.6f})")
    np.testing.assert_allclose(loss.item(), d["out.loss"], rtol=2e-2)
    params = dict(m.named_parameters())
    worst = []
    for k, g in section(d, "g").items():
        # the key bias of this block's attention is analytically gradient-free too (softmax
        # invariance, as goldens.NULL_GRAD_SUFFIXES' self_attn.linear_k.bias): its fp32 reference
        # gradient is rounding noise (~1e-8), no yardstick for a relative distance
        if is_null_grad(k) or k.endswith(".attn.linear_k.bias"):
            continue
        mine = params[k].grad.double().cpu()
        ref = torch.from_numpy(g).double()
        worst.append((float((mine - ref).norm() / ref.norm().clamp_min(1e-30)), k))
    worst.sort(reverse=True)
    print(name, "worst per-tensor bf16 rel L2:", worst[:4])
    assert worst[0][0] < 6e-2, worst[:5]


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("amp", [False, True])
def test_second_step_carries_nothing_stale(name, amp):
    """Two identical steps from the same weights (gradient arena zeroed between them) give
    bit-equal losses and gradient arenas."""
    cfg, d, m, loss, stats, weight, _ = run(name, amp=amp)
    g1 = m.arena.grad.clone()
    m.arena.zero_grad()
    inp = {k: torch.from_numpy(v) for k, v in section(d, "in").items()}
    loss2, _, _ = m(**inp)
    loss2.backward()
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2)
    assert torch.equal(g1, m.arena.grad)


def test_eval_encode_and_ctc_greedy():
    from espnet_amd.asr.inference import ctc_greedy
    cfg, d, m, loss, stats, weight, _ = run("ebf_hybrid", train=False)
    np.testing.assert_allclose(loss.item(), d["out.loss"], rtol=2e-6, atol=1e-4)  # dropout 0: eval == train
    assert stats["cer_ctc"] is not None and np.isfinite(float(stats["cer_ctc"]))
    inp = {k: torch.from_numpy(v) for k, v in section(d, "in").items()}
    with torch.no_grad():
        enc, lens = m.encode(inp["speech"], inp["speech_lengths"])
    np.testing.assert_array_equal(lens.cpu().numpy(), d["out.encoder_out_lens"])
    np.testing.assert_allclose(enc.cpu().numpy(), d["out.encoder_out"], atol=1e-4, rtol=1e-4)
    hyps = ctc_greedy(m, inp["speech"], inp["speech_lengths"])
    assert len(hyps) == inp["speech"].shape[0] and all(isinstance(h, list) for h in hyps)
    with torch.no_grad():  # the helper decodes each utterance alone, unpadded
        le = int(inp["speech_lengths"][0])
        e0, l0 = m.encode(inp["speech"][:1, :le], inp["speech_lengths"][:1])
        ids = m.ctc.argmax(e0)[0, :int(l0[0])].tolist()
    want, prev = [], None
    for t in ids:
        if t != prev and t != 0:
            want.append(t)
        prev = t
    assert hyps[0] == want


def _setup(dropout=0.1):
    from espnet_amd.optim.adam import ArenaAdam
    from espnet_amd.schedulers.warmup_lr import WarmupLR
    cfg, d, m = build_loaded("ebf_hybrid", dropout_rate=dropout, positional_dropout_rate=dropout,
                             attention_dropout_rate=dropout)
    m.prepare("cuda:0", amp=True, seed=77)
    m.train()
    opt = ArenaAdam(m, lr=0.002, weight_decay=1e-6)
    return m, opt, WarmupLR(opt, warmup_steps=15000)


def _same_state(m1, m2):
    """Every parameter bit-equal (the arena's alignment padding between them is not state)."""
    sd2 = m2.state_dict()
    for k, v in m1.state_dict().items():
        assert torch.equal(v, sd2[k]), k


def test_checkpoint_round_trip_is_bit_exact(tmp_path):
    """save_checkpoint after one step, resume into a freshly built model: weights, optimizer
    state and the next step are bit-equal to the run that never stopped."""
    import test_dp_ragged_gpu as R
    from espnet_amd.train.checkpoint import EpochReporter, resume, save_checkpoint
    from espnet_amd.train.trainer import Trainer
    batches = [R._global_batches(1, seed=21 + i)[0] for i in range(2)]
    m, opt, sched = _setup(dropout=0.0)
    Trainer.train_one_step(m, batches[0], opt, sched, grad_clip=5.0)
    save_checkpoint(tmp_path, m, EpochReporter(epoch=1), [opt], [sched])
    ck = torch.load(tmp_path / "checkpoint.pth", map_location="cpu", weights_only=True)
    assert any(k.startswith("encoder.encoders.2.cgmlp.csgu.conv.") for k in ck["model"])
    for k, v in m.state_dict().items():
        assert torch.equal(ck["model"][k], v.cpu()), k
    m2, opt2, sched2 = _setup(dropout=0.0)
    with torch.no_grad():
        m2.arena.data.add_(1.0)  # whatever it held is replaced
    resume(tmp_path / "checkpoint.pth", m2, EpochReporter(), [opt2], [sched2], ngpu=1)
    torch.cuda.synchronize()
    _same_state(m, m2)
    la = Trainer.train_one_step(m, batches[1], opt, sched, grad_clip=5.0)[0]
    lb = Trainer.train_one_step(m2, batches[1], opt2, sched2, grad_clip=5.0)[0]
    torch.cuda.synchronize()
    assert float(la) == float(lb)
    _same_state(m, m2)


def test_captured_steps_equal_eager_steps_with_dropout():
    """Dropout 0.1 everywhere (the CSGU's, both branch outputs', the merge's): three eager steps
    and three CapturedTrainStep steps (warm-up, capture, replay) give bit-equal losses, gradients
    and weights, and leave the host generator at the same position."""
    import test_dp_ragged_gpu as R
    from espnet_amd.train.graph import CapturedTrainStep
    from espnet_amd.train.trainer import Trainer
    torch.cuda.set_device(0)
    batches = [R._global_batches(1, seed=11 + i)[0] for i in range(STEPS)]  # one input shape
    m1, o1, s1 = _setup()
    torch.manual_seed(99)
    eager = [float(Trainer.train_one_step(m1, b, o1, s1, grad_clip=5.0)[0]) for b in batches]
    rng_eager = torch.get_rng_state()
    m2, o2, s2 = _setup()
    run_ = CapturedTrainStep(m2, o2, s2, grad_clip=5.0, warmup=1)
    torch.manual_seed(99)
    graph = [float(run_(b)[0]) for b in batches]
    torch.cuda.synchronize()
    assert len(run_.graphs) == 1 and run_.mode == "graph"
    assert eager == graph
    assert len(set(eager)) == len(eager)
    assert torch.equal(rng_eager, torch.get_rng_state())
    assert torch.equal(m1.arena.grad, m2.arena.grad)
    for (k, p1), p2 in zip(m1.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(p1, p2), k
