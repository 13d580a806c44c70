"""Legacy rel-pos Conformer (rel_pos_type: legacy), whole model on the MI355X against the
reference fixtures (tests/capture_legacy_relpos_goldens.py): legacy_tiny (head dim 16) and
legacy_dk64 (head dim 64, T' = 66 and 49) in fp32 with the assertions and tolerances of
tests/test_model_gpu.py test_model_fp32_parity; bf16 AMP within test_model_bf16_amp_close's
per-tensor bound of the reference's fp32 gradients; eval-mode encode() against the stored
eval-mode output; a shorter utterance after a longer one sees the grown table; intermediate /
self-conditioned CTC taps run on top of it; eager steps == captured-step replays bit-for-bit."""
import numpy as np
import pytest
import torch

from goldens import assert_grad_close, is_null_grad, section
from legacy_relpos_goldens import FIXTURES, build_loaded

pytestmark = pytest.mark.gpu


def run(name, amp=False):
    cfg, d, m = build_loaded(name)
    m.prepare("cuda", amp=amp)
    m.train()
    inp = {k: torch.from_numpy(v) for k, v in section(d, "in").items()}
    loss, stats, weight = m(**inp)
    loss.backward()
    torch.cuda.synchronize()
    return cfg, d, m, loss, stats, weight


@pytest.mark.parametrize("name", FIXTURES)
def test_legacy_fp32_parity(name):
    cfg, d, m, loss, stats, weight = run(name)
    print(f"{name} loss: {loss.item():.6f} (reference {d['out.loss'].item():.6f})")
    np.testing.assert_allclose(loss.item(), d["out.loss"], rtol=2e-6, atol=1e-4)
    assert weight.item() == d["out.weight"]
    for k, v in section(d, "stat").items():
        np.testing.assert_allclose(stats[k].item(), v, rtol=2e-6, atol=1e-4, err_msg=k)
    enc, olens = m._last_encoder_out
    np.testing.assert_array_equal(olens.cpu().numpy(), d["out.encoder_out_lens"])
    np.testing.assert_allclose(enc.detach().cpu().numpy(), d["out.encoder_out"], atol=1e-4, rtol=1e-4)
    np.testing.assert_allclose(m.ctc.logits(enc.detach()).cpu().numpy(), d["out.ctc_logits"], atol=1e-4, rtol=1e-4)
    np.testing.assert_array_equal(m.ctc.argmax(enc.detach()).cpu().numpy(), d["out.ctc_argmax"])
    params = dict(m.named_parameters())
    grads = section(d, "g")
    assert set(grads) == set(params)
    for k, g in grads.items():
        assert_grad_close(params[k].grad.cpu().numpy(), g, k, rtol=2e-4, scale_tol=1e-5, atol=2e-5)
    sd = m.state_dict()
    for k, v in section(d, "buf_after").items():
        np.testing.assert_allclose(sd[k].cpu().numpy(), v, atol=1e-5, rtol=1e-5, err_msg=k)


@pytest.mark.parametrize("name", FIXTURES)
def test_legacy_bf16_amp_close(name):
    """As test_model_bf16_amp_close: per-tensor relative L2 distance from the reference's fp32
    gradient below 6e-2 (legacy_dk64: the fused kernels' legacy variant, forward and backward)."""
    cfg, d, m, loss, stats, weight = run(name, amp=True)
    print(f"{name} bf16 loss: {loss.item():.6f} (reference {d['out.loss'].item():.6f})")
    np.testing.assert_allclose(loss.item(), d["out.loss"], rtol=2e-2)
    params = dict(m.named_parameters())
    worst = []
    for k, g in section(d, "g").items():
        if is_null_grad(k):
            continue
        mine = params[k].grad.double().cpu()
        ref = torch.from_numpy(g).double()
        worst.append((float((mine - ref).norm() / ref.norm().clamp_min(1e-30)), k))
    worst.sort(reverse=True)
    print(name, "worst per-tensor bf16 rel L2:", worst[:4])
    assert worst[0][0] < 6e-2, worst[:5]


def test_legacy_eval_encode_matches_reference():
    cfg, d, m = build_loaded("legacy_dk64")
    m.prepare("cuda", amp=False)
    m.eval()
    inp = {k: torch.from_numpy(v) for k, v in section(d, "in").items()}
    with torch.no_grad():
        enc, lens = m.encode(inp["speech"], inp["speech_lengths"])
    np.testing.assert_array_equal(lens.cpu().numpy(), d["out.encoder_out_eval_lens"])
    np.testing.assert_allclose(enc.cpu().numpy(), d["out.encoder_out_eval"], atol=1e-4, rtol=1e-4)
    assert float(np.abs(d["out.encoder_out_eval"] - d["out.encoder_out"]).max()) > 1e-3  # not the training output


def test_short_utterance_after_a_long_one_sees_the_grown_table():
    """max_pos_emb_len 16 < T' = 29: the first forward rebuilds the table at 29 rows and it stays;
    the second utterance alone (T' = 15) then reads rows of the 29-row table, not of a 16-row one:
    its output differs from a fresh model's, and equals a fresh model's whose table was built at
    29 rows from the start."""
    def model(max_len):
        cfg, d, m = build_loaded("legacy_tiny", max_pos_emb_len=max_len)
        m.prepare("cuda", amp=False)
        m.eval()
        return d, m

    def enc(m, speech, lens):
        with torch.no_grad():
            return m.encode(speech, lens)[0].cpu()

    d, m = model(16)
    inp = {k: torch.from_numpy(v) for k, v in section(d, "in").items()}
    short = (inp["speech"][2:3, :64].contiguous(), inp["speech_lengths"][2:3])
    enc(m, inp["speech"], inp["speech_lengths"])
    assert m.encoder.embed.out[1].n_rows == 29
    after_long = enc(m, *short)
    _, fresh16 = model(16)
    _, fresh29 = model(29)
    assert torch.equal(after_long, enc(fresh29, *short))
    assert float((after_long - enc(fresh16, *short)).abs().max()) > 1e-3


@pytest.mark.parametrize("conditioning", [False, True])
def test_legacy_with_interctc_taps_trains_and_encodes(conditioning):
    """interctc_layer_idx (and the conditioning) on a legacy encoder: a training step gives finite
    gradients for every parameter, and eval encode() returns the tap outputs."""
    from test_model_build import build
    from legacy_relpos_goldens import load
    cfg, d = load("legacy_tiny")
    cfg["encoder_conf"] = dict(cfg["encoder_conf"], interctc_layer_idx=[1], interctc_use_conditioning=conditioning)
    cfg["model_conf"] = dict(cfg["model_conf"], interctc_weight=0.3)
    torch.manual_seed(0)
    m = build(cfg)
    m.prepare("cuda", amp=False)
    m.train()
    inp = {k: torch.from_numpy(v) for k, v in section(d, "in").items()}
    loss, stats, _ = m(**inp)
    loss.backward()
    torch.cuda.synchronize()
    assert np.isfinite(loss.item()) and "loss_interctc_layer1" in stats
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    g = dict(m.named_parameters())["encoder.encoders.0.self_attn.linear_pos.weight"].grad
    assert float(g.abs().max()) > 0
    m.eval()
    with torch.no_grad():
        (enc, taps), lens = m.encode(inp["speech"], inp["speech_lengths"])
    assert [li for li, _ in taps] == [1] and taps[0][1].shape == enc.shape


def _setup(dropout, name="legacy_tiny", amp=False):
    from espnet_amd.optim.adam import ArenaAdam
    from espnet_amd.schedulers.warmup_lr import WarmupLR
    cfg, d, m = build_loaded(name, dropout_rate=dropout, positional_dropout_rate=dropout,
                             attention_dropout_rate=dropout)
    m.prepare("cuda:0", amp=amp, seed=77)
    m.train()
    opt = ArenaAdam(m, lr=0.002, weight_decay=1e-6)
    return m, opt, WarmupLR(opt, warmup_steps=15000)


@pytest.mark.parametrize("name,amp", [("legacy_tiny", False), ("legacy_dk64", True)])
def test_captured_steps_equal_eager_steps(name, amp):
    """Two training steps through CapturedTrainStep (warm-up, then capture and replay) equal two
    eager steps bit-for-bit: losses, gradients and weights — legacy_tiny in fp32 (the unfused
    kernels) and legacy_dk64 under AMP (the fused ones, the band fix-up and the zeroed table rows).
    Dropout 0.1, so the T-row table's dropout site and the attention dropout are in the graph."""
    import test_dp_ragged_gpu as R
    from espnet_amd.train.graph import CapturedTrainStep
    from espnet_amd.train.trainer import Trainer
    torch.cuda.set_device(0)
    batches = [R._global_batches(1, seed=11 + i)[0] for i in range(2)]  # one input shape
    nf = 48 if name == "legacy_dk64" else 80  # the fixture model's input size
    batches = [dict(b, speech=b["speech"][..., :nf].contiguous()) for b in batches]
    m1, o1, s1 = _setup(0.1, name, amp)
    torch.manual_seed(99)
    eager = [float(Trainer.train_one_step(m1, b, o1, s1, grad_clip=5.0)[0]) for b in batches]
    m2, o2, s2 = _setup(0.1, name, amp)
    run_ = CapturedTrainStep(m2, o2, s2, grad_clip=5.0, warmup=1)
    torch.manual_seed(99)
    graph = [float(run_(b)[0]) for b in batches]
    torch.cuda.synchronize()
    assert len(run_.graphs) == 1 and run_.mode == "graph"
    assert eager == graph
    assert eager[0] != eager[1]
    assert torch.equal(m1.arena.grad, m2.arena.grad)
    for (k, p1), p2 in zip(m1.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(p1, p2), k


def test_amp_eval_encode_runs_the_fused_legacy_forward(monkeypatch):
    """Head dim 64 under bf16 AMP without a backward (eval encode()): the fused forward's legacy
    variant runs, once per block, and agrees with the unfused legacy kernels on the same model.
    Bound: 2e-2 rel-L2 on the encoder output, two blocks of the 1e-2 that
    tests/test_attention_gpu.py allows between the fused and the unfused attention output."""
    from espnet_amd._lib import REL_LEGACY, lib
    from espnet_amd.layers import common
    cfg, d, m = build_loaded("legacy_dk64")
    m.prepare("cuda", amp=True)
    m.eval()
    inp = {k: torch.from_numpy(v) for k, v in section(d, "in").items()}
    calls = []
    real = lib.ea_attn_fused_fwd2_mode
    monkeypatch.setattr(lib, "ea_attn_fused_fwd2_mode", lambda *a: (calls.append(a[-2]), real(*a))[1])
    with torch.no_grad():
        fused, lens = m.encode(inp["speech"], inp["speech_lengths"])
    assert calls == [REL_LEGACY] * len(m.encoder.encoders)
    monkeypatch.setattr(common, "FUSED_ATTN", False)
    with torch.no_grad():
        unfused, _ = m.encode(inp["speech"], inp["speech_lengths"])
    assert len(calls) == len(m.encoder.encoders)
    e = float((fused - unfused).norm() / unfused.norm())
    print(f"legacy_dk64 AMP eval encode, fused vs unfused forward: rel-L2 {e:.3g}")
    assert 0 < e < 2e-2
    ref = torch.from_numpy(d["out.encoder_out_eval"]).cuda()
    print("  vs the reference's fp32 eval output:", float((fused - ref).norm() / ref.norm()),
          float((unfused - ref).norm() / ref.norm()))


def test_fused_amp_step_matches_the_unfused_amp_step(monkeypatch):
    """legacy_dk64 under AMP: the training step on the fused kernels against the same step with the
    encoder's attention on the unfused kernels.  Both are bf16 evaluations of the same function, each
    allowed 6e-2 per tensor from the fp32 reference (test_legacy_bf16_amp_close); the same bound is
    asked between them."""
    from espnet_amd._lib import REL_LEGACY, lib
    from espnet_amd.layers import sublayers
    calls = []
    real = lib.ea_attn_fused_bwd2_mode
    monkeypatch.setattr(lib, "ea_attn_fused_bwd2_mode", lambda *a: (calls.append(a[-2]), real(*a))[1])
    cfg, d, m, loss, _, _ = run("legacy_dk64", amp=True)
    assert calls.count(REL_LEGACY) == len(m.encoder.encoders)  # (the decoder's calls are latest)
    fused = {k: p.grad.double().cpu() for k, p in m.named_parameters()}
    n = len(calls)
    monkeypatch.setattr(sublayers, "fused_attn_ok", lambda *a: False)
    _, _, m2, loss2, _, _ = run("legacy_dk64", amp=True)
    assert REL_LEGACY not in calls[n:]
    np.testing.assert_allclose(loss.item(), loss2.item(), rtol=2e-2)
    worst = []
    for k, p in m2.named_parameters():
        if is_null_grad(k):
            continue
        g = p.grad.double().cpu()
        worst.append((float((fused[k] - g).norm() / g.norm().clamp_min(1e-30)), k))
    worst.sort(reverse=True)
    print("legacy_dk64 fused vs unfused AMP step, worst per-tensor rel L2:", worst[:4])
    assert worst[0][0] < 6e-2, worst[:5]
