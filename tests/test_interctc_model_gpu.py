"""Intermediate CTC / self-conditioned CTC, whole model on the MI355X against the reference
fixtures (tests/capture_interctc_goldens.py): loss, every stat including the taps' losses,
encoder output, the taps' normalised outputs, every parameter gradient (the conditioning
layer's, and ctc_lo / after_norm, which every tap and the final head write), the BatchNorm
buffers, and the host RNG position after the step (no layer-drop draw with taps)."""
import numpy as np
import pytest
import torch

from goldens import assert_grad_close, is_null_grad, section
from interctc_goldens import FIXTURES, build_loaded

pytestmark = pytest.mark.gpu


def run(name, amp=False, train=True, backward=True):
    cfg, d, m = build_loaded(name)
    m.prepare("cuda", amp=amp)
    m.train(train)
    inp = {k: torch.from_numpy(v) for k, v in section(d, "in").items()}
    torch.manual_seed(4242)  # as the capture: the host generator a layer-drop draw would advance
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
def test_interctc_fp32_parity(name):
    cfg, d, m, loss, stats, weight, next_rand = run(name)
    np.testing.assert_allclose(loss.item(), d["out.loss"], rtol=2e-6, atol=1e-4)
    assert weight.item() == d["out.weight"]
    ref_stats = section(d, "stat")
    taps = cfg["encoder_conf"]["interctc_layer_idx"]
    assert all(f"loss_interctc_layer{l}" in ref_stats for l in taps)
    for k, v in ref_stats.items():
        print(f"{name} {k}: {stats[k].item():.6f} (reference {v.item():.6f})")
        np.testing.assert_allclose(stats[k].item(), v, rtol=2e-6, atol=1e-4, err_msg=k)
    for l in taps:
        assert stats[f"cer_interctc_layer{l}"] is None  # training
    assert torch.equal(next_rand, torch.from_numpy(d["out.next_rand"]))
    enc, olens = m._last_encoder_out
    np.testing.assert_array_equal(olens.cpu().numpy(), d["out.encoder_out_lens"])
    np.testing.assert_allclose(enc.detach().cpu().numpy(), d["out.encoder_out"], atol=1e-4, rtol=1e-4)
    inter = dict(m._last_intermediate_outs)
    assert sorted(inter) == sorted(taps)
    for l in taps:
        np.testing.assert_allclose(inter[l].cpu().numpy(), d[f"mid.interctc{l}"], atol=1e-4, rtol=1e-4,
                                   err_msg=f"tap {l}")
    params = dict(m.named_parameters())
    grads = section(d, "g")
    assert set(grads) == set(params)
    for k in ("ctc.ctc_lo.weight", "ctc.ctc_lo.bias", "encoder.after_norm.weight", "encoder.after_norm.bias"):
        assert k in grads
    if cfg["encoder_conf"]["interctc_use_conditioning"]:
        assert "encoder.conditioning_layer.weight" in grads and "encoder.conditioning_layer.bias" in grads
    for k, g in grads.items():
        assert_grad_close(params[k].grad.cpu().numpy(), g, k, rtol=2e-4, scale_tol=1e-5, atol=2e-5)
    sd = m.state_dict()
    for k, v in section(d, "buf_after").items():
        np.testing.assert_allclose(sd[k].cpu().numpy(), v, atol=1e-5, rtol=1e-5, err_msg=k)


@pytest.mark.parametrize("name", FIXTURES)
def test_interctc_bf16_amp_close(name):
    """As test_model_bf16_amp_close: per-tensor relative L2 distance from the reference's fp32
    gradient below 6e-2."""
    cfg, d, m, loss, stats, weight, _ = run(name, amp=True)
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


def test_interctc_eval_stats_encode_and_greedy():
    from espnet_amd.asr.inference import ctc_greedy
    cfg, d, m, loss, stats, weight, _ = run("interctc_sc_hybrid", train=False)
    taps = cfg["encoder_conf"]["interctc_layer_idx"]
    for l in taps:
        cer = stats[f"cer_interctc_layer{l}"]
        assert cer is not None and np.isfinite(float(cer)), (l, cer)
        assert np.isfinite(stats[f"loss_interctc_layer{l}"].item())
    assert stats["cer_ctc"] is not None
    inp = {k: torch.from_numpy(v) for k, v in section(d, "in").items()}
    with torch.no_grad():
        (enc, inter), lens = m.encode(inp["speech"], inp["speech_lengths"])
    assert [l for l, _ in inter] == taps and all(y.shape == enc.shape for _, y in inter)
    np.testing.assert_array_equal(lens.cpu().numpy(), d["out.encoder_out_lens"])
    hyps = ctc_greedy(m, inp["speech"], inp["speech_lengths"])
    assert len(hyps) == inp["speech"].shape[0] and all(isinstance(h, list) for h in hyps)
    with torch.no_grad():  # the helper decoded the unwrapped encoder output of utterance 0 alone
        le = int(inp["speech_lengths"][0])
        (e0, _), l0 = m.encode(inp["speech"][:1, :le], inp["speech_lengths"][:1])
        ids = m.ctc.argmax(e0)[0, :int(l0[0])].tolist()
    want, prev = [], None
    for t in ids:
        if t != prev and t != 0:
            want.append(t)
        prev = t
    assert hyps[0] == want


@pytest.mark.parametrize("name", ["interctc_sc_hybrid", "interctc_plain"])
def test_second_step_accumulates_nothing_stale(name):
    """Two identical steps from the same weights (gradient arena zeroed between them) give
    bit-equal gradient arenas: no tap state survives a backward."""
    cfg, d, m, loss, stats, weight, _ = run(name)
    g1 = m.arena.grad.clone()
    m.arena.zero_grad()
    inp = {k: torch.from_numpy(v) for k, v in section(d, "in").items()}
    loss2, _, _ = m(**inp)
    loss2.backward()
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2)
    assert torch.equal(g1, m.arena.grad)
