"""VGGRNNEncoder (encoder: vgg_rnn) on the GPU against the reference's fixtures
(tests/capture_vgg_rnn_goldens.py).  f32: output, output lengths, every parameter gradient, exact
zeros past the output lengths, junk in the padded input frames (VGG2L masks nothing: the
convolutions see it, as the reference's do).  bf16: the same arrays against the float64 restatement
on bf16-rounded operands and the kernels' own decisions, and those decisions against the
restatement's outside the recorded bands.  Unsorted lengths; padding beyond the longest row; the
hybrid model with decoder: rnn: the four-step training trace, eager against the captured-step
runner (f32 and bf16) on batches of one shape and different lengths, and the beam search.

The fixtures' seeds keep every float64 pre-activation and pooling gap MARGIN x the reference's own
f32 error away from a decision boundary, so every ReLU and argmax decision is pinned and the
arrays are smooth functions of the weights around them.

Tolerance (tests/lstm_train_goldens.py tolerance): an array passes within 4 x its recorded err
(max |f32 - f64| of the reference itself) or 4 f32 ulps at the array's largest magnitude.
"""
import numpy as np
import pytest
import torch

import vgg_rnn_goldens as G
from goldens import load, section

pytestmark = pytest.mark.gpu
MARGIN = G.MARGIN


def _check(got, ref, err, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    tol = G.tolerance(ref, err, MARGIN)
    worst = float(np.abs(got - ref).max()) if ref.size else 0.0
    print(f"{what}: max |err| {worst:.3e}, tolerance {tol:.3e}")
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    assert worst <= tol, f"{what}: max |err| {worst:.3e} > {tol:.3e}"


def _train_pass(enc, inp):
    """forward + backward under the cotangent -> (y, olens, grads) on the CPU."""
    enc.train()
    for p in enc.parameters():
        p.grad.zero_()
    y, olens, _ = enc(inp["xs_pad"].cuda(), inp["ilens"].cuda())
    y.backward(inp["cot"].cuda())
    torch.cuda.synchronize()
    return y.detach().cpu(), olens.cpu(), {k: p.grad.detach().cpu().clone() for k, p in enc.named_parameters()}


def _fixture(name, amp=False):
    from espnet_amd.asr.encoder.vgg_rnn_encoder import VGGRNNEncoder
    cfg, d, enc, inp = G.build(name, VGGRNNEncoder)
    G.prepare_encoder(enc, amp)
    return cfg, d, enc, inp


def _check_grads(cfg, d, g):
    for k, v in g.items():
        err, s = d[f"err.grad.{k}"], cfg["gstride"][k]
        _check(v.reshape(-1)[::s], d[f"gsamp.{k}"], err, "grad sample " + k)
        tol = G.tolerance(d[f"gsamp.{k}"], err, MARGIN)
        # the norm of n elements each within the array's tolerance
        assert abs(float(v.double().norm()) - float(d[f"gnorm.{k}"])) <= tol * v.numel() ** 0.5, k


@pytest.mark.parametrize("name", G.NAMES)
def test_fixture_parity(name):
    cfg, d, enc, inp = _fixture(name)
    y, olens, g = _train_pass(enc, inp)
    _check(y, d["out.y"], d["err.y"], "y")
    assert olens.tolist() == d["out.olens"].tolist() == [G.half2(n) for n in cfg["ilens"]]
    assert len(set(olens.tolist())) > 1
    for b, n in enumerate(olens.tolist()):
        assert not y[b, n:].any(), "output frames past olens must be exactly 0"
    _check_grads(cfg, d, g)


@pytest.mark.parametrize("name", G.NAMES)
def test_bf16_against_the_restatement_on_the_kernels_decisions(name):
    """bf16 end to end.  A decision near a tie cannot be pinned (a bf16 operand on the other side of
    a rounding boundary moves later pre-activations by about 1e-3), so the encoder's own decisions()
    are fed to the float64 restatement on bf16-rounded operands (tests/vgg_rnn_goldens.py restate):
    output and every gradient within MARGIN x bf.err.*; and the decisions themselves must be the
    restatement's own wherever its |pre-activation| (top-two gap) exceeds the layer's recorded band."""
    cfg, d, enc, inp = _fixture(name, amp=True)
    sd = {k: v.detach().cpu().clone() for k, v in enc.state_dict().items()}
    vgg = enc.enc[0]
    vgg.keep_decisions = True
    y, olens, g = _train_pass(enc, inp)
    D = {k: v.cpu() for k, v in vgg.decisions().items()}
    ry, rl, rg, _, _ = G.restate(sd, cfg, inp, torch.float64, bf=True, decisions=D)
    assert olens.tolist() == rl.tolist() == d["out.olens"].tolist()
    for b, n in enumerate(olens.tolist()):
        assert not y[b, n:].any(), "output frames past olens must be exactly 0"
    _, _, _, pre, D0 = G.restate(sd, cfg, inp, torch.float64, bf=True)
    relu_in, pool_in = G.in_band(pre, cfg["bands"])
    for i, m in relu_in.items():
        ndiff = int((D[f"relu{i}"] != D0[f"relu{i}"]).sum())
        print(f"relu{i}: {ndiff} of {m.numel()} differ, {int(m.sum())} in the band")
        assert float(m.double().mean()) <= 0.05
        assert torch.equal(D[f"relu{i}"][~m], D0[f"relu{i}"][~m]), f"relu{i} outside the band"
    for j, m in pool_in.items():
        ndiff = int((D[f"pool{j}"] != D0[f"pool{j}"]).sum())
        print(f"pool{j}: {ndiff} of {m.numel()} differ, {int(m.sum())} in the band")
        assert float(m.double().mean()) <= 0.20
        assert torch.equal(D[f"pool{j}"][~m], D0[f"pool{j}"][~m]), f"pool{j} outside the band"
    _check(y, ry, d["bf.err.y"], "y")
    for k, v in g.items():
        _check(v, rg[k], d[f"bf.err.grad.{k}"], "grad " + k)


def test_unsorted_lengths():
    """The rows permuted: the permuted outputs, the same parameter gradients (another summation
    order, so within the fixture tolerance, not bitwise).  The reference raises on this batch."""
    cfg, d, enc, inp = _fixture("vgg_rnn_tiny")
    perm = [1, 0]
    y, olens, g = _train_pass(enc, {k: v[perm].contiguous() for k, v in inp.items()})
    _check(y, d["out.y"][perm], d["err.y"], "y")
    assert olens.tolist() == d["out.olens"][perm].tolist()
    _check_grads(cfg, d, g)


def test_padding_beyond_the_longest_row():
    """Four more frames (of zeros), one more output frame: the lengths and the shape law hold and the
    added output frame is exactly 0.  VGG2L masks nothing, so outputs within the receptive field of
    the added frames change (an appended frame is not the image edge: conv1_1 gives relu(bias)
    there, not the zero padding conv1_2 saw in the fixture).  Output frame j reads conv1_1 outputs
    of the input frames 4j - 5 .. 4j + 8 only, so the shorter row (7 frames, 2 output frames) reads
    none of the added ones and is the fixture's."""
    cfg, d, enc, inp = _fixture("vgg_rnn_tiny")
    B, T, Fd = inp["xs_pad"].shape
    assert T % 4 == 1  # 13 -> 7 -> 4 frames; 17 -> 9 -> 5: the fixture's windows keep their pixels
    xs = torch.cat([inp["xs_pad"], torch.zeros(B, 4, Fd)], dim=1)
    To = inp["cot"].shape[1]
    cot = torch.cat([inp["cot"], torch.randn(B, 1, cfg["proj"], generator=torch.Generator().manual_seed(1))], dim=1)
    y, olens, g = _train_pass(enc, dict(xs_pad=xs, ilens=inp["ilens"], cot=cot))
    assert y.shape == (B, To + 1, cfg["proj"]) and olens.tolist() == d["out.olens"].tolist()
    assert not y[:, To:].any()
    short = int(np.argmin(cfg["ilens"]))
    _check(y[short, :To], d["out.y"][short], d["err.y"], "y of the shorter row")


# ------------------------------------------------------------------ the hybrid model
def hybrid_model():
    """ESPnetASRModel (encoder: vgg_rnn, decoder: rnn, ctc_weight 0.5) rebuilt from the fixture's seed
    on the CPU and checked against its recorded weight sums."""
    from espnet_amd.tasks.asr import build_model
    cfg, d = load("vgg_rnn_tiny")
    h = cfg["hyb"]
    V = h["vocab_size"]
    tok = ["<blank>", "<unk>"] + [f"t{i}" for i in range(V - 3)] + ["<sos/eos>"]
    torch.manual_seed(h["seed"])
    m = build_model(dict(token_list=tok, input_size=h["input_size"], encoder="vgg_rnn", encoder_conf=h["encoder_conf"],
                         decoder="rnn", decoder_conf=h["decoder_conf"], model_conf=h["model_conf"]))
    sd, sums = m.state_dict(), section(d, "hyb.wsum")
    assert list(sd) == list(sums), "state_dict layout differs from the reference's"
    for k, v in sums.items():
        np.testing.assert_allclose(sd[k].double().sum().item(), float(v), rtol=1e-12, atol=1e-12, err_msg=k)
    return cfg, d, m


def _hyb_setup(amp=False):
    from espnet_amd.optim.adam import ArenaAdam
    cfg, d, m = hybrid_model()
    m.prepare("cuda:0", amp=amp, seed=3)
    m.train()
    batch = {k: torch.from_numpy(v) for k, v in section(d, "hyb.in").items()}
    return cfg, d, m, ArenaAdam(m, lr=cfg["hyb"]["lr"]), batch


def _other_lengths(batch):
    """A batch of the same shape (the same maxima) with other lengths, rows no longer sorted."""
    b = {k: v.clone() for k, v in batch.items()}
    assert b["speech_lengths"].tolist() == [36, 25, 13] and b["text_lengths"].tolist() == [4, 3, 2]
    b["speech_lengths"] = torch.tensor([36, 9, 20])
    b["text_lengths"] = torch.tensor([4, 2, 3])
    b["text"][1, 2] = -1
    b["text"][2, 2] = b["text"][2, 1] % 8 + 2  # differs from its neighbour: no CTC repeat
    return b


KEYS = ("loss", "loss_att", "loss_ctc", "acc")


def test_four_step_trace_against_the_fixture():
    from espnet_amd.train.trainer import Trainer
    torch.cuda.set_device(0)
    cfg, d, m, opt, batch = _hyb_setup()
    h = cfg["hyb"]
    got = []
    for _ in range(h["steps"]):
        loss, stats, _, _ = Trainer.train_one_step(m, batch, opt, None, grad_clip=h["grad_clip"])
        got.append([float(stats[k]) for k in KEYS])
    torch.cuda.synchronize()
    for j, k in enumerate(KEYS):
        _check([e[j] for e in got], d["hyb." + k], d["err.hyb." + k], "hybrid " + k)


@pytest.mark.parametrize("amp", [False, True], ids=["f32", "bf16"])
def test_captured_step_equals_eager_over_changing_lengths(amp):
    from espnet_amd.train.graph import CapturedTrainStep
    from espnet_amd.train.trainer import Trainer
    torch.cuda.set_device(0)
    cfg, d, m1, o1, batch = _hyb_setup(amp)
    h = cfg["hyb"]
    seq = [batch, _other_lengths(batch), batch, _other_lengths(batch)]
    eager = []
    for b in seq:
        loss, stats, _, _ = Trainer.train_one_step(m1, b, o1, None, grad_clip=h["grad_clip"])
        eager.append([float(stats[k]) for k in KEYS])
    torch.cuda.synchronize()
    assert eager[0] != eager[1]
    cfg, d, m2, o2, batch = _hyb_setup(amp)
    run = CapturedTrainStep(m2, o2, None, grad_clip=h["grad_clip"], warmup=1)
    graph = []
    for b in seq:
        loss, stats, _, _ = run(b)
        graph.append([float(stats[k]) for k in KEYS])
    torch.cuda.synchronize()
    assert len(run.graphs) == 1 and run.mode == "graph"
    assert eager == graph
    for (k, p1), p2 in zip(m1.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(p1, p2), k


@pytest.mark.parametrize("case", [0, 1])
def test_beam_search_returns_the_references_hypotheses(case):
    from espnet_amd.asr.inference import attention_beam_search
    cfg, d, m = hybrid_model()
    m.prepare("cuda:0", amp=False)
    m.eval()
    h = cfg["hyb"]
    beam, cw = h["beam_cases"][case]
    batch = {k: torch.from_numpy(v) for k, v in section(d, "hyb.in").items()}
    with torch.no_grad():  # encode() and the greedy CTC path
        enc, lens = m.encode(batch["speech"], batch["speech_lengths"])
        assert enc.shape[:2] == (3, 9) and lens.tolist() == [9, 7, 4]
        assert m.ctc.argmax(enc).shape == (3, 9)
    res = attention_beam_search(m, batch["speech"], batch["speech_lengths"], beam, ctc_weight=cw)
    meta = [e for e in h["nbest"] if e["case"] == case]
    assert len(res) == len(meta)
    for e, nbest in zip(meta, res):
        assert len(nbest) == e["n"]
        for r, hyp in enumerate(nbest):
            key = f"hyb.beam.c{case}.u{e['utt']}.h{r}"
            assert [int(t) for t in hyp.yseq] == d[key + ".yseq"].tolist(), key
            np.testing.assert_allclose(float(hyp.score), float(d[key + ".score"]), rtol=1e-4, atol=1e-4, err_msg=key)


def test_checkpoint_load_refreshes_the_conv_packs():
    cfg, d, m = hybrid_model()
    ref_sd = {k: (v + 0.25 if v.is_floating_point() else v.clone()) for k, v in m.state_dict().items()}
    m.prepare("cuda:0", amp=False)
    m.load_state_dict(ref_sd)
    torch.cuda.synchronize()
    vgg = m.encoder.enc[0]
    for name in ("conv1_2", "conv2_1", "conv2_2"):
        w = getattr(vgg, name).weight.detach()
        wp, wd = vgg._packs[name]
        assert torch.equal(wp, w.permute(0, 2, 3, 1).reshape(wp.shape))  # (Co, 9, Ci)
        assert torch.equal(wd, w.permute(1, 2, 3, 0).reshape(wd.shape))  # (Ci, 9, Co)
