"""RNNEncoder (encoder: rnn) on the GPU against the reference's fixtures
(tests/capture_rnn_encoder_goldens.py): output, output lengths, every parameter gradient and the
input gradient of the four fixtures in f32 and bf16 (junk in the padded input frames); unsorted
lengths; padding beyond the longest row; dropout against the float64 restatement on the kernels'
own masks (RNNP's in eval mode too); the hybrid model with decoder: rnn: the four-step training
trace, eager against the captured-step runner on batches of one shape and different lengths, and
the beam search.

Tolerance (tests/lstm_train_goldens.py tolerance): an array passes within 4 x its recorded err
(max |f32 - f64| of the reference itself; bf16: of the bf16 restatement, which includes what the
bf16 roundings that sit on a rounding boundary cost, see the capture script) or 4 f32 ulps at the
array's largest magnitude, whichever is larger.  Output frames past the output length must be
exactly 0, and so must the input gradient of the padded frames.
"""
import numpy as np
import pytest
import torch

import rnn_encoder_goldens as G
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


def _train_pass(enc, inp, seed=0, train=True):
    """forward + backward under the cotangent -> (y, olens, grads) on the CPU."""
    enc.train(train)
    for p in enc.parameters():
        p.grad.zero_()
    xs = inp["xs_pad"].cuda().requires_grad_(True)
    y, olens, _ = enc(xs, inp["ilens"].cuda(), seed=seed)
    y.backward(inp["cot"].cuda())
    torch.cuda.synchronize()
    g = {k: p.grad.detach().cpu().clone() for k, p in enc.named_parameters()}
    g["xs_pad"] = xs.grad.cpu()
    return y.detach().cpu(), olens.cpu(), g


def _fixture(name, amp=False, dropout=0.0):
    from espnet_amd.asr.encoder.rnn_encoder import RNNEncoder
    cfg, d, enc, inp = G.build(name, RNNEncoder, dropout=dropout)
    sd = {k: v.clone() for k, v in enc.state_dict().items()}
    G.prepare_encoder(enc, amp)
    return cfg, d, enc, inp, sd


@pytest.mark.parametrize("amp", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", G.NAMES)
def test_fixture_parity(name, amp):
    cfg, d, enc, inp, _ = _fixture(name, amp)
    y, olens, g = _train_pass(enc, inp)
    pre, out = ("bf.", "bf.") if amp else ("", "out.")
    _check(y, d[out + "y"], d[pre + "err.y"], "y")
    assert olens.tolist() == d["out.olens"].tolist()
    for b, n in enumerate(olens.tolist()):
        assert not y[b, n:].any(), "output frames past olens must be exactly 0"
        assert not g["xs_pad"][b, int(inp["ilens"][b]):].any(), "the padded input frames receive no gradient"
    for k, v in g.items():
        err = d[f"{pre}err.grad.{k}"]
        if name in G.STORED:
            _check(v, d[f"{pre}grad.{k}"], err, "grad " + k)
        else:
            s = cfg["gstride"][k]
            _check(v.reshape(-1)[::s], d[f"{pre}gsamp.{k}"], err, "grad sample " + k)
            tol = G.tolerance(d[f"{pre}gsamp.{k}"], err, MARGIN)
            # the norm of n elements each within the array's tolerance
            assert abs(float(v.double().norm()) - float(d[f"{pre}gnorm.{k}"])) <= tol * v.numel() ** 0.5, k


def test_unsorted_lengths():
    """The rows permuted: the permuted outputs, the same parameter gradients (another summation
    order, so within the fixture tolerance, not bitwise).  The reference raises on this batch."""
    cfg, d, enc, inp, _ = _fixture("rnn_enc_tiny")
    perm = [2, 0, 1]
    pin = {k: v[perm].contiguous() for k, v in inp.items()}
    y, olens, g = _train_pass(enc, pin)
    _check(y, d["out.y"][perm], d["err.y"], "y")
    assert olens.tolist() == d["out.olens"][perm].tolist()
    for k, v in g.items():
        ref = d[f"grad.{k}"]
        _check(v, ref[perm] if k == "xs_pad" else ref, d[f"err.grad.{k}"], "grad " + k)


def test_padding_beyond_the_longest_row():
    """3 more frames of junk: the same valid outputs and gradients, zeros beyond."""
    cfg, d, enc, inp, _ = _fixture("rnn_enc_tiny")
    B, T, F = inp["xs_pad"].shape
    T2 = T + 3
    gen = torch.Generator().manual_seed(1)
    To, To2 = inp["cot"].shape[1], G.out_frames(cfg, T2)
    xs = torch.cat([inp["xs_pad"], torch.randn(B, 3, F, generator=gen)], dim=1)
    cot = torch.cat([inp["cot"], torch.randn(B, To2 - To, cfg["proj"], generator=gen)], dim=1)
    y, olens, g = _train_pass(enc, dict(xs_pad=xs, ilens=inp["ilens"], cot=cot))
    assert y.shape == (B, To2, cfg["proj"]) and olens.tolist() == d["out.olens"].tolist()
    _check(y[:, :To], d["out.y"], d["err.y"], "y")
    assert not y[:, To:].any() and not g["xs_pad"][:, T:].any()
    for k, v in g.items():
        _check(v[:, :T] if k == "xs_pad" else v, d[f"grad.{k}"], d[f"err.grad.{k}"], "grad " + k)


def _draw(rows, cols, p, seed):
    from espnet_amd import hip_ops as ops
    y = torch.empty(rows, cols, device="cuda")
    ops.scale_dropout(torch.ones(rows, cols, device="cuda"), y, p=p, seed=seed)
    return y.cpu()


def _masks(enc, cfg, seed, T, B, p, train):
    """The dropout factors (0 or 1 / (1 - p)) the kernels draw for a forward with `seed`."""
    m, seeds = {}, enc.enc[0].dropout_seeds(seed)
    if cfg["use_projection"]:
        for i, sub in enumerate(G.sub_law(cfg)[:-1]):
            T = -(-T // sub)
            m[f"proj{i}"] = _draw(T * B, cfg["proj"], p, seeds[i])
    elif train:
        width = cfg["H"] * (2 if cfg["bidirectional"] else 1)
        for k in range(cfg["layers"] - 1):
            m[f"layer{k}"] = _draw(T * B, width, p, seeds[k])
    return m


@pytest.mark.parametrize("name,train", [("rnn_enc_tiny", True), ("rnn_enc_tiny", False), ("rnn_enc_noproj", True),
                                        ("rnn_enc_noproj", False)])
def test_dropout_against_the_restatement_on_the_kernels_masks(name, train):
    """RNNP's F.dropout has no `training=`: its masks apply in eval mode too.  nn.LSTM's inter-layer
    dropout (RNN) applies in training only."""
    p, seed = 0.3, 12345
    cfg, d, enc, inp, sd = _fixture(name, dropout=p)
    y, olens, g = _train_pass(enc, inp, seed=seed, train=train)
    B, T, _ = inp["xs_pad"].shape
    masks = _masks(enc, cfg, seed, T, B, p, train)
    assert bool(masks) == (cfg["use_projection"] or train)
    for k, v in masks.items():
        kept = float((v != 0).double().mean())
        assert abs(kept - (1 - p)) < 0.15, (k, kept)
    r64 = G.restate(sd, cfg, inp, torch.float64, masks=masks)
    r32 = G.restate(sd, cfg, inp, torch.float32, masks=masks)
    _check(y, r64[0], float((r32[0].double() - r64[0]).abs().max()), "y")
    for k, v in g.items():
        _check(v, r64[2][k], float((r32[2][k].double() - r64[2][k]).abs().max()), "grad " + k)
    if not masks:  # no dropout drawn: the fixture's output
        _check(y, d["out.y"], d["err.y"], "y against the fixture")


# ------------------------------------------------------------------ the hybrid model
def hybrid_model():
    """ESPnetASRModel (encoder: rnn, decoder: rnn, ctc_weight 0.5) rebuilt from the fixture's seed on
    the CPU and checked against its recorded weight sums."""
    from espnet_amd.tasks.asr import build_model
    cfg, d = load("rnn_enc_tiny")
    h = cfg["hyb"]
    V = h["vocab_size"]
    tok = ["<blank>", "<unk>"] + [f"t{i}" for i in range(V - 3)] + ["<sos/eos>"]
    torch.manual_seed(h["seed"])
    m = build_model(dict(token_list=tok, input_size=h["input_size"], encoder="rnn", encoder_conf=h["encoder_conf"],
                         decoder="rnn", decoder_conf=h["decoder_conf"], model_conf=h["model_conf"]))
    sd, sums = m.state_dict(), section(d, "hyb.wsum")
    assert list(sd) == list(sums), "state_dict layout differs from the reference's"
    for k, v in sums.items():
        np.testing.assert_allclose(sd[k].double().sum().item(), float(v), rtol=1e-12, atol=1e-12, err_msg=k)
    return cfg, d, m


def _hyb_setup():
    from espnet_amd.optim.adam import ArenaAdam
    cfg, d, m = hybrid_model()
    m.prepare("cuda:0", amp=False, seed=3)
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


def test_captured_step_equals_eager_over_changing_lengths():
    from espnet_amd.train.graph import CapturedTrainStep
    from espnet_amd.train.trainer import Trainer
    torch.cuda.set_device(0)
    cfg, d, m1, o1, batch = _hyb_setup()
    h = cfg["hyb"]
    seq = [batch, _other_lengths(batch), batch, _other_lengths(batch)]
    eager = []
    for b in seq:
        loss, stats, _, _ = Trainer.train_one_step(m1, b, o1, None, grad_clip=h["grad_clip"])
        eager.append([float(stats[k]) for k in KEYS])
    torch.cuda.synchronize()
    assert eager[0] != eager[1]
    cfg, d, m2, o2, batch = _hyb_setup()
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


def test_checkpoint_load_refreshes_the_packs():
    from espnet_amd.lm.lstm_pack import pack_lstm_hh
    cfg, d, m = hybrid_model()
    ref_sd = {k: (v + 0.25 if v.is_floating_point() else v.clone()) for k, v in m.state_dict().items()}
    m.prepare("cuda:0", amp=False)
    m.load_state_dict(ref_sd)
    torch.cuda.synchronize()
    rnnp = m.encoder.enc[0]
    assert len(rnnp.lstm_layers()) == 2 * rnnp.elayers
    for i, dirs in enumerate(rnnp._layers):
        rnn = getattr(rnnp, f"birnn{i}")
        assert torch.equal(dirs[0].hh.fwd, pack_lstm_hh(rnn.weight_hh_l0, torch.float32))
        assert torch.equal(dirs[1].hh.fwd, pack_lstm_hh(rnn.weight_hh_l0_reverse, torch.float32))
