"""RNNDecoder (decoder: rnn) on the GPU against the reference's fixtures
(tests/capture_rnn_decoder_goldens.py): logits, per-step attention weights, every parameter
gradient and the hs_pad gradient of the three fixtures in f32 and bf16; dropout against the float64
restatement on the kernels' own masks; the scorer trace, batch_score, the beam search and the
four-step hybrid training trace (eager and through the captured-step runner); checkpoints.

Tolerance (tests/lstm_train_goldens.py tolerance): an array passes within 4 x its
recorded err (max |f32 - f64| of the reference itself; bf16: of the bf16 restatement) or 4 f32 ulps
at the array's largest magnitude, whichever is larger.  grad att_list.0.gvec.bias is an exact-zero
sum (sum_t de[t]): 4 x err or 4 ulps at the recorded sum |de[t]|.  Attention weights at padded
frames and logits rows past ys_in_lens must be exactly 0.
"""
import numpy as np
import pytest
import torch

import rnn_decoder_goldens as G
from goldens import load, perturb_norms, section
from lstm_train_goldens import ulp32

pytestmark = pytest.mark.gpu
MARGIN = G.MARGIN


def _check(got, ref, err, what, mag=None):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    tol = G.tolerance(ref, err, MARGIN) if mag is None else max(MARGIN * float(err), 4 * ulp32(float(mag)))
    worst = float(np.abs(got - ref).max()) if ref.size else 0.0
    print(f"{what}: max |err| {worst:.3e}, tolerance {tol:.3e}")
    assert worst <= tol, f"{what}: max |err| {worst:.3e} > {tol:.3e}"


def _train_pass(dec, inp, seed=0):
    """forward + backward under the fixture's cotangent -> (logits, att_w, grads) on the CPU."""
    dec.train()
    dec._b.arena.zero_grad()
    hs = inp["hs_pad"].cuda().requires_grad_(True)
    logits, lens = dec(hs, inp["hlens"].cuda(), inp["ys_in_pad"].cuda(), inp["ys_in_lens"].cuda(), seed=seed)
    logits.backward(inp["cot"].cuda())
    torch.cuda.synchronize()
    g = {k: p.grad.detach().cpu().clone() for k, p in dec.named_parameters()}
    g["hs_pad"] = hs.grad.cpu()
    return logits.detach().cpu(), dec._last_att_w.cpu(), g


@pytest.mark.parametrize("amp", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", G.NAMES)
def test_fixture_parity(name, amp):
    from espnet_amd.asr.decoder.rnn_decoder import RNNDecoder
    cfg, d, dec, inp = G.build(name, RNNDecoder)
    G.prepare_decoder(dec, amp)
    logits, att_w, g = _train_pass(dec, inp)
    pre, out = ("bf.", "bf.") if amp else ("", "out.")
    _check(logits, d[out + "logits"], d[pre + "err.logits"], "logits")
    _check(att_w, d[out + "att_w"], d[pre + "err.att_w"], "att_w")
    B, L = inp["ys_in_pad"].shape
    T = inp["hs_pad"].shape[1]
    for b in range(B):
        assert not logits[b, int(inp["ys_in_lens"][b]):].any(), "logits rows past ys_in_lens must be exactly 0"
        assert not att_w[:, b, int(inp["hlens"][b]):].any(), "attention weights at padded frames must be exactly 0"
        if int(inp["hlens"][b]) < T:
            assert not g["hs_pad"][b, int(inp["hlens"][b]):].any()
    for k, v in g.items():
        err = d[f"{pre}err.grad.{k}"]
        mag = d["mag.grad." + k] if k in G.ZERO_SUM_GRADS else None
        if name in G.STORED:
            _check(v, d[f"{pre}grad.{k}"], err, "grad " + k, mag)
        else:
            s = cfg["gstride"][k]
            _check(v.reshape(-1)[::s], d[f"{pre}gsamp.{k}"], err, "grad sample " + k, mag)
            ref_norm = float(d[f"{pre}gnorm.{k}"])
            n = v.numel()
            # the norm of n elements each within the array's tolerance
            tol = G.tolerance(d[f"{pre}gsamp.{k}"], err, MARGIN) if mag is None else max(MARGIN * float(err),
                                                                                           4 * ulp32(float(mag)))
            assert abs(float(v.double().norm()) - ref_norm) <= tol * n ** 0.5, k


def _masks(dec, seed, L, B, p):
    """The dropout factors (0 or 1 / (1 - p)) the kernels draw for a forward with `seed`."""
    from espnet_amd import hip_ops as ops
    H = dec.dunits
    seeds = dec.dropout_seeds(seed, L)

    def draw(rows, s):
        y = torch.empty(rows, H, device="cuda")
        ops.scale_dropout(torch.ones(rows, H, device="cuda"), y, p=p, seed=s)
        return y.cpu()

    m = {"emb": draw(L * B, seeds["emb"]).view(L, B, H), "out": draw(L * B, seeds["out"]).view(L, B, H),
         "query": torch.stack([draw(B, seeds["query"][i]) for i in range(L)])}
    for l in range(1, dec.dlayers):
        m[f"layer{l}"] = draw(L * B, seeds[f"layer{l}"]).view(L, B, H)
    return m


def test_dropout_against_the_restatement_on_the_kernels_masks():
    from espnet_amd.asr.decoder.rnn_decoder import RNNDecoder
    p, seed = 0.3, 12345
    cfg, d, dec, inp = G.build("rnn_dec_tiny", RNNDecoder, dropout=p)
    sd = {k: v.clone() for k, v in dec.state_dict().items()}
    G.prepare_decoder(dec)
    logits, att_w, g = _train_pass(dec, inp, seed=seed)
    B, L = inp["ys_in_pad"].shape
    masks = _masks(dec, seed, L, B, p)
    for k, v in masks.items():
        kept = float((v != 0).double().mean())
        assert abs(kept - (1 - p)) < 0.1, (k, kept)
    r64 = G.restate(sd, inp, torch.float64, masks=masks)
    r32 = G.restate(sd, inp, torch.float32, masks=masks)
    _check(logits, r64[0], float((r32[0].double() - r64[0]).abs().max()), "logits")
    _check(att_w, r64[1], float((r32[1].double() - r64[1]).abs().max()), "att_w")
    for k, v in g.items():
        err = float((r32[2][k].double() - r64[2][k]).abs().max())
        _check(v, r64[2][k], err, "grad " + k, r64[3] if k in G.ZERO_SUM_GRADS else None)
    # eval mode: no dropout, the fixture's logits
    dec.eval()
    with torch.no_grad():
        lg, _ = dec(inp["hs_pad"].cuda(), inp["hlens"].cuda(), inp["ys_in_pad"].cuda(), inp["ys_in_lens"].cuda(), seed=seed)
    _check(lg.cpu(), d["out.logits"], d["err.logits"], "eval logits")


def test_query_and_output_masks_of_one_layer_differ():
    """With one layer dropout_dec[0] is both the query's and the output's module: two calls, two
    masks, on the same z0."""
    from espnet_amd.asr.decoder.rnn_decoder import RNNDecoder
    cfg, d, dec, inp = G.build("rnn_dec_one", RNNDecoder, dropout=0.5)
    G.prepare_decoder(dec)
    L, B = 4, 3
    m = _masks(dec, 7, L, B, 0.5)
    for i in range(1, L):  # the query of step i and the output of step i - 1 drop the same z0_{i-1}
        assert not torch.equal(m["query"][i], m["out"][i - 1])
        assert not torch.equal(m["query"][i], m["query"][i - 1])
    assert not torch.equal(m["emb"], m["out"])


def _scorer(amp=False):
    from espnet_amd.asr.decoder.rnn_decoder import RNNDecoder
    cfg, d, dec, inp = G.build("rnn_dec_tiny", RNNDecoder)
    G.prepare_decoder(dec, amp)
    dec.eval()
    return cfg, d, dec, inp


def test_scorer_trace_and_batch_score():
    cfg, d, dec, inp = _scorer()
    x = inp["hs_pad"][0, :int(inp["hlens"][0])].cuda()
    ys = inp["ys_in_pad"][0].cuda()
    st = dec.init_state(x)
    assert set(st) == {"c_prev", "z_prev", "a_prev", "workspace"} and st["a_prev"] is None
    assert len(st["z_prev"]) == dec.dlayers and st["z_prev"][0].shape == (1, dec.dunits)
    states, lps = [st], []
    for i in range(4):
        logp, st = dec.score(ys[:i + 1], st, x)
        assert logp.shape == (cfg["V"],) and st["a_prev"].shape == (1, x.shape[0])
        _check(logp.cpu(), d["sc.logp"][i], d["err.sc.logp"], f"score {i} logp")
        _check(st["a_prev"][0].cpu(), d["sc.a_prev"][i], d["err.sc.a_prev"], f"score {i} a_prev")
        states.append(st)
        lps.append(logp)
    # n copies of one hypothesis as the rows of one step
    n = 3
    lp, new = dec.batch_score(ys[:3].unsqueeze(0).expand(n, 3), [states[2]] * n, x.unsqueeze(0).expand(n, *x.shape))
    assert lp.shape == (n, cfg["V"]) and len(new) == n
    for r in range(n):
        _check(lp[r].cpu(), lps[2].cpu(), d["err.sc.logp"], f"copy {r}")
        _check(new[r]["a_prev"][0].cpu(), states[3]["a_prev"][0].cpu(), d["err.sc.a_prev"], f"copy {r} a_prev")
        _check(new[r]["z_prev"][-1].cpu(), states[3]["z_prev"][-1].cpu(), d["err.sc.logp"], f"copy {r} z")
    # different hypotheses (the initial state among them) in one step
    pref = torch.full((3, 4), cfg["V"] - 1, dtype=torch.long, device="cuda")
    pref[0, -1:], pref[1, -2:], pref[2] = ys[:1], ys[:2], ys[:4]
    lp, new = dec.batch_score(pref, [states[0], states[1], states[3]], x.unsqueeze(0).expand(3, *x.shape))
    for r, i in enumerate((0, 1, 3)):
        _check(lp[r].cpu(), d["sc.logp"][i], d["err.sc.logp"], f"mixed row {r}")
        _check(new[r]["a_prev"][0].cpu(), d["sc.a_prev"][i], d["err.sc.a_prev"], f"mixed row {r} a_prev")


def test_batch_score_checks_whose_memory_is_cached():
    """The mlp_enc projection kept by init_state belongs to ONE utterance: a step over another
    memory (no init_state in between) must not use it."""
    cfg, d, dec, inp = _scorer()
    x0 = inp["hs_pad"][0, :7].cuda()
    x1 = inp["hs_pad"][1, :7].cuda().contiguous()  # same shape, other content
    ys = inp["ys_in_pad"][0, :1].cuda()
    want, _ = dec.score(ys, dec.init_state(x1), x1)
    st0 = dec.init_state(x0)
    got, _ = dec.batch_score(ys.unsqueeze(0), [st0], x1.unsqueeze(0))
    assert torch.equal(got[0], want)
    x1.mul_(0.5)  # the same storage with new content
    want2, _ = dec.score(ys, dec.init_state(x1.clone()), x1.clone())
    got2, _ = dec.batch_score(ys.unsqueeze(0), [st0], x1.unsqueeze(0))
    assert torch.equal(got2[0], want2) and not torch.equal(got2[0], got[0])


def test_scorer_bf16_runs_close_to_f32():
    cfg, d, dec, inp = _scorer(amp=True)
    x = inp["hs_pad"][0, :7].cuda()
    ys = inp["ys_in_pad"][0].cuda()
    st = dec.init_state(x)
    for i in range(3):
        logp, st = dec.score(ys[:i + 1], st, x)
        # bf16 operands: 2^-8 relative per product, a few products deep
        assert float((logp.cpu().double() - torch.from_numpy(d["sc.logp"][i]).double()).abs().max()) < 0.05


# ------------------------------------------------------------------ the hybrid model
def hybrid_model():
    """ESPnetASRModel (tiny_hybrid encoder, decoder: rnn, ctc_weight 0.5) rebuilt from the fixture's
    seed on the CPU and checked against its recorded weight sums."""
    from espnet_amd.tasks.asr import build_model
    cfg, d = load("rnn_dec_tiny")
    h = cfg["hyb"]
    V = h["vocab_size"]
    tok = ["<blank>", "<unk>"] + [f"t{i}" for i in range(V - 3)] + ["<sos/eos>"]
    torch.manual_seed(h["seed"])
    m = build_model(dict(token_list=tok, input_size=h["input_size"], encoder="conformer", encoder_conf=h["encoder_conf"],
                         decoder="rnn", decoder_conf=h["decoder_conf"], model_conf=h["model_conf"]))
    perturb_norms(m, torch.Generator().manual_seed(1000 + h["seed"]))
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
    h = cfg["hyb"]
    batch = {k: torch.from_numpy(v) for k, v in section(d, "hyb.in").items()}
    return cfg, d, m, ArenaAdam(m, lr=h["lr"]), batch


def test_four_step_trace_eager_and_captured():
    from espnet_amd.train.graph import CapturedTrainStep
    from espnet_amd.train.trainer import Trainer
    torch.cuda.set_device(0)
    cfg, d, m1, o1, batch = _hyb_setup()
    h = cfg["hyb"]
    keys = ("loss", "loss_att", "loss_ctc", "acc")
    eager = []
    for _ in range(h["steps"]):
        loss, stats, _, _ = Trainer.train_one_step(m1, batch, o1, None, grad_clip=h["grad_clip"])
        eager.append([float(stats[k]) for k in keys])
    torch.cuda.synchronize()
    for j, k in enumerate(keys):
        _check([e[j] for e in eager], d["hyb." + k], d["err.hyb." + k], "hybrid " + k)
    cfg, d, m2, o2, batch = _hyb_setup()
    run = CapturedTrainStep(m2, o2, None, grad_clip=h["grad_clip"], warmup=1)
    graph = []
    for _ in range(h["steps"]):
        loss, stats, _, _ = run(batch)
        graph.append([float(stats[k]) for k in keys])
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
    h = cfg["hyb"]
    beam, cw = h["beam_cases"][case]
    batch = {k: torch.from_numpy(v) for k, v in section(d, "hyb.in").items()}
    res = attention_beam_search(m, batch["speech"], batch["speech_lengths"], beam, ctc_weight=cw)
    meta = [e for e in h["nbest"] if e["case"] == case]
    assert len(res) == len(meta)
    for e, nbest in zip(meta, res):
        assert len(nbest) == e["n"]
        for r, hyp in enumerate(nbest):
            key = f"hyb.beam.c{case}.u{e['utt']}.h{r}"
            assert [int(t) for t in hyp.yseq] == d[key + ".yseq"].tolist(), key
            np.testing.assert_allclose(float(hyp.score), float(d[key + ".score"]), rtol=1e-4, atol=1e-4, err_msg=key)


def test_reference_checkpoint_round_trip():
    """A reference-layout state_dict loads into the prepared model and comes back bit-equal, in the
    same key order; the LSTM kernels' packs and the cached memory follow the load."""
    from espnet_amd.lm.lstm_pack import pack_lstm_hh
    cfg, d, m = hybrid_model()
    # a checkpoint with other weights
    ref_sd = {k: (v + 0.25 if v.is_floating_point() else v.clone()) for k, v in m.state_dict().items()}
    m.prepare("cuda:0", amp=False)
    dec = m.decoder
    dec._mem = ("stale",)
    m.load_state_dict(ref_sd)
    torch.cuda.synchronize()
    back = m.state_dict()
    assert list(back) == list(ref_sd)
    for k, v in ref_sd.items():
        assert torch.equal(back[k].cpu(), v), k
    for l, cell in enumerate(dec.decoder):
        assert torch.equal(dec._layers[l].hh.fwd, pack_lstm_hh(cell.weight_hh, torch.float32)), l
    assert dec._mem is None
    dsd = {k[len("decoder."):]: v for k, v in ref_sd.items() if k.startswith("decoder.")}
    assert list(dsd) == list(dec.state_dict())
    dec.load_state_dict({k: v - 0.25 for k, v in dsd.items()})  # a submodule load refreshes too
    torch.cuda.synchronize()
    assert torch.equal(dec._layers[0].hh.fwd, pack_lstm_hh(dec.decoder[0].weight_hh, torch.float32))
