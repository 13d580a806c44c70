"""SequentialRNNLM training path under ESPnetLanguageModel against the reference's fixtures
(tests/capture_lstm_train_goldens.py): tiny (unit 26 x 2, ragged B = 5 with id 0 inside a
sentence), nhid != unit (24 / 40 x 3, B = 1) and 650 x 2 (ragged B = 3).

f32: loss, nll, ntokens, every parameter gradient and the 5-step Adam loss trajectory, each
within tolerance(ref, err) of tests/lstm_train_goldens.py: MARGIN (4) x the reference's own
f32-vs-float64 error recorded for that array, or 4 float32 ulps at the array's magnitude.
bf16 (amp): loss, nll and every gradient, element-wise, against the float64 restatement of the
step with the operands of every matrix product, forward and backward, rounded to bf16 where the
path rounds them (restate_bf16), by the same rule on the error recorded for that restatement
(the same restatement run in f32 against float64).
Dropout 0.5: loss and gradients against a float64 restatement that uses the masks the kernels
drew (recovered by running ea_scale_dropout on ones with the same seeds), tolerance 4 x the
deviation of that restatement run in f32, or 4 ulps.
"""
import numpy as np
import pytest
import torch

from goldens import section
from lstm_train_goldens import NAMES, STORED, batch, build, restate_train, tolerance

pytestmark = pytest.mark.gpu

_RUNS = {}


def _prepared(name, amp=False, dropout_rate=0.0, seed=0):
    from espnet_amd.lm import ESPnetLanguageModel, SequentialRNNLM
    cfg, d, model = build(name, SequentialRNNLM, ESPnetLanguageModel, dropout_rate)
    model.prepare("cuda", amp=amp, seed=seed)
    model.train()
    return cfg, d, model


def _one_pass(model, text, lens):
    model.arena.zero_grad()
    loss, stats, ntok = model(text, lens)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.lm.named_parameters()}
    nll, _ = model.nll(text, lens)  # (training mode with autograd: the training forward again)
    return loss.detach().cpu(), nll.cpu(), int(ntok), grads, stats


def _run(name, amp):
    if (name, amp) not in _RUNS:
        cfg, d, model = _prepared(name, amp)
        _RUNS[(name, amp)] = (cfg, d) + _one_pass(model, *batch(d))
    return _RUNS[(name, amp)]


def _check(got, ref, err, margin, what):
    tol = tolerance(ref, err, margin)
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.size == ref.size, f"{what}: {got.shape} vs {ref.shape}"
    dev = float(np.abs(got.reshape(-1) - ref.reshape(-1)).max())  # (the reference's loss is 1-d)
    print(f"{what}: max |dev| {dev:.3e}, tolerance {tol:.3e} (reference's own error {float(err):.3e})")
    assert dev <= tol, f"{what}: {dev:.3e} > {tol:.3e}"


@pytest.mark.parametrize("name", NAMES)
def test_loss_nll_ntokens_f32(name):
    cfg, d, loss, nll, ntok, _, stats = _run(name, False)
    assert ntok == int(d["out.ntokens"]) == int(d["in.text_lengths"].sum() + len(d["in.text_lengths"]))
    assert tuple(nll.shape) == d["out.nll"].shape
    _check(loss.numpy(), d["out.loss"], d["err.loss"], cfg["margin"], "loss")
    _check(nll.numpy(), d["out.nll"], d["err.nll"], cfg["margin"], "nll")
    assert float(stats["loss"]) == float(loss)
    lens = d["in.text_lengths"]
    for i, n in enumerate(lens):  # masked by length
        assert not nll[i, n + 1:].any() and bool((nll[i, :n + 1] > 0).all())


@pytest.mark.parametrize("name", NAMES)
def test_gradients_f32(name):
    cfg, d, _, _, _, grads, _ = _run(name, False)
    errs = section(d, "err.grad")
    assert set(grads) == set(errs)
    for k, g in grads.items():
        if name in STORED:
            _check(g.numpy(), d[f"grad.{k}"], errs[k], cfg["margin"], f"grad {k}")
        else:
            s = cfg["gstride"][k]
            _check(g.reshape(-1)[::s].numpy(), d[f"gsamp.{k}"], errs[k], cfg["margin"], f"grad sample {k}")
            np.testing.assert_allclose(float(g.double().norm()), float(d[f"gnorm.{k}"]), rtol=1e-5)
    assert not grads["encoder.weight"][0].any(), "the ignore_id row of the embedding received a gradient"
    assert grads["encoder.weight"][1:].any()


@pytest.mark.parametrize("name", NAMES)
def test_loss_nll_gradients_bf16(name):
    cfg, d, loss, nll, ntok, grads, _ = _run(name, True)
    assert ntok == int(d["out.ntokens"])
    _check(loss.numpy(), d["bf.loss"], d["bf.err.loss"], cfg["margin"], "bf16 loss")
    _check(nll.numpy(), d["bf.nll"], d["bf.err.nll"], cfg["margin"], "bf16 nll")
    errs = section(d, "bf.err.grad")
    assert set(grads) == set(errs)
    failed = []
    for k, g in grads.items():
        if name in STORED:
            got, ref = g.numpy(), d[f"bf.grad.{k}"]
        else:
            got, ref = g.reshape(-1)[::cfg["gstride"][k]].numpy(), d[f"bf.gsamp.{k}"]
        try:
            _check(got, ref, errs[k], cfg["margin"], f"bf16 grad {k}")
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)
    assert not grads["encoder.weight"][0].any()


@pytest.mark.parametrize("name", NAMES)
def test_adam_trajectory(name):
    from espnet_amd.optim.adam import ArenaAdam
    from espnet_amd.train.trainer import Trainer
    cfg, d, model = _prepared(name)
    a = cfg["adam"]
    opt = ArenaAdam(model, lr=a["lr"])
    text, lens = batch(d)
    b = {"text": text.cuda(), "text_lengths": lens.cuda()}
    losses = []
    for _ in range(a["steps"]):
        loss, _, _, _ = Trainer.train_one_step(model, b, opt, None, grad_clip=a["grad_clip"])
        losses.append(loss)
    got = torch.stack(losses).cpu().numpy()
    assert got[-1] < got[0]
    _check(got, d["adam.losses"], d["err.adam"], cfg["margin"], "Adam losses")


def _masks(model, text, lens, nstep, p, p_rnn):
    """The keep-masks of training forward `nstep`: ea_scale_dropout on ones, same seeds."""
    from espnet_amd import hip_ops as ops
    lm = model.lm
    T, B = int(lens.max()) + 1, text.shape[0]
    seeds = lm.dropout_seeds(nstep)
    out, ps = {}, {}
    for key, seed in seeds.items():
        width = lm.ninp if key == "embed" else lm.nhid
        pk = p_rnn if key.startswith("rnn") else p
        ones = torch.ones(T * B, width, device="cuda")
        y = torch.empty_like(ones)
        ops.scale_dropout(ones, y, p=pk, seed=seed)
        out[key], ps[key] = (y > 0).cpu(), pk
    return out, ps


def test_dropout_against_restatement_with_the_kernels_masks():
    name, p = "lstm_train_tiny", 0.5
    cfg, d, model = _prepared(name, dropout_rate=p, seed=7)
    text, lens = batch(d)
    sd = {k: v.detach().cpu().clone() for k, v in model.lm.state_dict().items()}
    masks, ps = _masks(model, text, lens, 0, p, p)
    for m in masks.values():
        assert 0.3 < float(m.float().mean()) < 0.7
    loss, nll, _, grads, _ = _one_pass(model, text, lens)
    V = cfg["lm_conf"]["vocab_size"]
    l64, _, g64 = restate_train(sd, text, lens, V, masks, ps, torch.float64)
    l32, _, g32 = restate_train(sd, text, lens, V, masks, ps, torch.float32)
    _check(loss.numpy(), l64.numpy(), float((l32.double() - l64).abs()), 4, "loss with dropout")
    for k, g in grads.items():
        _check(g.numpy(), g64[k].numpy(), float((g32[k].double() - g64[k]).abs().max()), 4, f"grad {k} with dropout")
    # the second forward draws other masks (the step counter is part of the seed)
    masks1, _ = _masks(model, text, lens, 1, p, p)
    assert any(not torch.equal(masks[k], masks1[k]) for k in masks)


def test_same_seed_is_bit_equal_and_seeds_differ():
    runs = []
    for seed in (3, 3, 4):
        _, d, model = _prepared("lstm_train_tiny", dropout_rate=0.5, seed=seed)
        loss, _, _, grads, _ = _one_pass(model, *batch(d))
        runs.append((loss, grads))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    assert not torch.equal(runs[0][0], runs[2][0])


@pytest.mark.parametrize("amp", [False, True], ids=["f32", "bf16"])
def test_scorer_packs_follow_the_trained_weights(amp):
    """After optimizer steps the same object, in eval mode, scores exactly as a fresh scorer
    loaded from its state_dict: the packs were rebuilt."""
    from espnet_amd.lm import SequentialRNNLM
    from espnet_amd.optim.adam import ArenaAdam
    from espnet_amd.train.trainer import Trainer
    cfg, d, model = _prepared("lstm_train_tiny", amp=amp)
    text, lens = batch(d)
    lm = model.lm
    ys = text[:, :3].cuda()
    lm.eval()
    before, _ = lm.batch_score(ys, [None] * ys.shape[0], None)
    lm.train()
    opt = ArenaAdam(model, lr=1e-2)
    b = {"text": text.cuda(), "text_lengths": lens.cuda()}
    for _ in range(3):
        Trainer.train_one_step(model, b, opt, None, grad_clip=5.0)
    lm.eval()
    got, states = lm.batch_score(ys, [None] * ys.shape[0], None)
    with torch.no_grad():
        logits, _ = lm(ys, None)
    fresh = SequentialRNNLM(**cfg["lm_conf"])
    fresh.load_state_dict({k: v.detach().cpu() for k, v in lm.state_dict().items()})
    fresh.prepare("cuda", amp=amp).eval()
    want, wstates = fresh.batch_score(ys, [None] * ys.shape[0], None)
    with torch.no_grad():
        wlogits, _ = fresh(ys, None)
    assert torch.equal(got, want) and torch.equal(logits, wlogits)
    assert torch.equal(states[0][0], wstates[0][0])
    assert not torch.equal(got, before)
    # and training goes on afterwards
    lm.train()
    loss, _, _, _ = Trainer.train_one_step(model, b, opt, None, grad_clip=5.0)
    assert bool(torch.isfinite(loss))


def test_without_train_flag_it_is_still_a_scorer():
    from espnet_amd.lm import ESPnetLanguageModel, SequentialRNNLM, TransformerLM
    lm = SequentialRNNLM(vocab_size=11, unit=8, nlayers=1).prepare("cuda")
    lm.train()
    with pytest.raises(NotImplementedError, match="no training"):
        lm(torch.ones(2, 3, dtype=torch.long), None)
    with pytest.raises(NotImplementedError, match="no training"):
        ESPnetLanguageModel(TransformerLM(vocab_size=11, embed_unit=8, att_unit=8, unit=16, layer=1), 11).prepare("cuda")


def test_embedding_backward_beyond_one_call():
    """B * T > 4096 rows: EmbedFn's backward runs ea_embed_bwd in several calls that accumulate
    into the same gradient rows.  Against index_add in float64, within max(1e-6, 4 x the deviation
    of index_add in f32 on the CPU); the padding row stays zero."""
    from espnet_amd.lm import SequentialRNNLM
    from espnet_amd.lm.rnn_train import EMBED_BWD_ROWS, EmbedFn
    V, d, rows = 11, 20, 2 * EMBED_BWD_ROWS + 905
    lm = SequentialRNNLM(vocab_size=V, unit=d, nlayers=1).prepare("cuda", train=True)
    gen = torch.Generator().manual_seed(5)
    tok = torch.randint(0, V, (rows,), generator=gen)
    dx = torch.randn(rows, d, generator=gen)
    lm.arena.zero_grad()
    x = EmbedFn.apply(lm._anchor, tok.cuda(), lm._embed)
    assert torch.equal(x.cpu(), lm.encoder.weight.detach().cpu()[tok])
    x.backward(dx.cuda())
    got = lm.encoder.weight.grad.detach().cpu()
    ref64 = torch.zeros(V, d, dtype=torch.float64).index_add_(0, tok, dx.double())
    ref32 = torch.zeros(V, d).index_add_(0, tok, dx)
    ref64[0], ref32[0] = 0, 0
    bound = max(1e-6, 4 * float((ref32.double() - ref64).abs().max()))
    err = float((got.double() - ref64).abs().max())
    print(f"embedding gradient over {rows} rows: max |err| {err:.3e}, bound {bound:.3e}")
    assert err <= bound and not got[0].any()
