"""Intermediate CTC under data parallelism and graph capture.

after_norm, ctc_lo and the conditioning layer take gradients from every tap and from the final
head; their prefixes must report grad_ready once per backward, after the lowest tap — an
earlier report lets ArenaDataParallel all-reduce a bucket that is written again afterwards.
As tests/test_dp_streams_gpu.py's bucket test: a world-1 gloo group with the production
issue order and check_issue (every bucket compared between its all-reduce issue point and the
end of the backward), the self-conditioned hybrid model in bf16 with encoder dropout 0.1, three
steps on the ragged batches; gradients and final weights bit-equal to the single-process
serialised steps, with the side streams held back (delay) and in the default mode — with
0.25 MiB buckets and, because those put all three shared prefixes of this small model into one
bucket, also with 1/16 MiB buckets, where the CTC head's report alone releases a bucket.  And one
captured-step case: three captured steps equal three eager steps bit for bit, host RNG
position included (no layer-drop draw for the encoder, before a replay or in an eager step)."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = 3
SHARED = ("ctc.", "encoder.after_norm.", "encoder.conditioning_layer.")
SMALL_BUCKET_MB = 1.0 / 16


def _paths():
    import sys
    for p in (HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "espnet-1_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _setup(dropout=0.1):
    _paths()
    from goldens import section
    from interctc_goldens import load
    from test_model_build import build
    from espnet_amd.optim.adam import ArenaAdam
    from espnet_amd.schedulers.warmup_lr import WarmupLR
    cfg, d = load("interctc_sc_hybrid")
    cfg = dict(cfg)
    cfg["encoder_conf"] = dict(cfg["encoder_conf"], dropout_rate=dropout, positional_dropout_rate=dropout,
                               attention_dropout_rate=dropout)
    torch.manual_seed(0)
    m = build(cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in section(d, "w").items()})
    m.prepare("cuda:0", amp=True, seed=77)
    m.train()
    opt = ArenaAdam(m, lr=0.002, weight_decay=1e-6)  # the scctc recipe's optimizer settings
    return m, opt, WarmupLR(opt, warmup_steps=15000)


def _steps(dp=None, mode="default"):
    """STEPS training steps -> (per-step gradient arenas, final weights)."""
    _paths()
    import test_dp_ragged_gpu as R
    from espnet_amd import hip_ops
    from espnet_amd.train.trainer import Trainer
    m, opt, sched = _setup()
    if dp is not None:
        dp = dp(m)
    grads = []
    orig = opt.compute_grad_norm

    def snap(*a, **k):
        grads.append(m.arena.grad.detach().cpu().clone())
        return orig(*a, **k)

    opt.compute_grad_norm = snap
    prev = hip_ops.DEBUG_DELAY_NS, hip_ops.DEBUG_SERIAL
    hip_ops.DEBUG_DELAY_NS = 300_000 if mode == "delay" else 0
    hip_ops.DEBUG_SERIAL = mode == "serial"
    try:
        for b in R._global_batches(STEPS):
            Trainer.train_one_step(m, {k: v.to("cuda:0") for k, v in b.items()}, opt, sched, grad_clip=5.0, dp=dp)
        torch.cuda.synchronize()
    finally:
        hip_ops.DEBUG_DELAY_NS, hip_ops.DEBUG_SERIAL = prev
    return grads, m.arena.data.cpu().clone(), m


def _dp_worker(init, q):
    _paths()
    import torch.distributed as dist
    from espnet_amd.train.distributed import ArenaDataParallel
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"file://{init}", rank=0, world_size=1)
    try:
        shared = {}

        def mk(bucket_mb):
            def make(m):
                dp = ArenaDataParallel(m, bucket_mb=bucket_mb, force_collectives=True, check_issue=True)
                assert dp.active and len(dp.buckets) > 2
                for p in SHARED:
                    assert p in dp.prefixes, p
                shared[bucket_mb] = [sorted(mods & set(SHARED)) for mods in dp._bucket_mods if mods & set(SHARED)]
                return dp
            return make
        res = {}
        np_ = lambda g, w: ([x.numpy() for x in g], w.numpy())  # noqa: E731  (pickled by value)
        res["serial"] = np_(*_steps(mode="serial")[:2])
        for mode in ("delay", "default"):
            res[mode] = np_(*_steps(dp=mk(0.25), mode=mode)[:2])
        # 0.25 MiB buckets put the CTC head, the decoder, after_norm and the conditioning layer
        # of this small model into ONE bucket, which any of the three prefixes holds back; with
        # 1/16 MiB the CTC head shares its bucket with decoder parameters only, so the final
        # head's report alone would release it before the taps have written ctc_lo's gradient
        res["small"] = np_(*_steps(dp=mk(SMALL_BUCKET_MB), mode="delay")[:2])
        res["shared"] = shared
        q.put(res)
    except Exception:
        import traceback
        q.put({"error": traceback.format_exc()})
        raise
    finally:
        dist.destroy_process_group()


def test_dp_shared_tap_gradients_final_before_their_all_reduce():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_dp_worker, args=(tempfile.mktemp(prefix="ea_ictc_"), q))
    p.start()
    res = q.get(timeout=170)
    p.join(60)
    assert "error" not in res, res["error"]
    gs, ws = res["serial"]
    assert len(gs) == STEPS and all(float(np.abs(g).sum()) > 0 for g in gs)
    assert ["ctc."] in res["shared"][SMALL_BUCKET_MB], res["shared"]  # a bucket only the CTC head holds back
    for mode in ("delay", "default", "small"):
        g, w = res[mode]
        bad = [s for s, (x, y) in enumerate(zip(g, gs)) if not np.array_equal(x, y)]
        assert not bad, f"{mode}: gradients differ from the single-process serial step at steps {bad}"
        assert np.array_equal(w, ws), mode


def test_captured_steps_equal_eager_steps():
    _paths()
    import test_dp_ragged_gpu as R
    from espnet_amd.train.graph import CapturedTrainStep
    from espnet_amd.train.trainer import Trainer
    torch.cuda.set_device(0)
    # one input shape, so the second call captures and the third replays
    batches = [R._global_batches(1, seed=11 + i)[0] for i in range(STEPS)]
    m1, o1, s1 = _setup()
    torch.manual_seed(99)
    eager = [float(Trainer.train_one_step(m1, b, o1, s1, grad_clip=5.0)[0]) for b in batches]
    rng_eager = torch.get_rng_state()
    m2, o2, s2 = _setup()
    run = CapturedTrainStep(m2, o2, s2, grad_clip=5.0, warmup=1)
    torch.manual_seed(99)
    graph = []
    for b in batches:
        loss, stats, _, _ = run(b)
        graph.append(float(loss))
        assert "loss_interctc_layer1" in stats and "loss_interctc_layer3" in stats
    assert len(run.graphs) == 1 and run.mode == "graph"
    assert eager == graph
    assert len(set(eager)) == len(eager)
    assert torch.equal(rng_eager, torch.get_rng_state())  # the same host draws in both
    for (k, p1), p2 in zip(m1.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(p1, p2), k
