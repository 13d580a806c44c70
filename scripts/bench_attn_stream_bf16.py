"""Attention forward + backward in bf16 on three paths at one shape: the unfused chain (attn_fwd + attn_bwd), the
f32-MFMA streaming kernels (cores="f32") and the bf16-MFMA ones (cores="bf16"): ms per forward + backward from
device events over alternating windows, and torch's peak allocation during one call above the operands and the
gradient buffer.  With --step, also a captured training step of a 12-block Conformer (d 256, 8 heads, the
6-layer decoder, B 32, T 1000, bf16) under EA_STREAM_ATTN_TRAIN unset / 1 / bf16.

    python scripts/bench_attn_stream_bf16.py [--B 32 --H 8 --T 249 --dk 32 --p 0.1 --calls 50 --rounds 7] [--step]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "espnet-1_amd"))
sys.path.insert(0, ROOT)
from espnet_amd.layers import common as C  # noqa: E402

BF16 = torch.bfloat16


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def spread(v):
    return {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}


def attention(a):
    d = a.H * a.dk
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(a.B * a.T, 3 * d, generator=g).to(BF16).cuda()
    dO = torch.randn(a.B * a.T, d, generator=g).to(BF16).cuda()
    grad = torch.empty_like(qkv)
    kw = dict(B=a.B, H=a.H, T1=a.T, T2=a.T, dk=a.dk, ldq=3 * d, ldk=3 * d, ldv=3 * d, causal=False, scale=a.dk ** -0.5,
              klen=torch.full((a.B,), a.T, dtype=torch.long).cuda())
    ops = (qkv, qkv[:, d:], qkv[:, 2 * d:])
    out = dict(dq=grad, lddq=3 * d, dk_=grad[:, d:], lddk=3 * d, dv=grad[:, 2 * d:], lddv=3 * d)

    def unfused():
        O, P, Pd, ldT = C.attn_fwd(*ops, p=a.p, seed=1, cd=BF16, **kw)
        C.attn_bwd(dO, *ops, P, Pd, ldT, p=a.p, seed=1, cd=BF16, **out,
                   **{k: x for k, x in kw.items() if k not in ("klen", "causal")})
        return O

    def stream(cores):
        O, lse = C.attn_stream_train_fwd(*ops, p=a.p, seed=1, cd=BF16, cores=cores, **kw)
        C.attn_stream_bwd(dO, *ops, lse, p=a.p, seed=1, cores=cores, **out, **kw)
        return O

    fns = {"unfused": unfused, "stream_f32_cores": lambda: stream("f32"), "stream_bf16_cores": lambda: stream("bf16")}
    res = {"shape": dict(B=a.B, H=a.H, T=a.T, dk=a.dk, p=a.p), "max_abs_diff_to_unfused": {}, "peak_bytes": {}}
    ref, gref = unfused().float(), grad.float().clone()
    for k, f in fns.items():
        O = f().float()
        res["max_abs_diff_to_unfused"][k] = {"O": float((O - ref).abs().max()), "grad": float((grad.float() - gref).abs().max())}
        res["peak_bytes"][k] = peak(f)
    for f in fns.values():
        for _ in range(10):
            f()
    ms = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, f in fns.items():
            ms[k].append(timed(f, a.calls))
    res["ms_per_fwd_bwd"] = {k: spread(v) for k, v in ms.items()}
    return res


def step(a):
    import bench
    from espnet_amd.optim.adam import ArenaAdam
    from espnet_amd.schedulers.warmup_lr import WarmupLR
    from espnet_amd.train.graph import CapturedTrainStep
    cfg = bench.c3_config()
    cfg["encoder_conf"] = dict(cfg["encoder_conf"], output_size=256)
    batch = bench.synthetic_batch(cfg, 3)
    res = {}
    for name, (on, cores) in {"unset": (False, "f32"), "1": (True, "f32"), "bf16": (True, "bf16")}.items():
        C.STREAM_ATTN_TRAIN, C.STREAM_ATTN_CORES = on, cores
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        model = bench.build(cfg)
        model.prepare("cuda", amp=True, seed=1234)
        model.train()
        opt = ArenaAdam(model, lr=0.0025, weight_decay=1e-6)
        run = CapturedTrainStep(model, opt, WarmupLR(opt, warmup_steps=40000), grad_clip=5.0, warmup=2)
        for _ in range(5):
            loss = run(batch)[0]
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            run(batch)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        ms.sort()
        res[name] = {"ms_per_step": {"median": ms[len(ms) // 2], "p10": ms[len(ms) // 10], "p90": ms[len(ms) * 9 // 10]},
                     "peak_bytes": torch.cuda.max_memory_allocated(), "loss": float(loss), "mode": run.mode}
        del run, opt, model
    return res


def main():
    ap = argparse.ArgumentParser()
    for k, v in dict(B=32, H=8, T=249, dk=32, calls=50, rounds=7, steps=20).items():
        ap.add_argument("--" + k, type=int, default=v)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--step", action="store_true")
    a = ap.parse_args()
    print(json.dumps({"attention": attention(a)}))
    if a.step:
        print(json.dumps({"step": step(a)}))


if __name__ == "__main__":
    main()
