"""Time one joint step of transducer decoding: the two launches of csrc/transducer_step.hip
against the composition the project had before them -- torch tanh, the few-row GEMM (ops.linear),
log_softmax, torch.topk -- at V 5000, J 640, k 10, n in {1, 8, 32}, f32 and bf16.

    python scripts/bench_rnnt_step.py [--iters 2000] [--reps 7]

Device-event timing: per cell `reps` windows of `iters` steps after a warm-up, the two paths alternating
window by window; the median window and the spread (min .. max) per step are printed.  The workspace is
sized for 32-column slices, so that an A/B build of the library with another EA_RNNT_STEP_SW
(build.py --tag, EA_LIB_NAME) runs on it too."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "espnet-1_amd"))

from espnet_amd import hip_ops as ops  # noqa: E402
from espnet_amd._lib import RNNT_STEP_SW, dt, lib  # noqa: E402

V, J, K, T = 5000, 640, 10, 200


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rnnt_step.py measures on the GPU; none found")
    g = torch.Generator().manual_seed(0)
    E = (torch.randn(T, J, generator=g) * 0.7).cuda()
    W32 = (torch.randn(V, J, generator=g) * (2.0 / J ** 0.5)).cuda()
    bias = (torch.randn(V, generator=g) * 0.3).cuda()
    for cd in (torch.float32, torch.bfloat16):
        w = W32.to(cd)
        for n in (1, 8, 32):
            D = (torch.randn(n, J, generator=g) * 0.7).cuda()
            frame = torch.randint(0, T, (n,), generator=g).to(torch.int32).cuda()
            logits, part = torch.empty(n, V, device="cuda"), torch.empty(2 * n * -(-V // 32), device="cuda")
            out, top, ids = (torch.empty(2, n, device="cuda"), torch.empty(n, K, device="cuda"),
                             torch.empty(n, K, dtype=torch.int32, device="cuda"))

            def step():
                st = ops.stream()
                lib.ea_rnnt_step_logits(dt(w), n, V, J, E.data_ptr(), J, T, frame.data_ptr(), D.data_ptr(), J,
                                        w.data_ptr(), J, bias.data_ptr(), logits.data_ptr(), V, part.data_ptr(), st)
                lib.ea_rnnt_step_select(n, V, K, logits.data_ptr(), V, part.data_ptr(), out[0].data_ptr(),
                                        out[1].data_ptr(), top.data_ptr(), ids.data_ptr(), 0, st)

            fl = frame.long()
            y = torch.empty(n, V, device="cuda")
            epi = ops.make_epi(bias=bias)

            def composed():
                h = torch.tanh(E[fl] + D).to(cd)
                ops.linear(h, w, y, epi=epi)
                lp = torch.log_softmax(y, dim=-1)
                return lp[:, 0], lp[:, 1:].topk(K, dim=-1)

            step(), composed()
            lpb, (tv, ti) = composed()
            agree = bool((ti + 1 == ids).all()) and float((tv - top).abs().max()) < 1e-3 and \
                float((lpb - out[1]).abs().max()) < 1e-3  # the two paths time the same computation
            for fn in (step, composed):
                window(fn, a.iters)
            ts = {"step": [], "composed": []}
            for _ in range(a.reps):
                ts["step"].append(window(step, a.iters))
                ts["composed"].append(window(composed, a.iters))
            print(json.dumps(dict(sw=RNNT_STEP_SW if "EA_LIB_NAME" not in os.environ else os.environ["EA_LIB_NAME"],
                                  dtype=str(cd).split(".")[1], n=n, agree=agree,
                                  **{f"{k}_us": round(statistics.median(v), 2) for k, v in ts.items()},
                                  **{f"{k}_spread_us": [round(min(v), 2), round(max(v), 2)] for k, v in ts.items()})))


if __name__ == "__main__":
    main()
