"""SequentialRNNLM decoding step on the GPU: one batch_score call (nlayers fused LSTM launches,
the output Linear, the row log-softmax) at the two recipe sizes, f32 and bf16 packs.

    python scripts/bench_rnn_lm.py                      # device-event and host time per step, one JSON line each
    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python scripts/bench_rnn_lm.py --trace
    python scripts/bench_rnn_lm.py --kernel-csv DIR/.../t_kernel_trace.csv   # joins the kernel times

Every step feeds the previous step's states back in a rotated order, so the parent gather runs
as it does in a beam.  Bytes are computed from shapes: the packed LSTM operands and the padded
decoder.weight are each read once per step; the x / h operand re-reads (cache hits) are not
counted.  The rate printed is bytes / kernel time of the LSTM launches alone, beside the 6.3 TB/s
measured HBM copy ceiling; a model that fits the 256 MB Infinity Cache stays resident there
between steps, so its figure is a cache rate and is labelled as one."""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "espnet-1_amd"))

CONFIGS = [dict(n=10, nlayers=2, unit=650), dict(n=60, nlayers=4, unit=2048)]
VOCAB = 5000
HBM_CEILING = 6.3e12  # measured copy rate, bytes/s
INFINITY_CACHE = 256 * 2 ** 20


def kernel_name(unit, n, amp):
    """The ea_lstm_step instantiation a configuration launches (csrc/lstm_core.h launch_tiles)."""
    mt = 1 if n <= 16 else 2 if n <= 32 else 4
    nj = 2 if (unit + 3) // 4 >= 256 else 1
    return f"lstm_step_kernel<{'true' if amp else 'false'}, {mt}, {nj}, {4 if mt == 4 else 8}>"


def canonical(name):
    """A traced kernel name -> kernel_name()'s form."""
    m = re.search(r"lstm_step_kernel<(true|false),\s*(\d+),\s*(\d+),\s*(\d+)>", name)
    return m and f"lstm_step_kernel<{m.group(1)}, {m.group(2)}, {m.group(3)}, {m.group(4)}>"


def shape_bytes(nlayers, unit, amp):
    es = 2 if amp else 4
    kp = 2 * ((unit + 31) // 32 * 32)
    lstm = nlayers * ((unit + 3) // 4 * 16) * kp * es
    dec = VOCAB * (kp // 2) * es
    return lstm, dec


def make(cfg, amp):
    import torch
    from espnet_amd.lm import SequentialRNNLM
    torch.manual_seed(0)
    with torch.device("cuda"):
        lm = SequentialRNNLM(VOCAB, unit=cfg["unit"], nlayers=cfg["nlayers"])
    lm.prepare("cuda", amp=amp)
    lm.eval()
    n = cfg["n"]
    ys = torch.randint(1, VOCAB, (n, 8), device="cuda")
    _, states = lm.batch_score(ys, [None] * n, None)
    return lm, ys, states


def step(lm, ys, states):
    n = len(states)
    _, st = lm.batch_score(ys, [states[(i + 1) % n] for i in range(n)], None)
    return st


def run(cfg, amp, trace):
    import torch
    lm, ys, states = make(cfg, amp)
    for _ in range(20):
        states = step(lm, ys, states)
    torch.cuda.synchronize()
    if trace:
        for _ in range(100):
            states = step(lm, ys, states)
        torch.cuda.synchronize()
        return None
    reps, window = 100, 0.0
    while window < 0.2:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        for _ in range(reps):
            states = step(lm, ys, states)
        host = time.perf_counter() - t0  # enqueue only: nothing in the loop waits for the device
        e1.record()
        torch.cuda.synchronize()
        window = e0.elapsed_time(e1) * 1e-3
        used, reps = reps, reps * 2
    lstm_b, dec_b = shape_bytes(cfg["nlayers"], cfg["unit"], amp)
    assert lstm_b + dec_b == lm.packed_bytes()
    return dict(cfg, dtype="bf16" if amp else "f32", steps=used, window_s=round(window, 4),
                step_us=round(window / used * 1e6, 2), host_us_per_step=round(host / used * 1e6, 2),
                launches_per_step=cfg["nlayers"] + 2, lstm_bytes_per_step=lstm_b, linear_bytes_per_step=dec_b,
                fits_infinity_cache=lstm_b + dec_b < INFINITY_CACHE, kernel=kernel_name(cfg["unit"], cfg["n"], amp))


def join_kernel_times(path):
    by = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            by.setdefault(canonical(row["Kernel_Name"]), []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    for cfg in CONFIGS:
        for amp in (False, True):
            want = kernel_name(cfg["unit"], cfg["n"], amp)
            durs = by.get(want, [])
            if not durs:
                raise SystemExit(f"no launches of {want} in {path}")
            med = statistics.median(durs) * 1e-9
            lstm_b, _ = shape_bytes(cfg["nlayers"], cfg["unit"], amp)
            per = lstm_b / cfg["nlayers"]
            resident = sum(shape_bytes(cfg["nlayers"], cfg["unit"], amp)) < INFINITY_CACHE
            print(json.dumps(dict(cfg, dtype="bf16" if amp else "f32", kernel=want, launches=len(durs),
                                  kernel_us_median=round(med * 1e6, 2), bytes_per_launch=int(per),
                                  tb_per_s=round(per / med * 1e-12, 3),
                                  share_of_hbm_ceiling=round(per / med / HBM_CEILING, 3),
                                  source="Infinity Cache resident (not an HBM rate)" if resident else "HBM")))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true", help="fixed 100 steps per configuration, for a profiler run")
    ap.add_argument("--kernel-csv", help="rocprofv3 kernel_trace.csv of a --trace run: print the kernel figures")
    a = ap.parse_args()
    if a.kernel_csv:
        join_kernel_times(a.kernel_csv)
        sys.exit(0)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rnn_lm needs the GPU (no CPU fallback)")
    for cfg in CONFIGS:
        for amp in (False, True):
            r = run(cfg, amp, a.trace)
            if r:
                print(json.dumps(r), flush=True)
