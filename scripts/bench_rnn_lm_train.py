"""One training step (forward, backward, Adam with grad_clip 5) of SequentialRNNLM under
ESPnetLanguageModel on the GPU, at the two common recipe sizes (2 x 650 and 4 x 2048, V = 5000,
B = 64, T = 64), f32 and bf16, beside the same step of torch.nn.LSTM + nn.Linear +
F.cross_entropy + torch.optim.Adam on the same card (MIOpen's LSTM; bf16 = torch.autocast).

    python scripts/bench_rnn_lm_train.py [--steps 20] [--warmup 5] [--only 650|2048]

Times are device events around `steps` whole steps after `warmup` steps, profiler off.  The
step of this project includes the device-side repack of the recurrent kernels' weight packs
after Adam.  Also printed, per size and dtype: the time of one recurrent launch
(ea_lstm_cell_fwd / ea_lstm_cell_bwd, events around T launches of one layer) beside its
weight-stream bound = bytes of the W_hh pack (computed from shapes) / the HBM copy rate measured
in the same run (a 1 GiB device-to-device copy, read + write counted).  A pack that fits the
256 MB Infinity Cache stays resident between launches, so a launch faster than that bound is a
cache rate, not an error.  One JSON line per measurement.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "espnet-1_amd"))

VOCAB, B, T = 5000, 64, 64
CONFIGS = {"650": dict(unit=650, nlayers=2), "2048": dict(unit=2048, nlayers=4)}


def _timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def copy_rate():
    """bytes/s of a 1 GiB device-to-device copy (read + write)."""
    import torch
    n = 1 << 28
    x, y = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    ms = _timed(lambda: y.copy_(x), 10, 3)
    return 2 * 4 * n / (ms * 1e-3)


def ours(cfg, amp, steps, warmup):
    import torch
    from espnet_amd.lm import ESPnetLanguageModel, SequentialRNNLM
    from espnet_amd.optim.adam import ArenaAdam
    from espnet_amd.train.trainer import Trainer
    torch.manual_seed(0)
    model = ESPnetLanguageModel(SequentialRNNLM(VOCAB, **cfg), VOCAB)
    model.prepare("cuda", amp=amp)
    model.train()
    opt = ArenaAdam(model, lr=1e-3)
    text = torch.randint(1, VOCAB - 1, (B, T - 1), device="cuda")
    batch = {"text": text, "text_lengths": torch.full((B,), T - 1, device="cuda")}
    ms = _timed(lambda: Trainer.train_one_step(model, batch, opt, None, grad_clip=5.0), steps, warmup)
    return ms, model


def recurrent_launch(model, amp):
    """ms per ea_lstm_cell_fwd / ea_lstm_cell_bwd launch of layer 0 (events around T launches)."""
    import torch
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import BF16, F32, lib
    lm = model.lm
    H = lm.nhid
    Hp, G = (H + 31) // 32 * 32, 4 * H
    ldd = (G + 31) // 32 * 32
    wd = BF16 if amp else F32
    dev = "cuda"
    xproj = torch.randn(T, B, G, device=dev)
    hs, cs = torch.zeros(T + 1, B, Hp, device=dev), torch.zeros(T + 1, B, Hp, device=dev)
    hb = torch.zeros(T + 1, B, Hp, dtype=torch.bfloat16, device=dev)
    gates = torch.empty(T, B, G, device=dev)
    dy = torch.randn(T, B, Hp, device=dev) * 1e-3
    dg = torch.empty(T, B, ldd, device=dev)
    dgb = torch.empty(T, B, ldd, dtype=torch.bfloat16, device=dev)
    dc = torch.empty(2, B, Hp, device=dev)
    hh = lm._layers[0].hh
    pk, pkt = hh.fwd.data_ptr(), hh.bwd.data_ptr()
    hin = hb if amp else hs
    dgn = dgb if amp else dg

    def fwd():
        st = ops.stream()
        for t in range(T):
            lib.ea_lstm_cell_fwd(wd, B, H, pk, xproj[t].data_ptr(), G, hin[t].data_ptr(), cs[t].data_ptr(), Hp,
                                 hs[t + 1].data_ptr(), cs[t + 1].data_ptr(), Hp, hb[t + 1].data_ptr(),
                                 gates[t].data_ptr(), G, st)

    def bwd():
        st = ops.stream()
        for t in range(T - 1, -1, -1):
            first = t == T - 1
            lib.ea_lstm_cell_bwd(wd, B, H, pkt, None if first else dgn[t + 1].data_ptr(), ldd, dy[t].data_ptr(), Hp,
                                 gates[t].data_ptr(), G, cs[t + 1].data_ptr(), cs[t].data_ptr(), Hp,
                                 None if first else dc[(t + 1) & 1].data_ptr(), dc[t & 1].data_ptr(), Hp,
                                 dg[t].data_ptr(), dgb[t].data_ptr(), ldd, None, 0, st)

    return _timed(fwd, 10, 3) / T, _timed(bwd, 10, 3) / T


def baseline(cfg, amp, steps, warmup):
    import torch
    import torch.nn.functional as F
    torch.manual_seed(0)
    H, L = cfg["unit"], cfg["nlayers"]
    emb = torch.nn.Embedding(VOCAB, H, padding_idx=0).cuda()
    rnn = torch.nn.LSTM(H, H, L, batch_first=True).cuda()
    dec = torch.nn.Linear(H, VOCAB).cuda()
    params = [p for m in (emb, rnn, dec) for p in m.parameters()]
    opt = torch.optim.Adam(params, lr=1e-3)
    x = torch.randint(1, VOCAB - 1, (B, T), device="cuda")
    t = torch.randint(1, VOCAB - 1, (B, T), device="cuda")

    def step():
        opt.zero_grad(set_to_none=False)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            y, _ = rnn(emb(x))
            logits = dec(y)
        loss = F.cross_entropy(logits.float().view(-1, VOCAB), t.view(-1))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 5.0)
        opt.step()

    return _timed(step, steps, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=list(CONFIGS), default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rnn_lm_train.py measures on the GPU: none found")
    rate = copy_rate()
    print(json.dumps({"hbm_copy_TBps": round(rate / 1e12, 3)}), flush=True)
    for name, cfg in CONFIGS.items():
        if a.only not in (None, name):
            continue
        for amp in (False, True):
            ms, model = ours(cfg, amp, a.steps, a.warmup)
            fwd_ms, bwd_ms = recurrent_launch(model, amp)
            del model
            torch.cuda.empty_cache()
            base = baseline(cfg, amp, a.steps, a.warmup)
            torch.cuda.empty_cache()
            H = cfg["unit"]
            es = 2 if amp else 4
            pack_f = ((H + 3) // 4 * 16) * ((H + 31) // 32 * 32) * es
            pack_b = ((H + 15) // 16 * 16) * ((4 * H + 31) // 32 * 32) * es
            print(json.dumps({"model": f"{cfg['nlayers']}x{H}", "dtype": "bf16" if amp else "f32", "B": B, "T": T,
                              "V": VOCAB, "step_ms": round(ms, 3), "torch_miopen_step_ms": round(base, 3),
                              "cell_fwd_us": round(fwd_ms * 1e3, 2), "cell_fwd_stream_bound_us":
                              round(pack_f / rate * 1e6, 2), "cell_bwd_us": round(bwd_ms * 1e3, 2),
                              "cell_bwd_stream_bound_us": round(pack_b / rate * 1e6, 2),
                              "pack_fwd_MB": round(pack_f / 2 ** 20, 2), "pack_bwd_MB": round(pack_b / 2 ** 20, 2)}),
                  flush=True)


if __name__ == "__main__":
    main()
