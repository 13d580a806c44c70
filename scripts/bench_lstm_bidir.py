"""Per-step time of the two-direction LSTM launch (ea_lstm_bicell_fwd / ea_lstm_bicell_bwd, one
launch for both directions) beside the same sweep on ea_lstm_cell_fwd / ea_lstm_cell_bwd launched
once per direction (two LSTMTapes: what the encoder would cost on the single-direction kernels,
without the length mask), at B 30, T 250, H 320 and H 1024, f32 and bf16; and the whole hybrid
training step (encoder: rnn 4 x 320 with subsample (2, 2, 1, 1), decoder: rnn, ctc_weight 0.5) at
B 30, T 1000, F 80, eager and through the captured-step runner.

    python scripts/bench_lstm_bidir.py [--reps 5] [--only kernels|step]

A sweep is T launches; the time is device events around whole sweeps after two warm-up sweeps,
divided by T.  The two variants alternate inside one process, `reps` times each; every repeat is
printed with the median and the spread (min .. max), one JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "espnet-1_amd"))

B, T = 30, 250


def _sweep_ms(fn, n=1):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def _report(what, **kw):
    for k, v in list(kw.items()):
        if isinstance(v, list):
            kw[k] = dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3),
                         all=[round(x, 3) for x in v])
    print(json.dumps(dict(what=what, **kw)), flush=True)


def kernels(H, cd, reps):
    import torch
    from espnet_amd.lm.rnn_train import BiLSTMTape, LSTMLayer, LSTMTape
    torch.manual_seed(0)
    m = torch.nn.LSTM(80, H, 1, bidirectional=True).cuda()
    lays = []
    for d in range(2):
        w = getattr(m, "weight_ih_l0" + ("_reverse" if d else "")).detach().to(cd)
        lay = LSTMLayer(m, w, cd, k=0, reverse=bool(d))
        lay.refresh()
        lays.append(lay)
    xproj = [torch.randn(T * B, 4 * H, device="cuda") for _ in range(2)]
    dy = torch.randn(T * B, 2 * H, device="cuda")
    dys = [dy[:, :H].contiguous(), dy[:, H:].contiguous()]
    lens = torch.full((B,), T, dtype=torch.long, device="cuda")
    bi = BiLSTMTape(lays, lens, T, B, "cuda")
    singles = [LSTMTape(lay, T, B, "cuda") for lay in lays]

    def single_fwd():
        for tape, xp in zip(singles, xproj):
            step = tape.fwd_steps(xp)
            for t in range(T):
                step(t)

    def single_bwd():
        for tape, g in zip(singles, dys):
            step = tape.bwd_steps(g, H)
            for t in range(T - 1, -1, -1):
                step(t)

    variants = {"fwd": (lambda: bi.forward(xproj), single_fwd), "bwd": (lambda: bi.backward(dy), single_bwd)}
    for name, (two, one) in variants.items():
        for fn in (two, one, two, one):  # warm-up: both variants, twice
            fn()
        torch.cuda.synchronize()
        t2, t1 = [], []
        for _ in range(reps):
            t2.append(_sweep_ms(two, 4) / T * 1e3)
            t1.append(_sweep_ms(one, 4) / T * 1e3)
        _report(f"lstm_bidir {name} per step, us", H=H, dtype=str(cd).split(".")[-1], B=B, T=T,
                one_launch_two_directions=t2, one_launch_per_direction=t1)


def step(reps, amp=False):
    import torch
    from espnet_amd.optim.adam import ArenaAdam
    from espnet_amd.tasks.asr import build_model
    from espnet_amd.train.graph import CapturedTrainStep
    from espnet_amd.train.trainer import Trainer
    Bs, Ts, F, V, L = 30, 1000, 80, 52, 40
    tok = ["<blank>", "<unk>"] + [f"t{i}" for i in range(V - 3)] + ["<sos/eos>"]
    conf = dict(token_list=tok, input_size=F, encoder="rnn",
                encoder_conf=dict(num_layers=4, hidden_size=320, output_size=320, subsample=[2, 2, 1, 1]),
                decoder="rnn", decoder_conf=dict(hidden_size=320, att_conf=dict(adim=320)),
                model_conf=dict(ctc_weight=0.5, lsm_weight=0.1))
    g = torch.Generator().manual_seed(0)
    sl = torch.randint(Ts // 2, Ts + 1, (Bs,), generator=g)
    sl[0] = Ts
    tl = torch.randint(L // 2, L + 1, (Bs,), generator=g)
    tl[0] = L
    text = torch.randint(2, V - 1, (Bs, L), generator=g)
    for b in range(Bs):
        text[b, tl[b]:] = -1
    batch = dict(speech=torch.randn(Bs, Ts, F, generator=g), speech_lengths=sl, text=text, text_lengths=tl)
    out = {}
    for mode in ("eager", "captured"):
        torch.manual_seed(0)
        m = build_model(conf)
        m.prepare("cuda:0", amp=amp, seed=1)
        m.train()
        opt = ArenaAdam(m, lr=1e-3)
        if mode == "eager":
            run = lambda: Trainer.train_one_step(m, batch, opt, None, grad_clip=5.0)  # noqa: E731
        else:
            cap = CapturedTrainStep(m, opt, None, grad_clip=5.0, warmup=1)
            run = lambda: cap(batch)  # noqa: E731
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        out[mode] = [_sweep_ms(run, 3) for _ in range(reps)]
    _report("hybrid step encoder rnn 4x320 + decoder rnn, ms", B=Bs, T=Ts, F=F, amp=amp, **out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["kernels", "step"], default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_lstm_bidir.py measures on the GPU only")
    if a.only != "step":
        for H in (320, 1024):
            for cd in (torch.float32, torch.bfloat16):
                kernels(H, cd, a.reps)
    if a.only != "kernels":
        step(a.reps)
