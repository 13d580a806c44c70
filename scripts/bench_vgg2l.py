"""VGG2L forward + backward at the aishell shape (B 30, T 800, F 83) in f32 and bf16 on the HIP
kernels, beside the eager torch.nn module (four Conv2d + relu + max_pool2d with autograd; under
torch.autocast(bfloat16) for the bf16 column) on the same GPU and input: that module is the
baseline.  And the aishell recipe's hybrid training step (encoder: vgg_rnn 3 x 1024 without
projection, decoder: rnn 2 x 1024, ctc_weight 0.5), eager and through the captured-step runner.

    python scripts/bench_vgg2l.py [--reps 5] [--only vgg|step]

Device events around whole passes after warm-up passes; the two variants alternate inside one
process, `reps` times each; every repeat is printed with the median and the spread, one JSON line
per measurement, with the achieved fraction of the derived bounds (1.1 TFLOP at the
157 TF f32 matrix peak is 7 ms; bf16 is bound by activation traffic, compute under 1 ms).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "espnet-1_amd"))

B, T, F = 30, 800, 83
F32_MATRIX_PEAK_TF = 157.0
HBM_PEAK_GBS = 8000.0


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


def flops():
    """Forward FLOPs of the four convolutions; the backward of the three GEMM layers is twice that
    (input and weight gradient; conv1_1 has no input gradient)."""
    h2, w2 = (T + 1) // 2, (F + 1) // 2
    layers = [(T * F, 1, 64), (T * F, 64, 64), (h2 * w2, 64, 128), (h2 * w2, 128, 128)]
    fwd = sum(2.0 * B * p * 9 * ci * co for p, ci, co in layers)
    bwd = 2 * fwd - 2.0 * B * T * F * 9 * 64
    return fwd, fwd + bwd


def bytes_moved(e):
    """Compulsory HBM traffic of one forward + backward with activations of e bytes (every tensor
    counted once per kernel that reads or writes it; the nine taps' re-reads are taken as cache hits;
    weights and partials, a few MB, left out).  p1 / p2 / p4: elements of a 64-channel map at full,
    half and quarter resolution."""
    h2, w2 = (T + 1) // 2, (F + 1) // 2
    h4, w4 = (h2 + 1) // 2, (w2 + 1) // 2
    p1, p2, p4 = B * T * F * 64, B * h2 * w2 * 64, B * h4 * w4 * 64
    x1, pm, x3, out, dec1, dec2 = p1 * e, p2 * e, 2 * p2 * e, 2 * p4 * 4, p2, 2 * p4
    fwd = B * T * F * 4 + 2 * x1 + (2 * pm + dec1) + 2 * x3 + (out + dec2)  # each map written once, read once
    g4, dp1 = out + dec2, p2 * 4 + dec1  # a pooled gradient (f32) with its decision bytes
    bwd = (g4 + (x3 + g4) + (g4 + x3 + x3)           # conv2_2: dbias, wgrad, dgrad (mask, d3 out)
           + x3 + (pm + x3) + (x3 + p2 * 4)          # conv2_1: colsum, wgrad, dgrad (dp1 out)
           + dp1 + (x1 + dp1) + (dp1 + x1 + x1)      # conv1_2: dbias, wgrad, dgrad (mask, d1 out)
           + x1 + B * T * F * 4)                     # conv1_1: wgrad
    return fwd + bwd


def vgg(amp, reps):
    import torch
    import torch.nn.functional as Fn
    from espnet_amd.arena import ParamArena
    from espnet_amd.asr.encoder.vgg_rnn_encoder import VGGRNNEncoder
    torch.manual_seed(0)
    enc = VGGRNNEncoder(F, num_layers=1, hidden_size=8, output_size=8)
    ref = [torch.nn.Conv2d(c.in_channels, c.out_channels, 3, padding=1).cuda() for c in enc.enc[0].children()]
    for r, c in zip(ref, enc.enc[0].children()):
        r.load_state_dict(c.state_dict())
    holder = torch.nn.Module()  # a parameter arena of the encoder's own, as ESPnetASRModel.prepare makes
    holder.encoder = enc
    cd = torch.bfloat16 if amp else torch.float32
    arena = ParamArena(holder, torch.device("cuda:0"), enc.arena_groups("encoder."), shadow_dtype=cd)
    enc.bind(arena, "encoder.", cd, torch.zeros(1, device="cuda:0", requires_grad=True))
    m = enc.enc[0]
    m.train()
    xs = torch.randn(B, T, F, device="cuda")
    lens = torch.full((B,), T, device="cuda")
    h4, w4 = ((T + 1) // 2 + 1) // 2, ((F + 1) // 2 + 1) // 2
    cot = torch.randn(h4 * B, 128 * w4, device="cuda")
    cot_ref = cot.view(h4, B, 128, w4).permute(1, 2, 0, 3).contiguous()

    def hip():
        y, _, _ = m(xs, lens, enc._anchor)
        y.backward(cot)

    def eager():
        for r in ref:
            r.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            x = xs.unsqueeze(1)
            x = Fn.relu(ref[1](Fn.relu(ref[0](x))))
            x = Fn.max_pool2d(x, 2, stride=2, ceil_mode=True)
            x = Fn.relu(ref[3](Fn.relu(ref[2](x))))
            x = Fn.max_pool2d(x, 2, stride=2, ceil_mode=True)
        x.float().backward(cot_ref)

    for fn in (hip, eager, hip, eager):
        fn()
    torch.cuda.synchronize()
    th, te = [], []
    for _ in range(reps):
        th.append(_sweep_ms(hip, 2))
        te.append(_sweep_ms(eager, 2))
    _, total = flops()
    med = statistics.median(th)
    extra = dict(tflops=round(total / med / 1e9, 1))
    if not amp:
        extra["fraction_of_f32_matrix_bound"] = round(total / (F32_MATRIX_PEAK_TF * 1e9) / med, 3)
    gb = bytes_moved(2 if amp else 4) / 1e9
    extra.update(compulsory_gb=round(gb, 2), achieved_gb_s=round(gb / med * 1e3, 1),
                 fraction_of_hbm_bound=round(gb / HBM_PEAK_GBS * 1e3 / med, 3))
    _report("vgg2l forward + backward, ms", dtype="bf16" if amp else "f32", B=B, T=T, F=F, hip=th, eager_torch=te,
            **extra)


def step(reps):
    import torch
    from espnet_amd.optim.adam import ArenaAdam
    from espnet_amd.tasks.asr import build_model
    from espnet_amd.train.graph import CapturedTrainStep
    from espnet_amd.train.trainer import Trainer
    V, L = 4233, 20
    tok = ["<blank>", "<unk>"] + [f"t{i}" for i in range(V - 3)] + ["<sos/eos>"]
    conf = dict(token_list=tok, input_size=F, encoder="vgg_rnn",
                encoder_conf=dict(rnn_type="lstm", bidirectional=True, use_projection=False, num_layers=3,
                                  hidden_size=1024, output_size=1024, dropout=0.0, in_channel=1),
                decoder="rnn", decoder_conf=dict(rnn_type="lstm", num_layers=2, hidden_size=1024,
                                                 sampling_probability=0.0, dropout=0.0, att_conf=dict(adim=1024)),
                model_conf=dict(ctc_weight=0.5, lsm_weight=0.0))
    g = torch.Generator().manual_seed(0)
    sl = torch.randint(T // 2, T + 1, (B,), generator=g)
    sl[0] = T
    tl = torch.randint(L // 2, L + 1, (B,), generator=g)
    tl[0] = L
    text = torch.randint(2, V - 1, (B, L), generator=g)
    for b in range(B):
        text[b, tl[b]:] = -1
    batch = dict(speech=torch.randn(B, T, F, generator=g), speech_lengths=sl, text=text, text_lengths=tl)
    out = {}
    for mode in ("eager", "captured"):
        torch.manual_seed(0)
        m = build_model(conf)
        m.prepare("cuda:0", amp=False, seed=1)
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
        out[mode] = [_sweep_ms(run, 2) for _ in range(reps)]
        del m, opt, run
        torch.cuda.empty_cache()
    _report("aishell hybrid step, vgg_rnn 3x1024 + decoder rnn 2x1024, f32, ms", B=B, T=T, F=F, **out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["vgg", "step"], default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_vgg2l.py measures on the GPU only")
    if a.only != "step":
        for amp in (False, True):
            vgg(amp, a.reps)
    if a.only != "vgg":
        step(a.reps)
