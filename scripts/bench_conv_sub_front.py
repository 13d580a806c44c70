"""The conv2d6 / conv2d2 front alone on the GPU, forward + backward: ConformerEncoder.front (conv1,
the strided valid-conv kernels of csrc/conv_sub.hip, the output Linear) against the eager torch.nn
module of the reference's definition (subsampling.py:94-200) on the same GPU in the same run.

    python scripts/bench_conv_sub_front.py [--layers conv2d6 conv2d2] [--rounds 3] [--steps 5]

Shapes: B 32, T 1000, F 80; d 512 for conv2d6, d 256 for conv2d2; f32 and bf16.  The two sides are
timed alternately, `rounds` times `steps` forward + backward pairs each, with device events around
every round; the line gives each side's median round and its min-max spread in ms per pair, their
ratio, and the FLOPs of conv.2 (forward, input gradient, weight gradient: 3 x 2 M N K, from the shapes)
over the HIP side's whole-front time: a lower bound of the kernels' own rate, not a kernel time."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "espnet-1_amd"))

B, T, FD = 32, 1000, 80
LAYERS = {"conv2d6": (5, 3, 512), "conv2d2": (3, 1, 256)}  # kernel, stride of conv.2; d


def hip_front(layer, d, amp):
    import torch
    from espnet_amd.arena import ParamArena
    from espnet_amd.asr.encoder.conformer_encoder import ConformerEncoder
    torch.manual_seed(0)
    enc = ConformerEncoder(FD, output_size=d, attention_heads=4, linear_units=8, num_blocks=1, dropout_rate=0.0,
                           positional_dropout_rate=0.0, attention_dropout_rate=0.0, input_layer=layer,
                           rel_pos_type="latest")
    holder = torch.nn.Module()
    holder.encoder = enc
    cd = torch.bfloat16 if amp else torch.float32
    arena = ParamArena(holder, torch.device("cuda:0"), enc.arena_groups("encoder."), shadow_dtype=cd)
    enc.bind(arena, "encoder.", cd, torch.zeros(1, device="cuda:0", requires_grad=True))
    enc.train()
    return enc, (holder, arena)


def torch_front(layer, d, amp):
    import torch
    from torch import nn
    k, s, _ = LAYERS[layer]
    f2 = ((FD - 1) // 2 - k) // s + 1

    class Ref(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = nn.Sequential(nn.Conv2d(1, d, 3, 2), nn.ReLU(), nn.Conv2d(d, d, k, s), nn.ReLU())
            self.out = nn.Linear(d * f2, d)

        def forward(self, x):
            x = self.conv(x.unsqueeze(1))
            b, c, t, f = x.size()
            return self.out(x.transpose(1, 2).contiguous().view(b, t, c * f)) * math.sqrt(d)

    torch.manual_seed(0)
    return Ref().to("cuda:0", torch.bfloat16 if amp else torch.float32)


def run(layer, amp, rounds, steps):
    import torch
    k, s, d = LAYERS[layer]
    t1, f1 = (T - 1) // 2, (FD - 1) // 2
    t2, f2 = (t1 - k) // s + 1, (f1 - k) // s + 1
    gen = torch.Generator().manual_seed(1)
    xs = torch.randn(B, T, FD, generator=gen).cuda()
    ilens = torch.full((B,), T, device="cuda")
    cot = torch.randn(B, t2, d, generator=gen).cuda()
    enc, keep = hip_front(layer, d, amp)
    ref = torch_front(layer, d, amp)
    xr, cr = (xs.bfloat16(), cot.bfloat16()) if amp else (xs, cot)

    def hip_pair():
        x, _ = enc.front(xs, ilens, 0)
        x.backward(cot)

    def torch_pair():
        ref.zero_grad(set_to_none=True)
        ref(xr).backward(cr)

    times = {"hip": [], "torch": []}
    for fn in (hip_pair, torch_pair):  # warm-up: code objects, MIOpen's algorithm choice, the allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in (("hip", hip_pair), ("torch", torch_pair)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / steps)
    hip, tor = statistics.median(times["hip"]), statistics.median(times["torch"])
    flops = 3 * 2 * (B * t2 * f2) * d * (k * k * d)
    print(json.dumps(dict(layer=layer, dtype="bf16" if amp else "f32", B=B, T=T, F=FD, d=d,
                          hip_ms=round(hip, 3), hip_spread=[round(min(times["hip"]), 3), round(max(times["hip"]), 3)],
                          torch_ms=round(tor, 3),
                          torch_spread=[round(min(times["torch"]), 3), round(max(times["torch"]), 3)],
                          torch_over_hip=round(tor / hip, 3), conv2_tflops_over_front_time=round(flops / hip / 1e9, 1))),
          flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", nargs="+", default=list(LAYERS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_conv_sub_front.py needs the GPU: there is no CPU timing")
    for layer in a.layers:
        for amp in (False, True):
            run(layer, amp, a.rounds, a.steps)
