"""Forward + backward of the attention-RNN decoder (decoder: rnn) on the GPU at two shapes over a
Conformer-L-sized encoder memory (B = 30, T' = 249 with ragged lengths 249 .. 150, E = 512, L = 40
target positions, V = 5000): the egs2/aishell/asr1/conf/train_asr_rnn.yaml decoder (2 x 1024,
adim 1024, aconv_chans 10, aconv_filts 100) and the 1 x 320 / adim 320 variant, f32 and bf16,
beside the same module written in eager torch (torch.nn.LSTMCell, conv2d, Linear, softmax: the
reference's forward; bf16 = torch.autocast) on the same card in the same run.

    python scripts/bench_rnn_decoder.py [--steps 10] [--warmup 3] [--only 1024|320]

Times are device events around `steps` forward + backward passes after `warmup` passes, profiler
off.  Also printed, per shape and dtype: the time of one ea_attloc_fwd / ea_attloc_bwd call (events
around L calls) beside the bytes each must move — pre_enc and hs of the valid frames, computed from
shapes — at the HBM copy rate measured in the same run (a 1 GiB device-to-device copy, read + write
counted).  pre_enc and hs of one batch fit the 256 MB Infinity Cache and are re-read by every step,
so a call faster than that bound is a cache rate, not an error.  One JSON line per measurement.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "espnet-1_amd"))

VOCAB, B, T, E, L = 5000, 30, 249, 512, 40
CONFIGS = {"1024": dict(num_layers=2, hidden_size=1024, att_conf=dict(adim=1024, aconv_chans=10, aconv_filts=100)),
           "320": dict(num_layers=1, hidden_size=320, att_conf=dict(adim=320, aconv_chans=10, aconv_filts=100))}


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


def inputs():
    import torch
    g = torch.Generator().manual_seed(0)
    hlens = torch.linspace(T, 150, B).long()
    return dict(hs=torch.randn(B, T, E, generator=g).cuda(), hlens=hlens.cuda(),
                ys=torch.randint(1, VOCAB - 1, (B, L), generator=g).cuda(),
                ylens=torch.linspace(L, 20, B).long().cuda(), cot=(torch.randn(B, L, VOCAB, generator=g) * 1e-3).cuda())


def build(cfg, amp):
    import torch
    from espnet_amd.arena import ParamArena
    from espnet_amd.asr.decoder.rnn_decoder import RNNDecoder
    torch.manual_seed(0)
    dec = RNNDecoder(VOCAB, E, **cfg)
    holder = torch.nn.Module()
    holder.decoder = dec
    cd = torch.bfloat16 if amp else torch.float32
    arena = ParamArena(holder, torch.device("cuda", torch.cuda.current_device()), shadow_dtype=cd)
    dec.bind(arena, "decoder.", cd)
    dec.train()
    return dec, arena


def ours(dec, arena, inp, steps, warmup):
    hs = inp["hs"].clone().requires_grad_(True)

    def step():
        arena.zero_grad()
        hs.grad = None
        y, _ = dec(hs, inp["hlens"], inp["ys"], inp["ylens"])
        y.backward(inp["cot"])

    return _timed(step, steps, warmup)


def attloc_launch(dec, inp, amp):
    """ms per ea_attloc_fwd / ea_attloc_bwd call (events around L calls, each step on the weights
    of the step before, as the decoder runs them)."""
    import torch
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import BF16, F32, lib
    att, b = dec.att_list[0], dec._b
    A, C, F = att.att_dim, att.aconv_chans, att.aconv_filts
    md, mt = (BF16, torch.bfloat16) if amp else (F32, torch.float32)
    dev = "cuda"
    hs = inp["hs"].to(mt).contiguous()
    pre = torch.randn(B, T, A, device=dev).to(mt)
    q = torch.randn(L, B, A, device=dev)
    w = torch.zeros(L, B, T, device=dev)
    c = torch.empty(B, E, device=dev)
    dc = torch.randn(B, E, device=dev) * 1e-3
    dwc = torch.zeros(2, B, T, device=dev)
    dpre, dhs = torch.zeros(B, T, A, device=dev), torch.zeros(B, T, E, device=dev)
    dq = torch.empty(B, A, device=dev)
    part = torch.zeros(B, A * C + C * (2 * F + 1) + A + 1, device=dev)
    ws = torch.empty(B * T * (1 + (3 + (A + 63) // 64) * C), device=dev)
    kw, mw, gw, gb = (b.f(f"att_list.0.{n}").data_ptr() for n in ("loc_conv.weight", "mlp_att.weight", "gvec.weight",
                                                                  "gvec.bias"))
    hl = inp["hlens"].data_ptr()

    def fwd():
        st = ops.stream()
        for i in range(L):
            lib.ea_attloc_fwd(md, B, T, E, A, C, F, hs.data_ptr(), E, T * E, pre.data_ptr(), A, T * A, hl, q[i].data_ptr(),
                              A, w[i - 1].data_ptr() if i else None, T, kw, mw, gw, gb, w[i].data_ptr(), T, c.data_ptr(),
                              E, ws.data_ptr(), ws.numel(), st)

    def bwd():
        st = ops.stream()
        for i in range(L - 1, -1, -1):
            last = i == L - 1
            lib.ea_attloc_bwd(md, B, T, E, A, C, F, hs.data_ptr(), E, T * E, pre.data_ptr(), A, T * A, hl, q[i].data_ptr(),
                              A, w[i - 1].data_ptr() if i else None, T, w[i].data_ptr(), T, kw, mw, gw, dc.data_ptr(), E,
                              None if last else dwc[(i + 1) & 1].data_ptr(), T, dpre.data_ptr(), A, T * A, dhs.data_ptr(),
                              E, T * E, dq.data_ptr(), A, dwc[i & 1].data_ptr() if i else None, T, part.data_ptr(),
                              part.stride(0), ws.data_ptr(), ws.numel(), st)

    return _timed(fwd, 5, 2) / L, _timed(bwd, 5, 2) / L


def baseline(dec, inp, amp, steps, warmup):
    """The reference's forward (rnn_decoder.py:167-249 over AttLoc) in eager torch on the decoder's
    own parameters, differentiated by autograd."""
    import torch
    import torch.nn.functional as F
    att = dec.att_list[0]
    hs = inp["hs"].clone().requires_grad_(True)
    hlens, ys, ylens, cot = inp["hlens"], inp["ys"], inp["ylens"], inp["cot"]
    pad = torch.arange(T, device="cuda").unsqueeze(0) >= hlens.unsqueeze(1)
    ypad = (torch.arange(L, device="cuda").unsqueeze(0) >= ylens.unsqueeze(1)).unsqueeze(2)
    params = list(dec.parameters())

    def step():
        for p in params:
            p.grad = None
        hs.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            z = [hs.new_zeros(B, dec.dunits) for _ in range(dec.dlayers)]
            c = [hs.new_zeros(B, dec.dunits) for _ in range(dec.dlayers)]
            pre = att.mlp_enc(hs)
            aprev = (~pad).float() / hlens.float().unsqueeze(1)
            eys = dec.embed(ys)
            outs = []
            for i in range(L):
                conv = att.loc_conv(aprev.view(B, 1, 1, T)).squeeze(2).transpose(1, 2)
                e = att.gvec(torch.tanh(att.mlp_att(conv) + pre + att.mlp_dec(z[0]).view(B, 1, -1))).squeeze(2)
                w = F.softmax(2.0 * e.float().masked_fill(pad, float("-inf")), dim=1)
                ctx = torch.sum(hs * w.view(B, T, 1), dim=1)
                aprev = w
                x = torch.cat((eys[:, i], ctx), dim=1)
                for l, cell in enumerate(dec.decoder):
                    z[l], c[l] = cell(x if l == 0 else z[l - 1], (z[l], c[l]))
                outs.append(z[-1])
            y = dec.output(torch.stack(outs, dim=1)).float().masked_fill(ypad, 0.0)
        y.backward(cot)

    ms = _timed(step, steps, warmup)
    for p in params:  # the arena's gradient views again
        p.grad = None
    dec._b.arena.rebind()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=list(CONFIGS), default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rnn_decoder.py measures on the GPU: none found")
    rate = copy_rate()
    print(json.dumps({"hbm_copy_TBps": round(rate / 1e12, 3)}), flush=True)
    inp = inputs()
    frames = int(inp["hlens"].sum())
    for name, cfg in CONFIGS.items():
        if a.only not in (None, name):
            continue
        for amp in (False, True):
            dec, arena = build(cfg, amp)
            ms = ours(dec, arena, inp, a.steps, a.warmup)
            fwd_ms, bwd_ms = attloc_launch(dec, inp, amp)
            base = baseline(dec, inp, amp, a.steps, a.warmup)
            A = cfg["att_conf"]["adim"]
            nbytes = frames * (A + E) * (2 if amp else 4)
            print(json.dumps({"decoder": f"{cfg['num_layers']}x{cfg['hidden_size']}", "adim": A,
                              "dtype": "bf16" if amp else "f32", "B": B, "T": T, "E": E, "L": L, "V": VOCAB,
                              "fwd_bwd_ms": round(ms, 3), "torch_eager_fwd_bwd_ms": round(base, 3),
                              "attloc_fwd_us": round(fwd_ms * 1e3, 2), "attloc_bwd_us": round(bwd_ms * 1e3, 2),
                              "attloc_bytes_MB": round(nbytes / 2 ** 20, 2),
                              "attloc_stream_bound_us": round(nbytes / rate * 1e6, 2)}), flush=True)
            del dec, arena
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
