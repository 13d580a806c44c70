"""Forward + backward of the transducer's joint + loss node in f32 and bf16 against
two baselines, in one run:

    fused        RNNTJointLossFn (csrc/transducer.hip): the logits are never stored
    composition  what the kernels before it allow: tanh(E + D) materialised, ea_gemm to f32 logits,
                 ea_softmax_lse_rows (lse and the probabilities in the compute dtype), the same lattice,
                 dlogits from the stored probabilities in ONE chunk, the same two GEMMs and tanh backward
    eager        torch: tanh, Linear, log_softmax and the two gathers under autograd in the same dtype;
                 its lattice is ea_rnnt_lattice too, whose kappa are the gradients of lp_blank / lp_label

    python scripts/bench_rnnt.py [--shape B T U V J] [--steps 10] [--warmup 3] [--out results.json]

Per path: the median of `steps` device-event timings of one forward + backward after `warmup` calls,
and the growth of the allocator's peak over one call.  Prints one JSON line.  The three losses are
compared before anything is timed."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "espnet-1_amd"))

from espnet_amd import hip_ops as ops  # noqa: E402
from espnet_amd._lib import dt, lib  # noqa: E402
from espnet_amd.asr.joint_network import RNNTJointLossFn  # noqa: E402
from espnet_amd.layers.common import rup  # noqa: E402


def lattice(lpb, lpl, tl, ul):
    """-> (loss, gamma, kappa_blank, kappa_label) of (B, T, U1) f32 log-probabilities."""
    B, T, U1 = lpb.shape
    dev = lpb.device
    ab = torch.empty(2, B, T, U1, dtype=torch.float64, device=dev)
    co = torch.empty(3, B, T, U1, device=dev)
    ll, loss = torch.empty(B, dtype=torch.float64, device=dev), torch.empty((), device=dev)
    lib.ea_rnnt_lattice(B, T, U1, lpb.data_ptr(), lpl.data_ptr(), tl.data_ptr(), ul.data_ptr(), ab[0].data_ptr(),
                        ab[1].data_ptr(), ll.data_ptr(), co[0].data_ptr(), co[1].data_ptr(), co[2].data_ptr(),
                        loss.data_ptr(), ops.stream())
    return loss, co[0], co[1], co[2]


def fused(E, D, W, b, w, y, tl, ul):
    E, D = E.detach().requires_grad_(True), D.detach().requires_grad_(True)
    loss = RNNTJointLossFn.apply(E, D, y, tl, ul, (W, b, w), 1 << 30)
    loss.backward()
    return loss.detach()


def composition(E, D, W, b, w, y, tl, ul):
    (B, T, J), U1, V, cd = E.shape, D.shape[1], w.shape[0], w.dtype
    N, Vp = B * T * U1, rup(w.shape[0])
    h = ops.cast(torch.tanh(E[:, :, None] + D[:, None]).view(N, J), cd)
    logits = torch.empty(N, V, device=E.device)
    ops.linear(h, w, logits, epi=ops.make_epi(bias=b.detach()))
    lse, dl = torch.empty(N, device=E.device), torch.zeros(N, Vp, dtype=cd, device=E.device)
    lib.ea_softmax_lse_rows(N, V, logits.data_ptr(), V, lse.data_ptr(), dl.data_ptr(), dt(dl), Vp, ops.stream())
    yl = torch.cat([y.long(), y.new_zeros(B, 1, dtype=torch.long)], dim=1)[:, None, :].expand(B, T, U1).reshape(N, 1)
    lpb = (logits[:, 0] - lse).view(B, T, U1).contiguous()
    lpl = (logits.gather(1, yl)[:, 0] - lse).view(B, T, U1).contiguous()
    del logits
    loss, gamma, kb, kl = lattice(lpb, lpl, tl, ul)
    dl[:, :V].mul_(gamma.view(N, 1).to(cd))  # gloss = 1: dlogits = (gamma p - [0] kb - [y] kl) / B
    dl[:, 0] -= kb.view(N).to(cd)
    dl.scatter_add_(1, yl, -(kl.view(N, 1).to(cd)))
    dl.mul_(1.0 / B)
    dh = torch.empty(N, J, device=E.device)
    ops.gemm(dl, w, dh, M=N, N=J, K=V, a_kmajor=1, b_kmajor=0, lda=Vp, ldb=J, ldc=J, splitk=False)
    ops.gemm(dl, h, W.grad, M=V, N=J, K=N, a_kmajor=0, b_kmajor=0, lda=Vp, ldb=J, ldc=J, epi=ops.make_epi(beta=1.0),
             splitk=False)
    ops.colsum(dl[:, :V], b.grad, accumulate=True, defer=False)
    dE, dD = torch.empty_like(E), torch.empty_like(D)
    lib.ea_rnnt_joint_dact(B, T, U1, J, E.data_ptr(), D.data_ptr(), tl.data_ptr(), ul.data_ptr(), 0, B * T,
                           dh.data_ptr(), dE.data_ptr(), dD.data_ptr(), ops.stream())
    return loss


def eager(E, D, W, b, w, y, tl, ul):
    (B, T, J), U1, cd = E.shape, D.shape[1], w.dtype
    E, D = E.detach().requires_grad_(True), D.detach().requires_grad_(True)
    wt, bt = w.detach().requires_grad_(True), b.detach().requires_grad_(True)
    lp = torch.log_softmax(torch.nn.functional.linear(torch.tanh(E[:, :, None] + D[:, None]).to(cd), wt, bt.to(cd)).float(),
                           dim=-1)
    yl = torch.cat([y.long(), y.new_zeros(B, 1, dtype=torch.long)], dim=1)[:, None, :, None].expand(B, T, U1, 1)
    lpb, lpl = lp[..., 0].contiguous(), lp.gather(3, yl)[..., 0].contiguous()
    loss, _, kb, kl = lattice(lpb.detach(), lpl.detach(), tl, ul)
    torch.autograd.backward([lpb, lpl], [-kb / B, -kl / B])
    return loss


def measure(fn, args, steps, warmup):
    for _ in range(warmup):
        fn(*args)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn(*args)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(*args)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(ms_median=round(statistics.median(ms), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3),
                peak_mb=round(peak / 2 ** 20, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=5, default=[32, 300, 59, 5000, 640], metavar=("B", "T", "U", "V", "J"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rnnt.py needs the GPU: there is nothing to time without one")
    B, T, U, V, J = a.shape
    g = torch.Generator().manual_seed(0)
    E, D = (torch.randn(B, T, J, generator=g) * 0.7).cuda(), (torch.randn(B, U + 1, J, generator=g) * 0.7).cuda()
    W = torch.nn.Parameter((torch.randn(V, J, generator=g) * (2.0 / J ** 0.5)).cuda())
    b = torch.nn.Parameter((torch.randn(V, generator=g) * 0.3).cuda())
    W.grad, b.grad = torch.zeros_like(W), torch.zeros_like(b)
    y = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32).cuda()
    tl = torch.randint(T * 3 // 4, T + 1, (B,), generator=g, dtype=torch.int32).cuda()
    ul = torch.randint(U // 2, U + 1, (B,), generator=g, dtype=torch.int32).cuda()
    res = dict(shape=dict(B=B, T=T, U=U, V=V, J=J), steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0))
    for name, cd in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        args = (E, D, W, b, W.detach().to(cd), y, tl, ul)
        losses = {f.__name__: float(f(*args)) for f in (fused, composition, eager)}
        ref = losses["fused"]
        assert all(abs(v - ref) <= (1e-4 if cd == torch.float32 else 2e-2) * abs(ref) for v in losses.values()), losses
        res[name] = dict(loss=losses, **{f.__name__: measure(f, args, a.steps, a.warmup) for f in (fused, composition, eager)})
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
