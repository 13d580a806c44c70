"""The joint-step kernels of transducer decoding (csrc/transducer_step.hip) against a plain float64
restatement on the CPU: tanh, the product, log_softmax, topk.  bf16 rounds the product's operands (rd of
tests/test_rnnt_kernels_gpu.py).  Tolerance: tests/lstm_train_goldens.py's rule with margin 4, err = this
restatement's own f32-vs-f64 deviation.

The inputs are made from the joint activations backwards: h is drawn on bf16 values and D = atanh(h) -
E[frame], so that tanh lands in the middle of a bf16 cell and one f32 ulp of tanh cannot move a rounded
operand by a bf16 step (asserted: the f32 and the f64 restatement round h alike).  Planted rows: blank the
global maximum, the maximum in column V - 1, the maximum in column 1, blank the minimum (as many as n holds).
The ids are compared exactly, which is sound because the f64 reference's top k + 1 non-blank values lie more
than twice the tolerance apart (asserted)."""
import functools

import pytest
import torch

from lstm_train_goldens import tolerance
from test_rnnt_kernels_gpu import _bf, rd

pytestmark = pytest.mark.gpu
MARGIN, DT = 4, {"f32": torch.float32, "bf16": torch.bfloat16}
SEED = 1  # the first for which every precondition in test_step holds in every case
# (n, V, J, k): the smallest; V and J tails; k = V - 1; a full row tile and several slices; a second row
# tile with 15 padding rows, the largest J and k
CASES = [(1, 5, 8, 1), (3, 37, 40, 5), (5, 17, 8, 16), (16, 300, 72, 8), (17, 130, 640, 16)]
PLANT = [(0, 1.0), (-1, 1.0), (1, 1.0), (0, -1.0)]  # (column, sign): h = sign * 0.90625 * sign(W[column])


@functools.lru_cache(maxsize=None)
def inputs(case):
    n, V, J, k = case
    g = torch.Generator().manual_seed(SEED + sum(case))
    n_frames = n + 3
    E = torch.randn(n_frames, J + 8, generator=g) * 0.7            # lde = J + 8
    frame = (torch.arange(n) * 7 + 3) % n_frames                   # non-monotone
    if n > 1:
        frame[-1] = frame[0]                                       # a repeat
    W = torch.randn(V, J, generator=g) * (2.0 / J ** 0.5)
    b = torch.randn(V, generator=g) * 0.3
    h = _bf(torch.rand(n, J, generator=g) * 1.9 - 0.95)
    for i, (col, sign) in enumerate(PLANT[:n]):
        h[i] = sign * 0.90625 * torch.sign(W[col])
    D = torch.zeros(n, J + 4)                                      # ldd = J + 4
    D[:, :J] = torch.atanh(h.double()).float() - E[frame, :J]
    return E, frame.to(torch.int32), D, W, b


@functools.lru_cache(maxsize=None)
def restate(case, amp, dtype):
    n, V, J, k = case
    E, frame, D, W, b = inputs(case)
    h = torch.tanh(E[frame.long(), :J].to(dtype) + D[:, :J].to(dtype))
    logits = rd(h, amp) @ rd(W.to(dtype), amp).t() + b.to(dtype)
    lse = torch.logsumexp(logits, dim=-1)
    logp = logits - lse[:, None]
    top = logp[:, 1:].sort(dim=-1, descending=True, stable=True)   # ties to the lower id
    return dict(h=h, lse=lse, lpb=logp[:, 0], logp=logp, top=top.values[:, :k + 1], ids=top.indices[:, :k] + 1)


def close(name, got, ref, r32):
    tol = tolerance(ref, float((r32.double() - ref).abs().max()), MARGIN)
    dev = float((got.double().cpu() - ref).abs().max())
    print(f"{name}: dev {dev:.3e} tol {tol:.3e}")
    assert dev <= tol, (name, dev, tol)  # (a NaN fails it too)


@pytest.mark.parametrize("cd", DT)
@pytest.mark.parametrize("case", CASES, ids="n%dv%dj%dk%d".__mod__)
def test_step(case, cd):
    from espnet_amd import hip_ops as ops
    from espnet_amd._lib import RNNT_STEP_SW, dt, lib
    n, V, J, k = case
    amp = cd == "bf16"
    ref, r32 = (restate(case, amp, d) for d in (torch.float64, torch.float32))
    # preconditions, on the CPU
    assert torch.equal(_bf(ref["h"]), _bf(r32["h"]).double())
    tol_top = tolerance(ref["top"][:, :k], float((r32["top"][:, :k].double() - ref["top"][:, :k]).abs().max()), MARGIN)
    assert float((ref["top"][:, :-1] - ref["top"][:, 1:]).min()) > 2 * tol_top
    assert ref["logp"].argmax(dim=1)[:3].tolist() == [0, V - 1, 1][:n] and 0 not in ref["ids"]  # the planted rows
    assert n < 4 or int(ref["logp"][3].argmin()) == 0

    E, frame, D, W, b = (v.cuda() for v in inputs(case))
    w = W.to(DT[cd])
    logits = torch.full((n, V), float("nan"), device="cuda")
    part = torch.empty(2 * n * -(-V // RNNT_STEP_SW), device="cuda")
    out, top = torch.full((2, n), float("nan"), device="cuda"), torch.full((n, k), float("nan"), device="cuda")
    ids = torch.zeros(n, k, dtype=torch.int32, device="cuda")
    lib.ea_rnnt_step_logits(dt(w), n, V, J, E.data_ptr(), E.stride(0), E.shape[0], frame.data_ptr(), D.data_ptr(),
                            D.stride(0), w.data_ptr(), J, b.data_ptr(), logits.data_ptr(), V, part.data_ptr(),
                            ops.stream())
    lib.ea_rnnt_step_select(n, V, k, logits.data_ptr(), V, part.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                            top.data_ptr(), ids.data_ptr(), 1, ops.stream())
    torch.cuda.synchronize()
    close("lse", out[0], ref["lse"], r32["lse"])
    close("lp_blank", out[1], ref["lpb"], r32["lpb"])
    close("top", top, ref["top"][:, :k], r32["top"][:, :k])
    close("logp", logits, ref["logp"], r32["logp"])
    assert torch.equal(ids.cpu().long(), ref["ids"])
