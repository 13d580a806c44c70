"""Tensor-level launchers for the HIP kernels in libespnet_amd.so.

Torch tensors are used only as device-memory handles (data_ptr / shape / stride) and for
the current HIP stream; every computation is one of the library's kernels.

The side streams and scratch buffers (streams.py) and the deferred weight-gradient /
reduction queues (deferred.py) are re-exported here for the `ops.<name>` call sites.  Their
switches live there and nowhere else: `ops.<switch>` (_MOVED) reads and assigns the one in
its home module, so no copy here can go unread.
"""
from __future__ import annotations

import ctypes
import os
import sys
import types
import weakref

import torch

from . import deferred, streams
from ._lib import ACT_NONE, EPI_STORE, Epilogue, HipError, dt, lib
from .deferred import (REDUCE_Q, WGRAD_Q, deferred_tensors, deferred_wgrad, flush_deferred,  # noqa: F401
                       flush_wgrad_side, fork_event, grad_ready, join_wgrad, wgrad)
from .streams import aux, join_aux, mark_aux_fork, on_side, scratch, stream, take_aux_fork  # noqa: F401

_MOVED = {**dict.fromkeys(("DEBUG_DELAY_NS", "DEBUG_SERIAL", "OVERLAP_CTC_BWD"), streams),
          **dict.fromkeys(("GRAD_READY", "DEFER_WGRAD", "DEFER_REDUCE", "DEFER_BUDGET"), deferred)}


class _Ops(types.ModuleType):
    def __getattr__(self, name):  # (only names this module does not define itself)
        if name in _MOVED:
            return getattr(_MOVED[name], name)
        raise AttributeError(f"module {self.__name__!r} has no attribute {name!r}")

    def __setattr__(self, name, value):
        if name in _MOVED:
            setattr(_MOVED[name], name, value)
        else:
            super().__setattr__(name, value)


sys.modules[__name__].__class__ = _Ops


class KernelProbe:
    """Measures named GEMM launches from inside the kernel (bench.py): the launch stamps its
    first-block start and last-block end on the GPU's constant 100 MHz clock
    (ea_gemm_set_probe); stream-ordered begin/end kernels accumulate the span, so a launch
    captured into a hipGraph is re-measured on every replay."""

    TICK_MS = 1e-5  # s_memrealtime: 100 MHz

    def __init__(self, names, device=None):
        self.names = set(names)
        dev = device or torch.device("cuda", torch.cuda.current_device())
        self.slots = {n: torch.zeros(4, dtype=torch.int64, device=dev) for n in names}
        self.active = True

    def begin(self, name):
        if self.active and name in self.names:
            s = self.slots[name].data_ptr()
            lib.ea_probe_begin(s, stream())
            lib.ea_gemm_set_probe(s)

    def end(self, name):
        if self.active and name in self.names:
            lib.ea_gemm_set_probe(None)
            lib.ea_probe_end(self.slots[name].data_ptr(), stream())

    def reset(self):
        for t in self.slots.values():
            t.zero_()

    def mean_ms(self, name):
        tot, cnt = (int(x) for x in self.slots[name][2:4].tolist())
        return (tot / cnt * self.TICK_MS if cnt else float("nan")), cnt


class EventProbe:
    """The same begin/end interface as KernelProbe, timed with HIP events recorded on the
    launch stream around the named launch (eager launches only: not inside a graph capture).
    bench.py reports it beside the in-kernel probe and the rocprof average."""

    def __init__(self, names):
        self.names = set(names)
        self.pairs = {n: [] for n in names}
        self.active = True

    def begin(self, name):
        if self.active and name in self.names:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(torch.cuda.current_stream())
            self.pairs[name].append([ev, None])

    def end(self, name):
        if self.active and name in self.names:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(torch.cuda.current_stream())
            self.pairs[name][-1][1] = ev

    def reset(self):
        for v in self.pairs.values():
            v.clear()

    def mean_ms(self, name):
        torch.cuda.synchronize()
        ts = [a.elapsed_time(b) for a, b in self.pairs[name] if b is not None]
        return (sum(ts) / len(ts) if ts else float("nan")), len(ts)


PROBE = None


def ptr(t):
    return None if t is None else t.data_ptr()


SPLITK_WS = 1 << 25  # 32M floats


def splitk_ws(device) -> torch.Tensor:
    """The current stream's f32 split-K workspace (SPLITK_WS elements)."""
    return scratch("splitk", SPLITK_WS, device)


def f32_ws(device, numel=1 << 22):
    """(pointer, elements) of the current stream's f32 scratch, at least `numel` elements."""
    w = scratch("f32", numel, device)
    return w.data_ptr(), w.numel()


def make_epi(kind=EPI_STORE, *, alpha=1.0, beta=0.0, bias=None, post_scale=1.0, act=ACT_NONE,
             aux=None, resid=None, rscale=1.0, drop_p=0.0, seed=0):
    e = Epilogue()
    e.kind = kind
    e.act = act
    e.alpha = alpha
    e.beta = beta
    e.post_scale = post_scale
    e.rscale = rscale
    e.drop_p = drop_p
    e.seed = seed & 0xFFFFFFFFFFFFFFFF
    e.bias = ptr(bias)
    if aux is not None:
        e.aux = aux.data_ptr()
        e.aux_dtype = dt(aux)
        e.ldaux = aux.stride(-2)
    if resid is not None:
        e.resid = resid.data_ptr()
        e.ldr = resid.stride(-2)
    return e


MN_TAIL_COPIES = 0  # operands re-homed by _mn_tail_guard (tests read it)


def _mn_tail_guard(X, MN, K, ld, s, batch, nh):
    """ea_gemm's contract for an MN-major bf16 operand whose width MN is not a multiple of 8
    (include/espnet_amd.h): the LDS-DMA loads move whole 16-B chunks, so the last chunk of a
    row reads up to 7 elements past MN — every row, the last one included, must be readable to
    MN rounded up to 8.  A view ending closer than that to the end of its storage (a
    column-offset slice at the end of an allocation) is copied, with its strides, into a
    buffer padded by 8 elements; the GEMM then reads the copy."""
    global MN_TAIL_COPIES
    if X.dtype != torch.bfloat16 or MN % 8 == 0 or K <= 0:
        return X
    esz = X.element_size()
    total = X.untyped_storage().nbytes() // esz
    off = X.storage_offset()
    last = off + (batch - 1) * s[0] + (nh - 1) * s[1] + (K - 1) * ld  # start of the last row read
    if last + (MN + 7) // 8 * 8 <= total:
        return X
    span = last + MN - off
    buf = torch.empty(span + 8, dtype=X.dtype, device=X.device)
    buf[:span].copy_(torch.as_strided(X, (span,), (1,), off))  # same strides from the new base
    buf[span:].zero_()
    MN_TAIL_COPIES += 1
    return buf


def gemm(A, B, C, *, M, N, K, a_kmajor, b_kmajor, lda, ldb, ldc,
         batch=1, nh=1, sA=(0, 0), sB=(0, 0), sC=(0, 0), epi: Epilogue = None, splitk=True):
    """Raw batched GEMM (see include/espnet_amd.h: ea_gemm).  An MN-major bf16 operand whose
    last row cannot be read to its width rounded up to 8 is re-homed first (_mn_tail_guard)."""
    if A.dtype != B.dtype:
        raise HipError(f"gemm operand dtypes differ: {A.dtype} vs {B.dtype}")
    if epi is None:
        epi = make_epi()
    if not a_kmajor:
        A = _mn_tail_guard(A, M, K, lda, sA, batch, nh)
    if not b_kmajor:
        B = _mn_tail_guard(B, N, K, ldb, sB, batch, nh)
    ws = splitk_ws(A.device) if splitk else None
    lib.ea_gemm(dt(A), int(a_kmajor), int(b_kmajor), M, N, K,
                A.data_ptr(), lda, sA[0], sA[1],
                B.data_ptr(), ldb, sB[0], sB[1],
                batch, nh,
                C.data_ptr(), dt(C), ldc, sC[0], sC[1],
                ctypes.byref(epi), ptr(ws), 0 if ws is None else ws.numel(), stream())
    return C


def _rows(x):
    """(…, K) tensor with unit inner stride -> (rows, K, ld)."""
    if x.stride(-1) != 1:
        raise HipError("inner dimension must be contiguous")
    K = x.shape[-1]
    rows = x.numel() // K if K else 0
    ld = x.stride(-2) if x.dim() >= 2 else K
    if x.dim() > 2:
        # leading dims must collapse onto a single row stride
        exp = ld
        for d in range(x.dim() - 2, 0, -1):
            exp *= x.shape[d]
            if x.shape[d - 1] > 1 and x.stride(d - 1) != exp:
                raise HipError("leading dims do not collapse onto one row stride")
    return rows, K, ld


def linear(x, w, out, *, epi: Epilogue = None):
    """out[r, n] = epi(sum_k x[r, k] * w[n, k]) — torch.nn.Linear forward."""
    M, K, lda = _rows(x)
    N = w.shape[0]
    _, _, ldc = _rows(out)
    return gemm(x, w, out, M=M, N=N, K=K, a_kmajor=1, b_kmajor=1, lda=lda, ldb=w.stride(0),
                ldc=ldc, epi=epi)


# ----------------------------------------------------------------------------- transposed shadow
# The Linear input gradient dX = dY . W has N = K_in: for K_in <= 512 it runs on the narrow
# 64x128 / 32x128 tiles, where W read MN-major (128-wide panels, transposed LDS reads) costs
# about a third of the launch.  A bf16 W^T copy per such weight, rewritten by one grouped
# transpose after every optimizer step (and shadow refresh), lets those GEMMs read both
# operands K-major.  EA_WT_SHADOW=0 turns it off (A/B).
WT_SHADOW = os.environ.get("EA_WT_SHADOW", "1") != "0"
WT_MAX_KIN = 512  # 2048-wide inputs too measured neutral (round 4): the FFN w_2 epilogue sets its time
TSHADOWS = {}  # arena shadow storage pointer -> weakref(TransposedShadow) (the arena owns it)


class TransposedShadow:
    def __init__(self, shadow):
        self.shadow = shadow  # the arena's bf16 weight shadow (flat)
        self.items = {}  # (element offset, R, C) -> (C, R) bf16 tensor
        self.tiles = self.probs = None
        self.ntiles = 0
        # set once a hipGraph captured refresh(): that graph holds this tile / problem table
        # and its count, so no weight may be registered afterwards (its W^T would never be
        # refreshed by the graph, and a rebuilt table would free the captured one) — such a
        # weight keeps the MN-major path instead
        self.frozen = False

    def _rebuild(self):
        probs, tiles = [], []
        for pi, ((off, R, C), dst) in enumerate(self.items.items()):
            probs.append((off, dst.data_ptr(), R | (C << 32)))
            tiles += [(pi, tr, tc, 0) for tr in range((R + 63) // 64) for tc in range((C + 63) // 64)]
        dev = self.shadow.device
        self.probs = torch.tensor(probs, dtype=torch.int64).to(dev)
        self.tiles = torch.tensor(tiles, dtype=torch.int32).to(dev)
        self.ntiles = len(tiles)

    def get(self, w):
        """W^T (C x R, row-major) of a contiguous (R x C) view of the shadow, created (and
        transposed from the current shadow) on first use."""
        off = (w.data_ptr() - self.shadow.data_ptr()) // w.element_size()
        key = (off, int(w.shape[0]), int(w.shape[1]))
        wt = self.items.get(key)
        if wt is None:
            if self.frozen or torch.cuda.is_current_stream_capturing():
                return None  # registration happens in the eager warm-up steps
            wt = torch.empty(key[2], key[1], dtype=w.dtype, device=w.device)
            self.items[key] = wt
            self._rebuild()
            self.refresh()
        return wt

    def refresh(self):
        if torch.cuda.is_current_stream_capturing():
            self.frozen = True
        if self.ntiles:
            lib.ea_transpose_bf16_grouped(self.ntiles, self.tiles.data_ptr(), self.probs.data_ptr(),
                                          self.shadow.data_ptr(), stream())


def attach_transposed_shadow(shadow):
    """Register an arena's bf16 shadow for transposed copies (returns the registry, or None)."""
    if not WT_SHADOW or shadow is None or shadow.dtype != torch.bfloat16:
        return None
    ts = TransposedShadow(shadow)
    TSHADOWS[shadow.untyped_storage().data_ptr()] = weakref.ref(ts)
    return ts


def _transposed(w):
    if not TSHADOWS or w.dtype != torch.bfloat16 or w.dim() != 2 or w.shape[1] > WT_MAX_KIN:
        return None
    if w.stride(1) != 1 or w.stride(0) != w.shape[1] or w.shape[0] % 8 or w.shape[1] % 8:
        return None
    ref = TSHADOWS.get(w.untyped_storage().data_ptr())
    ts = None if ref is None else ref()
    if ts is None or ts.shadow.untyped_storage().data_ptr() != w.untyped_storage().data_ptr():
        return None
    return ts.get(w)


def linear_dx(dy, w, out, *, epi: Epilogue = None):
    """out[r, k] = epi(sum_n dy[r, n] * w[n, k]) — Linear input gradient (W^T K-major from the
    transposed shadow when the arena keeps one for w)."""
    M, N, lda = _rows(dy)
    K = w.shape[1]
    _, _, ldc = _rows(out)
    wt = _transposed(w)
    if wt is not None:
        return gemm(dy, wt, out, M=M, N=K, K=N, a_kmajor=1, b_kmajor=1, lda=lda, ldb=wt.stride(0),
                    ldc=ldc, epi=epi)
    return gemm(dy, w, out, M=M, N=K, K=N, a_kmajor=1, b_kmajor=0, lda=lda, ldb=w.stride(0),
                ldc=ldc, epi=epi)


def linear_dw(dy, x, dw, *, accumulate=False, post=None, db=None, db_accumulate=True):
    """dw[n, k] (+)= sum_r dy[r, n] * x[r, k] — Linear weight gradient (f32 out).  While the
    weight-gradient queue is active (a training backward pass) the GEMM is deferred and
    launched with the others of the pass by WGRAD_Q.flush(); `post` (a callable consuming dw,
    e.g. a permute into the gradient arena) then runs right after that launch.
    db: the Linear's bias gradient, db (+)= column sums of dy (db_accumulate, colsum's default).
    The queued GEMM sums it from its dy operand (ea_group_gemm.a_sum) when it can; otherwise —
    queue off or problem not taken, f32 dy, EA_WGRAD_BIAS=0 — colsum(dy, db) runs as before."""
    R, N, lddy = _rows(dy)
    R2, K, ldx = _rows(x)
    if R != R2:
        raise HipError("row mismatch in linear_dw")
    beta = 1.0 if accumulate else 0.0
    took = WGRAD_Q.active and WGRAD_Q.add(dy, x, dw, M=N, N=K, K=R, lda=lddy, ldb=ldx, ldc=dw.stride(0), beta=beta,
                                          post=post, db=db, db_beta=1.0 if db_accumulate else 0.0)
    if db is not None and took != "db":
        colsum(dy, db, accumulate=db_accumulate)
    if took:
        return dw
    gemm(dy, x, dw, M=N, N=K, K=R, a_kmajor=0, b_kmajor=0, lda=lddy, ldb=ldx,
         ldc=dw.stride(0), epi=make_epi(beta=beta))
    if post is not None:
        post()
    return dw


# ----------------------------------------------------------------------------- norms
def layernorm_fwd(x, gamma, beta, y, mean, rstd, eps=1e-12):
    rows, d, ldx = _rows(x)
    lib.ea_layernorm_fwd(rows, d, x.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), eps,
                         y.data_ptr(), dt(y), y.stride(-2) if y.dim() > 1 else d,
                         mean.data_ptr(), rstd.data_ptr(), stream())


def linear_ln(x, gamma, beta, w, out, *, epi=None, eps=1e-12):
    """out = epi(LayerNorm(x) . w^T) in one launch (ea_gemm_ln): x f32 (rows, K), w bf16
    (N, K); the normalised rows are rounded to bf16 as the unfused LayerNorm stores them."""
    rows, K, ldx = _rows(x)
    N = w.shape[0]
    if epi is None:
        epi = make_epi()
    lib.ea_gemm_ln(rows, N, K, x.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), ctypes.c_float(eps),
                   w.data_ptr(), w.stride(0), out.data_ptr(), dt(out), out.stride(0), ctypes.byref(epi), stream())
    return out


def layernorm_bwd(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, accumulate=True, drop=None):
    """drop=(y, scale, p, seed[, ycol]): also y = dropout(scale * dx) once dx is final (the next
    residual site's dropout backward, ea_layernorm_bwd_drop), instead of an ea_scale_dropout
    pass; ycol (+)= column sums of y (that site's bias gradient) from the same kernel."""
    rows, d, ldx = _rows(x)
    _, _, lddy = _rows(dy)
    _, _, lddx = _rows(dx)
    if drop is not None:
        y, ysc, yp, yseed = drop[:4]
        ycol = drop[4] if len(drop) > 4 else None
        _, _, ldy = _rows(y)
        dargs = (y.data_ptr(), dt(y), ldy, float(ysc), float(yp), yseed & 0xFFFFFFFFFFFFFFFF,
                 0 if ycol is None else ycol.data_ptr())
    if REDUCE_Q.active and rows > 0 and dbeta.data_ptr() == dgamma.data_ptr() + 4 * d:
        # dx now; the (dgamma | dbeta) row-block partials go to a buffer of their own and are
        # summed with the pass's other parameter-gradient reductions (REDUCE_Q.flush)
        # the vectorized kernel's block count (16-row blocks; ln_bwd_impl), the generic paths'
        # at most 128 blocks
        vec8 = (d % 8 == 0 and d <= 1024 and lddy % 8 == 0 and ldx % 4 == 0 and lddx % 4 == 0
                and x.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0 and dx.data_ptr() % 16 == 0
                and gamma.data_ptr() % 16 == 0)
        nparts_max = (rows + 15) // 16 if vec8 else max((rows + 15) // 16, 128)
        part = torch.empty(nparts_max * (3 if drop is not None else 2) * d, dtype=torch.float32, device=x.device)
        np_ = ctypes.c_int(0)
        if drop is not None:
            yparts = ctypes.c_int(0)
            lib.ea_layernorm_bwd_partials_drop(rows, d, dy.data_ptr(), dt(dy), lddy, x.data_ptr(), ldx,
                                               gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                               lddx, int(accumulate), part.data_ptr(), part.numel(),
                                               ctypes.addressof(np_), *dargs, ctypes.addressof(yparts), stream())
            if yparts.value:
                npv = np_.value
                REDUCE_Q.add_reduce(part[npv * 2 * d:], npv, d, d, ycol, accumulate=True)
        else:
            lib.ea_layernorm_bwd_partials(rows, d, dy.data_ptr(), dt(dy), lddy, x.data_ptr(), ldx, gamma.data_ptr(),
                                          mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), lddx, int(accumulate),
                                          part.data_ptr(), part.numel(), ctypes.addressof(np_), stream())
        REDUCE_Q.add_reduce(part, np_.value, 2 * d, 2 * d, dgamma, accumulate=True)
        return
    w, n = f32_ws(x.device, max(1 << 22, 1024 * d))
    if drop is not None:
        lib.ea_layernorm_bwd_drop(rows, d, dy.data_ptr(), dt(dy), lddy, x.data_ptr(), ldx, gamma.data_ptr(),
                                  mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), lddx, int(accumulate),
                                  dgamma.data_ptr(), dbeta.data_ptr(), 1, w, n, *dargs, stream())
        return
    lib.ea_layernorm_bwd(rows, d, dy.data_ptr(), dt(dy), lddy, x.data_ptr(), ldx, gamma.data_ptr(),
                         mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), lddx, int(accumulate),
                         dgamma.data_ptr(), dbeta.data_ptr(), 1, w, n, stream())


def reduce_rows(part, nparts, n, stride, out, accumulate=True):
    """out[c] (+)= sum_p part[p*stride + c], p in fixed order (deterministic); deferred with the
    pass's other parameter-gradient reductions while the reduction queue is active."""
    if REDUCE_Q.active:
        REDUCE_Q.add_reduce(part, nparts, n, stride, out, accumulate)
        return
    lib.ea_reduce_partials(nparts, n, part.data_ptr(), stride, out.data_ptr(), int(accumulate), stream())


def colsum(x, out, accumulate=True, defer=True):
    """out (+)= column sums of x.  While the reduction queue is active the sum is deferred to
    REDUCE_Q.flush(): pass defer=False when x is modified in place before the pass ends."""
    rows, n, ld = _rows(x)
    if defer and REDUCE_Q.active and REDUCE_Q.add_colsum(x, rows, n, ld, out, accumulate):
        return
    w, wn = f32_ws(x.device)
    lib.ea_colsum(rows, n, x.data_ptr(), dt(x), ld, out.data_ptr(), int(accumulate), w, wn, stream())


def batchnorm_fwd(y, gamma, beta, mean, rstd, run_mean, run_var, nbt, z, training, act,
                  eps=1e-5, momentum=0.1):
    rows, C, _ = _rows(y)
    w, wn = f32_ws(y.device, (min(rows // 16 + 1, 256) + 2) * 2 * C)
    lib.ea_batchnorm_fwd(rows, C, y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, momentum,
                         int(training), mean.data_ptr(), rstd.data_ptr(), ptr(run_mean), ptr(run_var),
                         ptr(nbt), act, z.data_ptr(), dt(z), w, wn, stream())


def batchnorm_bwd(dz, y, mean, rstd, gamma, beta, act, dy, dgamma, dbeta):
    rows, C, _ = _rows(y)
    w, wn = f32_ws(y.device, (min(rows // 16 + 1, 256) + 2) * 2 * C)
    lib.ea_batchnorm_bwd(rows, C, dz.data_ptr(), dt(dz), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                         gamma.data_ptr(), beta.data_ptr(), act, dy.data_ptr(), dgamma.data_ptr(),
                         dbeta.data_ptr(), 1, w, wn, stream())


# ----------------------------------------------------------------------------- elementwise
def scale_dropout(x, y, scale=1.0, p=0.0, seed=0):
    rows, cols, ldx = _rows(x)
    _, _, ldy = _rows(y)
    lib.ea_scale_dropout(rows, cols, x.data_ptr(), dt(x), ldx, y.data_ptr(), dt(y), ldy,
                         float(scale), float(p), seed & 0xFFFFFFFFFFFFFFFF, stream())
    return y


def scale_dropout_colsum(x, y, out, scale=1.0, p=0.0, seed=0, accumulate=True):
    """y = dropout(scale * x) and out (+)= column sums of y: the two-pass form (ea_scale_dropout,
    then ea_colsum on the weight-gradient side stream).  The one-pass kernel
    (ea_scale_dropout_colsum) puts the reduction on the backward's critical path and measured
    slower on MI355X (C3: 27.43-28.07 vs 27.26 ms/step, round 1)."""
    scale_dropout(x, y, scale=scale, p=p, seed=seed)
    with wgrad(y):
        colsum(y, out, accumulate=accumulate)
    return y


def cast(x, dtype):
    """Copy-convert (f32 <-> bf16) through ea_scale_dropout; returns x if already dtype."""
    if x.dtype == dtype:
        return x
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    scale_dropout(x.reshape(-1, x.shape[-1]), y.view(-1, y.shape[-1]))
    return y


def permute3(src, dst, A, Bd, Cd, accumulate=False):
    lib.ea_permute3(A, Bd, Cd, src.data_ptr(), dt(src), dst.data_ptr(), dt(dst), int(accumulate), stream())
