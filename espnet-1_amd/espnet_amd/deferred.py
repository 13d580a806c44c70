"""The deferred work of a training backward pass: Linear weight gradients (WgradQueue) and
parameter-gradient reductions (ReduceQueue), queued during the pass and launched grouped, and
the points where the main stream forks onto / joins the weight-gradient side stream for them.
"""
from __future__ import annotations

import contextlib
import ctypes
import os

import torch

from ._lib import ColsumProb, GroupGemm, ReduceProb, dt, lib
from .streams import WGRAD, on_side, scratch, stream

GRAD_READY = None  # callable(prefix): a block's parameter gradients are final (DP overlap)

DEFER_WGRAD = os.environ.get("EA_DEFER_WGRAD", "1") != "0"
# Linear bias gradients from the deferred weight-gradient GEMM's dY operand (ea_group_gemm.a_sum)
# instead of a separate column-sum pass over dY; EA_WGRAD_BIAS=0 restores the column sums (A/B)
WGRAD_BIAS = os.environ.get("EA_WGRAD_BIAS", "1") != "0"
# bytes the deferred queues may keep alive (queued operands / partial buffers) before they
# flush early: a pass whose queued dY / X / LayerNorm partials exceed it launches what it has
# and continues (C3 queues ~3.5 GB per backward, under the default)
DEFER_BUDGET = int(float(os.environ.get("EA_DEFER_BUDGET_MB", "8192")) * 2 ** 20)


def _nbytes(t):
    return t.numel() * t.element_size()


class WgradQueue:
    """The Linear weight gradients of one backward pass (linear_dw: dW (+)= dY^T X, K = the
    pass's token count), deferred and launched together as ONE grouped GEMM
    (ea_gemm_grouped: every 256x256 tile over its problem's whole K on the pipelined main
    loop) instead of one split-K GEMM + combine pass per Linear.  The queue keeps dY and X
    alive until the flush.  Problems are ordered longest-K first; a problem whose output
    overlaps a queued one flushes the queue first (a launch never holds two writers of one
    element)."""

    def __init__(self):
        self.active = False
        self.items = []
        self.posts = []
        self.pending = 0  # bytes of queued dY / X kept alive
        # events recorded on the side stream where items were queued there (their operands may
        # be side-stream products, e.g. the linear_pos GEMM's dpp) since the main stream last
        # joined it: a flush on another stream waits for them first (data parallel: no
        # per-block joins)
        self.side_events = []

    def add(self, dy, x, dw, *, M, N, K, lda, ldb, ldc, beta, post=None, db=None, db_beta=None):
        """-> False (not queued), True (queued) or "db" (queued, and the launch also writes
        db (+)= the column sums of dy, as the problem's a_sum).  db is not carried — the caller
        sums it separately — when WGRAD_BIAS is off, when it does not share dw's accumulate,
        or when its span overlaps an output REDUCE_Q has claimed (the two queues flush on
        different streams at the end of the pass)."""
        if not (dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and dw.dtype == torch.float32):
            return False
        if (lda % 8 or ldb % 8 or dy.data_ptr() % 16 or x.data_ptr() % 16 or N % 4 or ldc % 4
                or dw.data_ptr() % 16 or M <= 0 or N <= 0 or K <= 0):
            return False
        if 2.0 * K * lda >= 4.0e9 or 2.0 * K * ldb >= 4.0e9:
            return False
        lo = dw.data_ptr()
        hi = lo + ((M - 1) * ldc + N) * 4
        spans = [(lo, hi)]
        if (db is not None and WGRAD_BIAS and db_beta == beta and db.dtype == torch.float32 and db.is_contiguous()
                and db.numel() == M and db.data_ptr() % 4 == 0):
            blo = db.data_ptr()
            bhi = blo + 4 * M
            if not (blo < hi and lo < bhi) and not REDUCE_Q.claimed(blo, bhi):
                spans.append((blo, bhi))
        if any(l_ < s[1] and s[0] < h for it in self.items for s in it[-1] for l_, h in spans):
            self.flush()
        if on_side():
            ev = torch.cuda.Event()
            ev.record()
            self.side_events.append(ev)
        fused = db if len(spans) > 1 else None
        self.items.append((K, dy, x, dw, M, N, lda, ldb, ldc, beta, fused, spans))
        if post is not None:
            self.posts.append(post)
        self.pending += _nbytes(dy) + _nbytes(x)
        if self.pending > DEFER_BUDGET:
            self.flush()
        return "db" if fused is not None else True

    def carries(self, lo, hi) -> bool:
        """Does a queued problem write a bias gradient (a_sum) overlapping bytes [lo, hi)?"""
        return any(lo < s[1] and s[0] < hi for it in self.items for s in it[-1][1:])

    def flush(self):
        """Launch the queued GEMMs on the current stream."""
        if not self.items:
            return
        if self.side_events:
            if not on_side():
                cur = torch.cuda.current_stream()
                for ev in self.side_events:
                    cur.wait_event(ev)
            self.side_events = []
        items = sorted(self.items, key=lambda t: -t[0])
        posts = self.posts
        self.items = []
        self.posts = []
        self.pending = 0
        n = len(items)
        cur = torch.cuda.current_stream()
        for it in items:  # operands may come from another stream's pool: keep them until this launch ran
            for t in it[1:4]:
                t.record_stream(cur)
        arr = (GroupGemm * n)()
        ntiles = 0
        for i, (K, dy, x, dw, M, N, lda, ldb, ldc, beta, db, _) in enumerate(items):
            arr[i] = GroupGemm(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), lda, ldb, ldc, M, N, K, beta,
                               None if db is None else db.data_ptr())
            ntiles += ((M + 255) // 256) * ((N + 255) // 256)
        nbytes = ctypes.c_long(0)
        lib.ea_gemm_grouped_ws_bytes(n, ntiles, ctypes.addressof(nbytes))
        ws = scratch("ggemm", nbytes.value, items[0][1].device)
        lib.ea_gemm_grouped(0, 0, n, ctypes.addressof(arr), ws.data_ptr(), ws.numel(), stream())
        for post in posts:
            post()

    def tensors(self):
        return [t for it in self.items for t in (it[1], it[2])]


WGRAD_Q = WgradQueue()

DEFER_REDUCE = os.environ.get("EA_DEFER_REDUCE", "1") != "0"


class ReduceQueue:
    """The parameter-gradient reductions of one backward pass, deferred: bias column sums
    (colsum: torch.nn.Linear bias.grad = dY summed over tokens) and the ordered sums of the
    LayerNorm (dgamma | dbeta) row-block partials.  flush() runs every queued column sum in
    ONE grouped launch (ea_colsum_grouped), then every reduction in ONE more
    (ea_reduce_grouped) — instead of ~450 launches of a few microseconds per C3 step.  The
    column sums use ea_colsum's row blocking, so results are bit-identical to the per-call
    path.  Outputs that overlap a queued one flush the queue first."""

    def __init__(self):
        self.active = False
        self.colsums = []
        self.reduces = []
        self.spans = []
        self.pending = 0  # bytes of queued inputs / partial buffers kept alive

    def _account(self, t):
        self.pending += _nbytes(t)
        if self.pending > DEFER_BUDGET:
            self.flush()

    def claimed(self, lo, hi) -> bool:
        return any(lo < h and l_ < hi for l_, h in self.spans)

    def _claim(self, out, n):
        lo = out.data_ptr()
        hi = lo + 4 * n
        if self.claimed(lo, hi):
            self.flush()
        if WGRAD_Q.carries(lo, hi):  # a queued weight-gradient problem writes this bias: it goes first
            WGRAD_Q.flush()
        self.spans.append((lo, hi))

    def add_colsum(self, x, rows, n, ld, out, accumulate) -> bool:
        """x: rows x n with row stride ld (hip_ops.colsum)."""
        if x.dtype not in (torch.bfloat16, torch.float32) or out.dtype != torch.float32 or not out.is_contiguous():
            return False
        if rows <= 0 or n % 4 or ld % 4 or x.data_ptr() % (8 if x.dtype == torch.bfloat16 else 16):
            return False
        self._claim(out, n)
        self.colsums.append((x, rows, n, ld, out, accumulate))
        self._account(x)
        return True

    def add_reduce(self, part, nparts, n, stride, out, accumulate=True):
        self._claim(out, n)
        self.reduces.append((part, nparts, n, stride, out, accumulate))
        self._account(part)

    def tensors(self):
        return [c[0] for c in self.colsums] + [r[0] for r in self.reduces]

    def flush(self):
        if not self.colsums and not self.reduces:
            return
        colsums, reduces = self.colsums, list(self.reduces)
        self.colsums, self.reduces, self.spans = [], [], []
        self.pending = 0
        cur = torch.cuda.current_stream()
        for t in [c[0] for c in colsums] + [r[0] for r in reduces]:
            t.record_stream(cur)
        dev = (colsums[0][0] if colsums else reduces[0][0]).device
        cb, rb = ctypes.c_long(0), ctypes.c_long(0)
        if colsums:
            rpps = [max(32, (c[1] + 127) // 128) for c in colsums]  # ea_colsum's row blocking
            nrbs = [(c[1] + r - 1) // r for c, r in zip(colsums, rpps)]
            part = torch.empty(sum(nrb * c[2] for c, nrb in zip(colsums, nrbs)), dtype=torch.float32, device=dev)
            arr = (ColsumProb * len(colsums))()
            off = 0
            for i, ((x, rows, n, ld, out, acc), rpp, nrb) in enumerate(zip(colsums, rpps, nrbs)):
                arr[i] = ColsumProb(x.data_ptr(), part.data_ptr() + 4 * off, ld, rows, n, dt(x), rpp)
                reduces.append((part, nrb, n, n, out, acc, off))
                off += nrb * n
            lib.ea_grouped_table_bytes(len(colsums), ctypes.addressof(cb), ctypes.addressof(rb))
            ws = scratch("colsum", cb.value, dev)
            lib.ea_colsum_grouped(len(colsums), ctypes.addressof(arr), ws.data_ptr(), ws.numel(), stream())
        arr = (ReduceProb * len(reduces))()
        for i, r in enumerate(reduces):
            part, nparts, n, stride, out, acc = r[:6]
            off = r[6] if len(r) > 6 else 0
            arr[i] = ReduceProb(part.data_ptr() + 4 * off, out.data_ptr(), stride, nparts, n, int(acc))
        lib.ea_grouped_table_bytes(len(reduces), ctypes.addressof(cb), ctypes.addressof(rb))
        ws = scratch("reduce", rb.value, dev)
        lib.ea_reduce_grouped(len(reduces), ctypes.addressof(arr), ws.data_ptr(), ws.numel(), stream())


REDUCE_Q = ReduceQueue()


def wgrad(*tensors, after=None, launches=False):
    """Context for weight-gradient work (dW GEMMs, bias column sums) that is off the
    backward critical path: it runs on the side stream (streams.WGRAD), ordered after
    everything the main stream has issued so far, or after the event `after` (fork_event);
    join_wgrad() makes the main stream wait for it.

    While the pass's weight gradients and reductions are deferred (deferred_wgrad), a block
    of linear_dw / colsum calls only queues work, and the fork is skipped unless `launches`
    says the block launches kernels of its own: in a captured step every fork is a graph
    dependency whose event costs the main chain ~5 us even when nothing runs on the side
    (a launch inside a skipped fork simply runs on the current stream, in order)."""
    if not launches and WGRAD_Q.active and REDUCE_Q.active:
        return contextlib.nullcontext()
    return WGRAD(*tensors, after=after)


def fork_event():
    """An event at the main stream's current point for a later wgrad(after=...), or None: a
    side-stream GEMM forked from an earlier point of the main stream is issued after the main
    stream's next kernel, so in the captured graph the main chain's kernel is the first successor
    of the fork point.  Single process only: with the data-parallel hooks (GRAD_READY) the side
    stream also carries the bucket all-reduces, and the late fork measured 4% slower there
    (1811 -> 1739 utt/s in the DP rehearsal, profiles/r5_fork_after_dp_ab.txt)."""
    return None if GRAD_READY is not None else WGRAD.fork_point()


def join_wgrad():
    """Main stream waits for all weight-gradient work issued so far (nothing to wait for —
    and no graph dependency — when the side stream was not forked since the last join)."""
    WGRAD.join()
    WGRAD_Q.side_events = []  # whatever the side stream produced is ordered before main now


def grad_ready(bound):
    """A block's backward is done.  Data parallel (GRAD_READY set): the hook flushes the
    deferred weight gradients and issues the bucket all-reduces from the side stream, so the
    main stream goes on with the backward.  Single process: the main stream joins the side
    stream here, once per block (the deferred queues flush at the end of the pass; flushing
    them per block on the side stream, or joining only once per pass, measured slower:
    profiles/r3_stream_wgrad_ab.txt)."""
    if GRAD_READY is not None:
        GRAD_READY(bound.prefix)
        return
    join_wgrad()


def _side_flush_ok():
    return GRAD_READY is None and WGRAD.enabled and torch.cuda.is_available()


def flush_wgrad_side(after=None):
    """Launch the weight gradients queued so far (one grouped GEMM) on the side stream, forked
    from `after` (fork_event); single process only (the data-parallel hooks flush per bucket)."""
    if WGRAD_Q.active and WGRAD_Q.items and _side_flush_ok():
        with WGRAD(*WGRAD_Q.tensors(), after=after):
            WGRAD_Q.flush()


def flush_deferred():
    """Launch every deferred weight gradient and gradient reduction (current stream)."""
    WGRAD_Q.flush()
    REDUCE_Q.flush()


def deferred_tensors():
    return WGRAD_Q.tensors() + REDUCE_Q.tensors()


class deferred_wgrad:
    """Context of a training backward pass: linear_dw calls inside are queued
    (EA_DEFER_WGRAD=0 turns this off), so are the bias column sums and LayerNorm
    parameter-gradient reductions (EA_DEFER_REDUCE=0); all are flushed on exit, on the
    current stream."""

    def __enter__(self):
        self.prev = (WGRAD_Q.active, REDUCE_Q.active)
        WGRAD_Q.active = DEFER_WGRAD
        REDUCE_Q.active = DEFER_REDUCE
        return WGRAD_Q

    def __exit__(self, *exc):
        WGRAD_Q.active, REDUCE_Q.active = self.prev
        if exc[0] is None:
            if _side_flush_ok():
                # the pass's reductions (bias column sums, LayerNorm parameter sums: bandwidth-
                # bound) on the side stream beside the grouped weight-gradient GEMM (MFMA-bound)
                # on this one; disjoint outputs (bias / norm vs weight gradients)
                with WGRAD(*REDUCE_Q.tensors()):
                    REDUCE_Q.flush()
                WGRAD_Q.flush()
            else:
                flush_deferred()
            if GRAD_READY is None:
                join_wgrad()  # gradients written on the side stream during the pass are final
        else:
            WGRAD_Q.items, WGRAD_Q.posts = [], []
            REDUCE_Q.colsums, REDUCE_Q.reduces, REDUCE_Q.spans = [], [], []
        return False
