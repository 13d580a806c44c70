"""The side HIP streams of the training step and the stream-ordered scratch buffers.

Two side streams overlap work with the main stream: WGRAD (weight-gradient GEMMs, bias column
sums, under data parallelism the bucket all-reduces) and AUX (latency-bound work such as the
CTC lattice).  Every fork onto either, and every join, goes through SideStream.
"""
from __future__ import annotations

import contextlib
import os

import torch

from ._lib import lib

# Stream-ordering diagnostics (tests/test_dp_streams_gpu.py): EA_DEBUG_DELAY_NS holds every side /
# auxiliary stream segment for that long before its first launch (ea_debug_spin), so a consumer
# that misses its dependency on a side-stream producer reads stale data in every run;
# EA_DEBUG_SERIAL=1 makes the main stream join the side / auxiliary stream at the end of every
# segment (the overlap keeps its launch order but nothing runs concurrently).  Read at call time.
DEBUG_DELAY_NS = int(os.environ.get("EA_DEBUG_DELAY_NS", "0"))
DEBUG_SERIAL = os.environ.get("EA_DEBUG_SERIAL", "0") != "0"


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class SideStream:
    """A side HIP stream per device, created on first use.  Calling the object gives a context
    whose launches run on the side stream, ordered after everything the main (current) stream
    has issued so far or, with `after=event`, only after that event (fork_point); `join()`
    makes the main stream wait for them.  The tensors it is given are record_stream()-ed so
    the caching allocator does not recycle them under the side stream.

    `enabled` False (or no GPU: the gloo DP tests) leaves everything on the current stream.
    `lazy_join`: join() adds no dependency — in a captured step, no graph edge — when the
    stream was not forked since the last join."""

    def __init__(self, enabled: bool, lazy_join: bool):
        self.enabled = enabled
        self.lazy_join = lazy_join
        self.streams = {}  # device -> torch.cuda.Stream
        self.dirty = {}  # device -> forked since the main stream last joined

    @contextlib.contextmanager
    def __call__(self, *tensors, after=None):
        if not self.enabled or not torch.cuda.is_available():
            yield
            return
        main = torch.cuda.current_stream()
        dev = main.device
        side = self.streams.get(dev)
        if side is None:
            side = self.streams[dev] = torch.cuda.Stream(device=dev)
        if after is not None:
            side.wait_event(after)
        else:
            side.wait_stream(main)
        self.dirty[dev] = True
        for t in tensors:
            if t is not None:
                t.record_stream(side)
        with torch.cuda.stream(side):
            if DEBUG_DELAY_NS:
                lib.ea_debug_spin(DEBUG_DELAY_NS, side.cuda_stream)
            yield
        if DEBUG_SERIAL:
            main.wait_stream(side)

    def fork_point(self):
        """An event at the current stream's present point for a later fork with `after=`
        (None while the stream is off)."""
        if not self.enabled or not torch.cuda.is_available():
            return None
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        return ev

    def join(self):
        """The current (main) stream waits for all work issued on the side stream so far."""
        if not self.streams:
            return
        main = torch.cuda.current_stream()
        side = self.streams.get(main.device)
        if side is None or (self.lazy_join and not self.dirty[main.device]):
            return
        main.wait_stream(side)
        self.dirty[main.device] = False

    def is_current(self) -> bool:
        if not self.streams or not torch.cuda.is_available():
            return False
        cur = torch.cuda.current_stream()
        side = self.streams.get(cur.device)
        return side is not None and cur == side


# weight-gradient GEMMs / bias reductions, off the backward critical path (EA_OVERLAP_WGRAD=0:
# serial, for profiling).  Joined once per block of the backward, where often nothing was forked
# since the last join: a join then would still be a dependency in the captured graph.
WGRAD = SideStream(os.environ.get("EA_OVERLAP_WGRAD", "1") != "0", lazy_join=True)
# latency-bound work that leaves most CUs idle (the CTC lattice: 2 workgroups per utterance)
# overlaps independent work on the auxiliary stream (EA_OVERLAP_AUX=0: serial)
AUX = SideStream(os.environ.get("EA_OVERLAP_AUX", "1") != "0", lazy_join=False)

aux = AUX
join_aux = AUX.join
on_side = WGRAD.is_current  # the current stream is the weight-gradient side stream

# the CTC head's backward (gradient kernel + ctc_lo input gradient) overlaps the attention
# decoder's backward on the auxiliary stream (EA_OVERLAP_CTC_BWD=0: serial)
OVERLAP_CTC_BWD = os.environ.get("EA_OVERLAP_CTC_BWD", "1") != "0"
_AUX_FORK = {}


def mark_aux_fork():
    """Record where the loss gradients exist on the main stream (the hybrid combination's
    backward): a backward issued later on the host can fork from this point onto the
    auxiliary stream instead of queueing behind everything issued in between."""
    ev = AUX.fork_point() if OVERLAP_CTC_BWD else None
    if ev is not None:
        _AUX_FORK[torch.cuda.current_device()] = ev


def take_aux_fork():
    """The event mark_aux_fork() recorded on this device (consumed), or None."""
    if not _AUX_FORK or not torch.cuda.is_available():
        return None
    return _AUX_FORK.pop(torch.cuda.current_device(), None)


# tag -> (element type, minimum elements)
_SCRATCH_KINDS = {
    "f32": (torch.float32, 1 << 22),  # partials / reductions shared by consecutive kernels
    "splitk": (torch.float32, 1 << 20),  # split-K slabs
    "ggemm": (torch.uint8, 1 << 16),  # ea_gemm_grouped's problem / tile tables
    "colsum": (torch.uint8, 1 << 16),  # ea_colsum_grouped's problem table
    "reduce": (torch.uint8, 1 << 16),  # ea_reduce_grouped's problem table
}
_SCRATCH = {}


def scratch(tag: str, numel: int, device) -> torch.Tensor:
    """Persistent stream-ordered scratch of at least `numel` elements, one per (device, current
    stream, tag), so the weight-gradient side stream never races the main one (and a graph
    capture's buffers come from its own pool); grows monotonically."""
    key = (str(device), stream(), tag)
    t = _SCRATCH.get(key)
    if t is None or t.numel() < numel:
        dtype, floor = _SCRATCH_KINDS[tag]
        t = _SCRATCH[key] = torch.empty(max(numel, floor), dtype=dtype, device=device)
    return t
