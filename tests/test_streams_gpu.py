"""The side-stream class (streams.SideStream: the weight-gradient stream and the auxiliary
stream are its two instances), the two rules in which they differ, and the scratch cache."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 1024


def _count_calls(monkeypatch, obj, name):
    calls = []
    orig = getattr(obj, name)

    def counted(*a, **k):
        calls.append(name)
        return orig(*a, **k)

    monkeypatch.setattr(obj, name, counted)
    return calls


@pytest.mark.parametrize("fork", ["current", "event"])
@pytest.mark.parametrize("which", ["wgrad", "aux"])
def test_side_stream_product_visible_after_join(which, fork, monkeypatch):
    """A tensor written on the side stream, held 300 us before its first launch, is read
    correctly on the main stream after the join: forked from the main stream's current point,
    and from an event recorded before an intervening main-stream op."""
    from espnet_amd import hip_ops as ops, streams
    from espnet_amd._lib import lib
    side = {"wgrad": streams.WGRAD, "aux": streams.AUX}[which]
    enter = {"wgrad": lambda *t, **k: ops.wgrad(*t, launches=True, **k), "aux": ops.aux}[which]
    join = {"wgrad": ops.join_wgrad, "aux": ops.join_aux}[which]
    assert side.enabled
    spins = _count_calls(monkeypatch, lib, "ea_debug_spin")
    monkeypatch.setattr(streams, "DEBUG_DELAY_NS", 300_000)
    main = torch.cuda.current_stream()
    x = torch.zeros(N, device="cuda")
    x.fill_(1.0)
    kw = {}
    if fork == "event":
        if which == "wgrad":
            kw["after"] = ops.fork_event()
        else:
            ops.mark_aux_fork()
            kw["after"] = ops.take_aux_fork()
        assert kw["after"] is not None
        other = torch.zeros(1 << 20, device="cuda").add_(3.0)  # the main stream goes on
    with enter(x, **kw):
        assert torch.cuda.current_stream() == side.streams[main.device] != main
        x.add_(1.0)
    assert torch.cuda.current_stream() == main
    join()
    got = (x * 2).cpu()
    assert len(spins) == 1
    assert torch.equal(got, torch.full((N,), 4.0))
    if fork == "event":
        assert float(other[-1]) == 3.0


def test_wgrad_fork_skipped_while_only_deferred_work_is_inside(monkeypatch):
    from espnet_amd import deferred, hip_ops as ops
    monkeypatch.setattr(deferred, "DEFER_WGRAD", True)
    monkeypatch.setattr(deferred, "DEFER_REDUCE", True)
    main = torch.cuda.current_stream()
    x = torch.zeros(N, device="cuda")
    with ops.deferred_wgrad():
        assert ops.WGRAD_Q.active and ops.REDUCE_Q.active
        with ops.wgrad(x):
            assert torch.cuda.current_stream() == main and not ops.on_side()
        with ops.wgrad(x, launches=True):
            assert torch.cuda.current_stream() != main and ops.on_side()
        # one queue alone does not skip the fork
        ops.REDUCE_Q.active = False
        with ops.wgrad(x):
            assert ops.on_side()
        ops.REDUCE_Q.active = True
    with ops.wgrad(x):  # outside a deferred pass the block launches its kernels itself
        assert ops.on_side()
    ops.join_wgrad()


def test_wgrad_joins_only_when_forked_and_aux_always(monkeypatch):
    from espnet_amd import hip_ops as ops, streams
    dev = torch.cuda.current_stream().device
    x = torch.zeros(N, device="cuda")
    with ops.wgrad(x, launches=True):
        x.add_(1.0)
        ops.WGRAD_Q.side_events.append(torch.cuda.Event())
    with ops.aux(x):
        pass
    waits = _count_calls(monkeypatch, torch.cuda.Stream, "wait_stream")
    assert streams.WGRAD.dirty[dev] is True
    ops.join_wgrad()
    assert streams.WGRAD.dirty[dev] is False and len(waits) == 1 and ops.WGRAD_Q.side_events == []
    ops.join_wgrad()  # not forked since the last join: no wait, no graph edge
    assert streams.WGRAD.dirty[dev] is False and len(waits) == 1
    ops.join_aux()
    ops.join_aux()  # the auxiliary stream has no such rule
    assert len(waits) == 3
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0


def test_scratch_cache():
    from espnet_amd import hip_ops as ops, streams
    dev = torch.device("cuda", torch.cuda.current_device())
    for tag, dtype, floor in [("splitk", torch.float32, 1 << 20), ("ggemm", torch.uint8, 1 << 16),
                              ("colsum", torch.uint8, 1 << 16), ("reduce", torch.uint8, 1 << 16),
                              ("f32", torch.float32, 1 << 22)]:
        t = streams.scratch(tag, 1, dev)
        assert t.dtype == dtype and t.numel() >= floor and t.device == dev
    a = streams.scratch("colsum", 100, dev)
    assert streams.scratch("colsum", a.numel(), dev).data_ptr() == a.data_ptr()
    assert streams.scratch("colsum", 1, dev).data_ptr() == a.data_ptr()
    b = streams.scratch("reduce", 100, dev)
    assert b.data_ptr() != a.data_ptr()  # two tags on one stream
    with ops.wgrad(launches=True):
        s = streams.scratch("colsum", 100, dev)
        assert s.data_ptr() not in (a.data_ptr(), b.data_ptr())  # the side stream's own buffer
        assert streams.scratch("colsum", 100, dev).data_ptr() == s.data_ptr()
    ops.join_wgrad()
    big = streams.scratch("colsum", a.numel() + 1, dev)  # only grows
    assert big.numel() > a.numel()
    assert streams.scratch("colsum", 100, dev).data_ptr() == big.data_ptr()
    assert ops.splitk_ws(dev).numel() >= ops.SPLITK_WS
    p, n = ops.f32_ws(dev, 5)
    assert n >= 1 << 22 and p == streams.scratch("f32", 1, dev).data_ptr()
