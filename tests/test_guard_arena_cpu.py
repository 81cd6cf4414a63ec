"""The guard-band harness (tests/_guard_arena.py) can fail: five fake "ops" in plain torch, on CPU tensors, each plant one
fault of a kind tests/test_gpu_guard_bands.py looks for -- and each is reported exactly once, with its region and byte offset.
A correct op is reported clean.  No GPU needed."""
import pytest
import torch

from _guard_arena import ALIGN, END_GUARD, GUARD, Arena, Finding, guarded_workspace

ROWS, N, LD = 5, 6, 8                      # a strided fp32 output [5, 6] with row stride 8: gap columns 6 and 7
DEVICE = "cpu"                             # tests/test_gpu_guard_bands.py runs the same planted faults on the GPU


def _setup():
    ar = Arena(DEVICE, capacity=1 << 20)
    g = torch.Generator().manual_seed(0)
    x = ar.input("x", torch.randn(ROWS, N, generator=g))
    out = ar.output("out", torch.float32, (ROWS, N), (LD, 1))
    idx = ar.output("idx", torch.int64, (7,))
    ws = ar.workspace(100)
    return ar, x, out, idx, ws


def _op(x, out, idx, ws):
    """the correct op: out = 2 x, idx = 0 .. 6, and it scribbles over all of its workspace"""
    out.copy_(2 * x)
    idx.copy_(torch.arange(7, device=idx.device))
    ws.fill_(3)


def _beyond(t, first, n=1):
    """``n`` elements of ``t``'s storage starting ``first`` elements from its first one (outside the view: what a kernel
    with a wrong index reaches)"""
    return t.as_strided((n,), (1,), t.storage_offset() + first)


def _refs(x):
    return {"out": 2 * x, "idx": torch.arange(7, device=x.device)}


def test_layout_alignment_sizes_and_fill():
    ar, x, out, idx, ws = _setup()
    starts = [r.start for r in ar.regions]
    assert all((ar.buf.data_ptr() + s) % ALIGN == 0 for s in starts)
    assert starts[0] >= END_GUARD and ar.buf.numel() - (ar.regions[-1].start + ar.regions[-1].nbytes) >= END_GUARD
    for a, b in zip(ar.regions, ar.regions[1:]):
        assert b.start - (a.start + a.nbytes) >= GUARD
    assert [r.nbytes for r in ar.regions] == [ROWS * N * 4, ((ROWS - 1) * LD + N) * 4, 56, 100]
    assert ws.numel() == 100 and out.stride() == (LD, 1) and x.is_contiguous()
    assert bool(torch.isnan(out).all()) and bool((idx == -1).all()) and bool((ws == 0xFF).all())
    lo, hi = ar.regions[1].start, ar.regions[1].start + ar.regions[1].nbytes
    assert bool((ar.buf[lo - GUARD:lo] == 0xA5).all()) and bool((ar.buf[hi + 200:hi + GUARD] == 0xA5).all())
    with pytest.raises(AssertionError):
        ar.take(10, torch.float32)                                     # not a whole number of elements
    with pytest.raises(MemoryError):
        ar.take(2 << 20)


def test_a_correct_op_has_no_findings():
    ar, x, out, idx, ws = _setup()
    _op(x, out, idx, ws)
    assert ar.check(_refs(x)) == []
    # NaN in the reference and the documented -1 padding may keep the fresh pattern
    ar, x, out, idx, ws = _setup()
    _op(x, out, idx, ws)
    out[2, 3] = float("nan")
    idx[5:] = -1
    want_out, want_idx = 2 * x, torch.arange(7, device=x.device)
    want_out[2, 3] = float("nan")
    want_idx[5:] = -1
    assert ar.check({"out": want_out, "idx": want_idx}, pad={"idx": -1}) == []
    # ... and only there
    assert ar.check({"out": want_out, "idx": want_idx}) == [Finding("unwritten", "idx", 40, 2)]


def test_store_past_an_output_is_found():
    ar, x, out, idx, ws = _setup()
    _op(x, out, idx, ws)
    _beyond(out, (ROWS - 1) * LD + N).fill_(1.0)                      # the element after the last live one
    nbytes = ar.region("out").nbytes
    assert ar.check(_refs(x)) == [Finding("guard", "out", nbytes, 4)]


def test_store_before_an_output_is_found():
    ar, x, out, idx, ws = _setup()
    _op(x, out, idx, ws)
    _beyond(idx, -1).fill_(7)
    assert ar.check(_refs(x)) == [Finding("guard", "idx", -8, 8)]


def test_store_into_a_stride_gap_is_found():
    ar, x, out, idx, ws = _setup()
    _op(x, out, idx, ws)
    _beyond(out, 2 * LD + N).fill_(0.0)                               # row 2, column N: the first gap column
    assert ar.check(_refs(x)) == [Finding("gap", "out", (2 * LD + N) * 4, 4)]


def test_an_unwritten_output_element_is_found():
    ar, x, out, idx, ws = _setup()
    keep = out[3, 4].clone()
    _op(x, out, idx, ws)
    out[3, 4] = keep                                                  # the op "forgot" it: still the fresh NaN
    assert ar.check(_refs(x)) == [Finding("unwritten", "out", (3 * LD + 4) * 4, 1)]
    assert ar.check() == []                                           # (outputs without a reference are not judged)


def test_a_changed_input_is_found_unless_declared_in_place():
    ar, x, out, idx, ws = _setup()
    _op(x, out, idx, ws)
    want = _refs(x)
    x.view(torch.int32)[1, 2] ^= -1                                   # every bit, so every byte, of one element
    assert ar.check(want) == [Finding("input", "x", (1 * N + 2) * 4, 4)]
    ar = Arena(DEVICE, capacity=1 << 20)
    y = ar.input("y", torch.ones(4, 4), in_place=True)
    y.mul_(2.0)
    assert ar.check() == []


def test_strided_input_keeps_nan_gaps_and_guarded_workspace_hands_out_exact_sizes(monkeypatch):
    from anyloc_amd import _lib
    ar = Arena("cpu", capacity=1 << 20)
    a = ar.input("a", torch.ones(3, 4), strides=(8, 1))
    assert ar.region("a").nbytes == (2 * 8 + 4) * 4 and bool(torch.isnan(_beyond(a, 4, 4)).all())
    handed = guarded_workspace(monkeypatch, ar)
    ws = _lib.workspace(1000, torch.device("cpu"), "vlad")
    ws2 = _lib.workspace(1000, torch.device("cpu"), "vlad")
    assert ws.numel() == 1000 and ws2.numel() == 1000 and ws.data_ptr() != ws2.data_ptr() and bool((ws == 0xFF).all())
    assert handed == [("vlad", 1000), ("vlad", 1000)]
    ws.fill_(0)
    assert ar.check() == []
    _beyond(ws, 1000).fill_(0)
    assert ar.check() == [Finding("guard", "workspace:vlad:1", 1000, 1)]
    # twice the bytes, and a base 16 bytes behind a 256-byte boundary
    ar = Arena("cpu", capacity=1 << 20)
    guarded_workspace(monkeypatch, ar, scale=2, skew=16)
    ws = _lib.workspace(1000, torch.device("cpu"), "topk")
    assert ws.numel() == 2000 and ws.data_ptr() % ALIGN == 16 and ar.regions[0].nbytes == 2016
    _beyond(ws, 2000).fill_(0)
    assert ar.check() == [Finding("guard", "workspace:topk:1", 2016, 1)]
