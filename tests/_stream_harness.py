"""Poison harness of tests/test_gpu_streams.py (not a test module): does an op keep the stream contract of
include/anyloc_hip.h ("Streams") -- every kernel, memset and copy of a call enqueued on the CURRENT stream?

Running an op on an idle side stream proves nothing: everything is ready in time by accident.  Here a mis-ordered access
READS POISON:

  1. reference   want = op(inputs) on the default stream (run twice: the second run is timed on the host, ``t_enqueue``,
                 and must reproduce the first bit for bit);
  2. poison      every device input gets a NaN twin (0x7f bytes for uint8, -1 for integers), the real values wait in
                 pinned host memory; the allocator's free blocks of the side stream are NaN too (the cache is emptied,
                 NaN blocks larger than anything the op allocates are filled and freed again, the library's per-stream
                 workspaces are dropped), so outputs, temporaries and workspaces of the op start as NaN;
  3. producer    on a side stream: a bounded chain of ``torch.mm`` (the delay, measured with events on that stream: at least
                 10 x t_enqueue and 20 ms), then the non-blocking host-to-device copies of the real values into the twins,
                 then an event -- and immediately, without a host sync, got = op(twins); ``pending`` = that event has not
                 happened when the call returns;
  4. verdict     after the stream is drained: got == want bit for bit (NaN == NaN).  Whatever the op ran on another stream,
                 or before its inputs, has read NaN or left NaN.

An ASYNCHRONOUS op must come back ``pending``: that proves both that the case was conclusive and that the call did not wait
for the device.  A case that is not pending runs ONCE more with twice the delay (logged); then it fails as inconclusive.
"""
import math
import time

import torch

MIN_DELAY_MS = 20.0
DELAY_FACTOR = 10.0
LOG = []                    # one dict per finished case: name, t_enqueue_ms, delay_ms, pending, reruns
_state = {}


def _streams():
    """The two side streams every case shares (with the default stream: three alive at most)."""
    if "streams" not in _state:
        _state["streams"] = (torch.cuda.Stream(), torch.cuda.Stream())
    return _state["streams"]


class _Delay:
    """A bounded chain of large matrix products on scratch matrices: the only thing a side stream runs in front of the copies."""
    N = 4096

    def __init__(self):
        g = torch.Generator(device="cuda").manual_seed(0)
        self.a = torch.randn(self.N, self.N, device="cuda", generator=g) / math.sqrt(self.N)
        self.out = [torch.empty_like(self.a) for _ in range(2)]
        for _ in range(3):
            torch.mm(self.a, self.a, out=self.out[0])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(8):
            torch.mm(self.a, self.a, out=self.out[0])
        e1.record()
        torch.cuda.synchronize()
        self.ms_per_mm = max(e0.elapsed_time(e1) / 8.0, 1e-3)

    def enqueue(self, ms, lane=0):
        """~``ms`` of work on the current stream -> (start, stop) timing events around it."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(int(math.ceil(1.25 * ms / self.ms_per_mm)) + 1):
            torch.mm(self.a, self.a, out=self.out[lane])
        e1.record()
        return e0, e1


def _delay():
    if "delay" not in _state:
        _state["delay"] = _Delay()
        # the matrix products of BOTH side streams once, untimed: the BLAS workspace of a stream is allocated on first use
        for lane, s in enumerate(_streams()):
            with torch.cuda.stream(s):
                _state["delay"].enqueue(1.0, lane)
        torch.cuda.synchronize()
    return _state["delay"]


def flat(out):
    """The tensors of an op's result, in order (tuples / lists are flattened, None dropped)."""
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [out]
    res = []
    for o in out:
        res += flat(o)
    return res


def same_bits(a, b):
    """torch.equal with NaN == NaN at equal positions."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.cpu(), b.cpu()
    if a.is_floating_point():
        return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())
    return torch.equal(a, b)


def _poison_value(t):
    if t.is_floating_point():
        return float("nan")
    return 0x7f if t.dtype == torch.uint8 else -1


def _poison_twin(t):
    return torch.full_like(t, _poison_value(t))


def _poison_allocator(streams, nbytes):
    """Every free block the caching allocator can hand to an allocation on ``streams`` holds NaN: the cache is emptied, then a
    large block and a run of small ones (the allocator keeps separate pools below 1 MiB) are filled and freed again."""
    from anyloc_amd import _lib
    _lib.release_workspaces()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    for s in streams:
        with torch.cuda.stream(s):
            big = torch.full((int(nbytes) // 4,), float("nan"), dtype=torch.float32, device="cuda")
            small = [torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
                     for n in (128, 1 << 10, 1 << 13, 1 << 16, 1 << 17) for _ in range(6)]
            del big, small
    torch.cuda.synchronize()


def _is_dev(t):
    return isinstance(t, torch.Tensor) and t.is_cuda


def _host_copy(t):
    """The real values of a device input in pinned host memory (None: nothing to restore)."""
    return t.detach().cpu().pin_memory() if _is_dev(t) and t.numel() else None


def tags_of(op, inputs):
    """The profiler tags ({tag: launches}) of one call of ``op`` on the default stream (which path served the shape)."""
    from anyloc_amd import ops
    torch.cuda.synchronize()
    ops.profile_enable(True)
    ops.profile_reset()
    try:
        op(*inputs)
        torch.cuda.synchronize()
        prof = ops.profile_dump()
    finally:
        ops.profile_enable(False)
        ops.profile_reset()
    return {k: int(v["calls"]) for k, v in prof.items()}


def _reference(op, inputs):
    """-> (want, t_enqueue in ms): the default-stream result, and the host time of a second call that must reproduce it."""
    torch.cuda.synchronize()
    want = flat(op(*inputs))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    again = op(*inputs)
    t_enqueue = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    again = flat(again)
    assert len(again) == len(want) and all(same_bits(a, w) for a, w in zip(again, want)), \
        "the op does not reproduce its own bits on the default stream"
    return want, t_enqueue


def run_case(name, op, inputs, asynchronous, in_place=False, poison_bytes=256 << 20):
    """One op on a side stream behind a delayed producer (module docstring).  ``inputs``: the op's positional arguments;
    device tensors among them are poisoned, everything else is passed through.  ``in_place``: the op reads the GIVEN
    tensors through pointers taken earlier (a built model): they are poisoned and restored themselves instead of twins.
    ``asynchronous``: the op is in ASYNC_OPS -- it must return while its inputs are still pending."""
    inputs = list(inputs)
    want, t_enqueue = _reference(op, inputs)
    hosts = [_host_copy(t) for t in inputs]
    s = _streams()[0]
    delay = _delay()
    need = max(MIN_DELAY_MS, DELAY_FACTOR * t_enqueue)
    reruns = 0
    while True:
        _poison_allocator([s], poison_bytes)
        if in_place:
            twins = inputs
            for t in twins:
                if _is_dev(t):
                    t.fill_(_poison_value(t))
        else:
            twins = [_poison_twin(t) if _is_dev(t) else t for t in inputs]
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            e0, e1 = delay.enqueue(need * (1 << reruns))
            for t, h in zip(twins, hosts):
                if h is not None:
                    t.copy_(h, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            got = op(*twins)
            pending = not ev.query()
        s.synchronize()
        torch.cuda.synchronize()
        delay_ms = e0.elapsed_time(e1)
        got = flat(got)
        conclusive = not asynchronous or (pending and delay_ms >= need)
        rec = dict(name=name, t_enqueue_ms=round(t_enqueue, 3), delay_ms=round(delay_ms, 1), pending=pending, reruns=reruns,
                   kind="async" if asynchronous else "syncing")
        print("STREAMCASE", rec, flush=True)
        if conclusive or reruns == 1:
            break
        reruns += 1           # the ONE allowed re-run, delay doubled
        print(f"STREAMCASE {name}: inconclusive (pending {pending}, delay {delay_ms:.1f} ms of {need:.1f}); once more, delay doubled",
              flush=True)
    LOG.append(rec)
    assert len(got) == len(want), f"{name}: {len(got)} outputs, {len(want)} on the default stream"
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if not same_bits(g, w)]
    assert not bad, f"{name}: outputs {bad} differ from the default-stream result (work ordered in front of the stream's inputs?)"
    assert conclusive, (f"{name}: inconclusive: delay too short or the call synchronised "
                        f"(pending {pending}, delay {delay_ms:.1f} ms, needed {need:.1f} ms, t_enqueue {t_enqueue:.3f} ms)")
    return rec


def run_two_streams(name, op_a, in_a, op_b, in_b, asynchronous, rounds=5, poison_bytes=256 << 20, between=None):
    """Two independent ops on two side streams at once: each stream gets its own delay and delayed inputs, the ops are
    enqueued alternately for ``rounds`` rounds without a host sync, and EVERY round's outputs must be the serial
    default-stream results bit for bit (shared scratch, shared tickets, a workspace key that ignores the stream).
    ``between(s1, s2)`` runs once after the first round (still no sync) for assertions on host-side state."""
    in_a, in_b = list(in_a), list(in_b)
    want_a, t_a = _reference(op_a, in_a)
    want_b, t_b = _reference(op_b, in_b)
    hosts_a = [_host_copy(t) for t in in_a]
    hosts_b = [_host_copy(t) for t in in_b]
    s1, s2 = _streams()
    delay = _delay()
    need = max(MIN_DELAY_MS, DELAY_FACTOR * rounds * (t_a + t_b))
    reruns = 0
    while True:
        _poison_allocator([s1, s2], poison_bytes)
        tw_a = [_poison_twin(t) if _is_dev(t) else t for t in in_a]
        tw_b = [_poison_twin(t) if _is_dev(t) else t for t in in_b]
        torch.cuda.synchronize()
        evs, marks = [], []
        for lane, (s, tw, hosts) in enumerate(((s1, tw_a, hosts_a), (s2, tw_b, hosts_b))):
            with torch.cuda.stream(s):
                marks.append(delay.enqueue(need * (1 << reruns), lane))
                for t, h in zip(tw, hosts):
                    if h is not None:
                        t.copy_(h, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                evs.append(ev)
        got_a, got_b = [], []
        for r in range(rounds):
            with torch.cuda.stream(s1):
                got_a.append(flat(op_a(*tw_a)))
            with torch.cuda.stream(s2):
                got_b.append(flat(op_b(*tw_b)))
            if r == 0 and between is not None:
                between(s1, s2)
        pending = not evs[0].query() and not evs[1].query()
        s1.synchronize()
        s2.synchronize()
        torch.cuda.synchronize()
        delay_ms = min(e0.elapsed_time(e1) for e0, e1 in marks)
        conclusive = not asynchronous or (pending and delay_ms >= need)
        rec = dict(name=name, t_enqueue_ms=round(rounds * (t_a + t_b), 3), delay_ms=round(delay_ms, 1), pending=pending,
                   reruns=reruns, kind="async" if asynchronous else "syncing")
        print("STREAMCASE", rec, flush=True)
        if conclusive or reruns == 1:
            break
        reruns += 1
        print(f"STREAMCASE {name}: inconclusive (pending {pending}, delay {delay_ms:.1f} ms of {need:.1f}); once more, delay doubled",
              flush=True)
    LOG.append(rec)
    for r in range(rounds):
        for which, got, want in (("first", got_a[r], want_a), ("second", got_b[r], want_b)):
            assert len(got) == len(want)
            bad = [i for i, (g, w) in enumerate(zip(got, want)) if not same_bits(g, w)]
            assert not bad, f"{name}: round {r}, {which} op: outputs {bad} differ from the serial default-stream result"
    assert conclusive, (f"{name}: inconclusive: delay too short or a call synchronised "
                        f"(pending {pending}, delay {delay_ms:.1f} ms, needed {need:.1f} ms)")
    return rec
