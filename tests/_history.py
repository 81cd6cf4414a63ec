"""Call-history harness of tests/test_gpu_history.py and tests/test_history_cpu.py (not a test module): does an op's result
depend on what the workspace, the handle or the options held when the call began?  include/anyloc_hip.h ("Buffers") promises
that it does not: a call initialises every word of the workspace it depends on.  profiles/workspace_state_audit.md lists those
words.

Plain torch, the device is an argument: the CPU test drives the same code with fake ops.

  OwnedWorkspace   stands in for ``anyloc_amd._lib.workspace``: one buffer per (stream, tag) from storage the test owns, so that
                   the test decides what a call finds there -- a fill pattern, or whatever the call before it left
  PATTERNS         what a workspace is filled with, from mild to hostile.  0xFF alone (the guard-band tests) is loud: a ticket of
                   2^32 - 1 never matches, a NaN spreads.  The dangerous leftovers are plausible ones: a count a few arrivals in
                   (``ones``), a float near one (``one_f32``), another call's values (``random``, and the donor sequences)
  bits_equal       NaN-safe bit equality of possibly nested results
  History          the baselines (each case twice on a zero-filled workspace) and the comparisons against them
"""
import numpy as np
import torch

PATTERNS = ("zero", "ones", "one_f32", "random", "ff")

# Cases whose own two runs on a zero-filled workspace may differ in bits: (case, the file:line that documents why).  They are held
# to what tests/test_gpu_screen.py::test_screened_search_is_reproducible_under_load asserts -- torch.equal of every output -- and
# to nothing less.  The candidate was the one-shot screened quantiser, whose residual sums are added with atomics
# (anyloc_amd/csrc/gemm_h3.hip:165): its rounding moves the candidate margin, not the re-scored result, and every screened case of
# the catalogue reproduces its bits.  The tuple is empty and does not grow without such a citation.
NOT_BITWISE = ()


class Irreproducible(AssertionError):
    """A case whose two runs on a zero-filled workspace differ: not history-dependent but irreproducible."""


def _align(n, a=256):
    return (int(n) + a - 1) // a * a


class OwnedWorkspace:
    """``workspace(nbytes, device, tag)`` with the signature of ``anyloc_amd._lib.workspace``: the first ``nbytes`` bytes of the
    buffer of (current stream, tag).  A buffer grows when a call asks for more than it holds (``grown`` counts that: new memory
    hides leftovers, so a sequence sizes its buffers first and then requires ``grown`` to stand still).  ``handed``: every
    (tag, nbytes) handed out."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.buffers = {}
        self.handed = []
        self.grown = 0

    def install(self, monkeypatch, owner=None):
        """Replace ``owner.workspace`` (default: anyloc_amd._lib) for the rest of the test."""
        if owner is None:
            from anyloc_amd import _lib as owner
        monkeypatch.setattr(owner, "workspace", self.workspace)
        return self

    def _stream(self):
        return torch.cuda.current_stream().cuda_stream if self.device.type == "cuda" else 0

    def workspace(self, nbytes, device, tag="default"):
        nbytes = int(nbytes)
        key = (self._stream(), tag)
        buf = self.buffers.get(key)
        if buf is None or buf.numel() < nbytes:
            self.buffers[key] = buf = torch.zeros(_align(max(nbytes, 1)), dtype=torch.uint8, device=self.device)
            self.grown += 1
        self.handed.append((tag, nbytes))
        return buf[:nbytes]

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()

    def fill(self, pattern, seed=0):
        """Every byte of every buffer (not only the bytes last asked for) <- ``pattern``."""
        assert pattern in PATTERNS, pattern
        self.sync()
        for n, buf in enumerate(self.buffers.values()):
            if pattern == "zero":
                buf.zero_()
            elif pattern == "ones":
                buf.fill_(0x01)
            elif pattern == "one_f32":
                buf.view(torch.int32).fill_(0x3F800000)
            elif pattern == "random":
                g = torch.Generator(device=self.device).manual_seed(1000 * seed + n)
                buf.copy_(torch.randint(0, 256, (buf.numel(),), dtype=torch.uint8, device=self.device, generator=g))
            else:
                buf.fill_(0xFF)
        self.sync()

    def snapshot(self):
        self.sync()
        return {k: b.clone() for k, b in self.buffers.items()}

    def restore(self, snap):
        self.sync()
        assert set(snap) == set(self.buffers), "a buffer appeared or was reallocated since the snapshot"
        for k, b in snap.items():
            self.buffers[k].copy_(b)
        self.sync()


# ---- bit equality -----------------------------------------------------------------------------------------------------------------
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _leaves(x, path="out"):
    """(path, leaf) of a possibly nested result: tensors and NumPy arrays as CPU tensors, everything else as it is."""
    if isinstance(x, torch.Tensor):
        yield path, x.detach().cpu()
    elif isinstance(x, np.ndarray):
        yield path, torch.from_numpy(np.ascontiguousarray(x))
    elif isinstance(x, dict):
        for k in sorted(x):
            yield from _leaves(x[k], f"{path}[{k!r}]")
    elif isinstance(x, (list, tuple)):
        yield path, ("sequence", len(x))
        for i, v in enumerate(x):
            yield from _leaves(v, f"{path}[{i}]")
    elif isinstance(x, (set, frozenset)):
        yield path, ("set", tuple(sorted(x)))
    elif isinstance(x, float):
        yield path, torch.tensor(x, dtype=torch.float64)
    else:
        yield path, x


def _bits(t):
    t = t.contiguous()
    if t.is_complex():
        t = torch.view_as_real(t).contiguous()
    if t.is_floating_point():
        return t.view(_INT_VIEW[t.element_size()])
    return t


def first_difference(a, b):
    """None if ``a`` and ``b`` hold the same bits, else a line that names the first leaf that differs.  Tensors compare through
    their integer views: NaN equals the same NaN and no other payload, -0.0 differs from 0.0."""
    la, lb = list(_leaves(a)), list(_leaves(b))
    if len(la) != len(lb):
        return f"{len(la)} leaves against {len(lb)}"
    for (pa, x), (pb, y) in zip(la, lb):
        if pa != pb:
            return f"structure differs at {pa} / {pb}"
        if isinstance(x, torch.Tensor) != isinstance(y, torch.Tensor):
            return f"{pa}: {type(x).__name__} against {type(y).__name__}"
        if not isinstance(x, torch.Tensor):
            if type(x) is not type(y) or x != y:
                return f"{pa}: {x!r} against {y!r}"
            continue
        if x.dtype != y.dtype or x.shape != y.shape:
            return f"{pa}: {x.dtype} {tuple(x.shape)} against {y.dtype} {tuple(y.shape)}"
        bx, by = _bits(x), _bits(y)
        if not torch.equal(bx, by):
            ne = (bx != by).reshape(-1)
            i = int(ne.nonzero()[0])
            return (f"{pa}: {int(ne.sum())} of {ne.numel()} elements differ, first at flat index {i}: "
                    f"{x.reshape(-1)[i].item()!r} against {y.reshape(-1)[i].item()!r}")
    return None


def bits_equal(a, b):
    return first_difference(a, b) is None


def values_equal(a, b):
    """What NOT_BITWISE cases are held to: torch.equal of every tensor (tests/test_gpu_screen.py, reproducible under load)."""
    la, lb = list(_leaves(a)), list(_leaves(b))
    if len(la) != len(lb):
        return False
    for (_, x), (_, y) in zip(la, lb):
        if isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor):
            if x.dtype != y.dtype or not torch.equal(x, y):
                return False
        elif isinstance(x, torch.Tensor) or isinstance(y, torch.Tensor) or x != y:
            return False
    return True


def frozen(x):
    """A result as the harness keeps it: CPU copies of the tensors (an op's outputs are never views of the workspace, but a
    kept reference must not alias anything a later call writes)."""
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().clone()
    if isinstance(x, np.ndarray):
        return x.copy()
    if isinstance(x, dict):
        return {k: frozen(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return tuple(frozen(v) for v in x)
    if isinstance(x, (set, frozenset)):
        return frozenset(x)
    return x


# ---- baselines and comparisons ----------------------------------------------------------------------------------------------------
class History:
    """The cases ``name -> dict(op=, inputs=)`` on one OwnedWorkspace.  ``baseline(name)``: the case twice on a zero-filled
    workspace (after one run that sizes the buffers), bit-equal or Irreproducible; kept for the session.  Every check below
    names the case, and what ran before it, in its failure."""

    def __init__(self, ws, cases, not_bitwise=NOT_BITWISE):
        self.ws, self.cases = ws, cases
        self.not_bitwise = {n for n, _ in not_bitwise}
        self._base = {}

    def run(self, name):
        case = self.cases[name]
        out = case["op"](*case["inputs"])
        self.ws.sync()
        return frozen(out)

    def same(self, name, got, want):
        if name in self.not_bitwise:
            return None if values_equal(got, want) else "values differ (a NOT_BITWISE case: torch.equal of every output)"
        return first_difference(got, want)

    def baseline(self, name):
        if name not in self._base:
            self.run(name)                       # sizes the buffers: the two runs below start on zeros, whole buffer
            self.ws.fill("zero")
            a = self.run(name)
            self.ws.fill("zero")
            b = self.run(name)
            diff = self.same(name, a, b)
            if diff is not None:
                raise Irreproducible(f"{name}: two runs on a zero-filled workspace differ ({diff}): irreproducible, not history-dependent")
            self._base[name] = a
        return self._base[name]

    def check_pattern(self, name, pattern, seed=0):
        want = self.baseline(name)
        grown = self.ws.grown
        self.ws.fill(pattern, seed)
        got = self.run(name)
        assert self.ws.grown == grown, f"{name}: the workspace grew under pattern {pattern!r}"
        diff = self.same(name, got, want)
        assert diff is None, f"{name} on a workspace filled with {pattern!r} differs from its zero-workspace baseline: {diff}"

    def check_sequence(self, names, label=None):
        """The cases ``names`` one after the other on the same buffers, the device waited for in between: every call's bits
        equal that call's own baseline.  The buffers are sized for all of them first (the baselines), then zeroed."""
        want = [self.baseline(n) for n in names]
        grown = self.ws.grown
        self.ws.fill("zero")
        for i, (n, w) in enumerate(zip(names, want)):
            got = self.run(n)
            assert self.ws.grown == grown, f"{n}: the workspace grew inside the sequence (new memory hides the leftovers)"
            diff = self.same(n, got, w)
            before = " -> ".join(names[:i]) or "a zero-filled workspace"
            assert diff is None, f"{label or 'sequence'}: call {i + 1}, {n}, behind [{before}] differs from its own baseline: {diff}"

    def check_behind(self, donor, victim):
        self.check_sequence([donor, victim], label=f"victim {victim} behind donor {donor}")
