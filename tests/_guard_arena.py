"""Guard-band arena of tests/test_gpu_guard_bands.py and tests/test_guard_arena_cpu.py (not a test module): does a call
write only where include/anyloc_hip.h ("Buffers") says it may?

``torch.empty`` hides a stray store: the caching allocator rounds every allocation up and packs small ones into shared
blocks, so a store past an output lands in slack or in a neighbour and nothing a test reads changes.  Here every buffer of
a call is a view of EXACTLY the documented size into one ``torch.uint8`` arena:

  * regions sit at 256-byte aligned offsets (what ``torch.empty`` gives and ``Arena::take`` of csrc/common.hpp assumes);
  * between two regions lie at least GUARD (64 KiB) guard bytes, at both ends of the arena at least END_GUARD (4 MiB).
    These are conditions, not measurements: GUARD must exceed one 256-row tile row of the widest output a case places,
    ``Arena(guard=...)`` raises it where a case needs more;
  * guard bytes are 0xA5; output and workspace regions start as 0xFF (NaN as fp16 / bf16 / fp32 / fp64, -1 as int64);
    input regions hold the real data (the stride gaps of a strided input 0xFF) and the arena keeps what they must still
    hold after the call.

``check()`` (after the device has been waited for) returns a list of ``Finding``: one per (kind, region), with the offset
of the first offending byte RELATIVE TO THE REGION (negative: in front of it; >= nbytes: behind it) and the count of
offending bytes (unwritten: of elements):

  guard      a guard byte changed (named after the nearest region);
  gap        a byte of a strided output's gap (columns [N, ld) of a row) changed;
  input      an input region differs from its copy (regions taken with ``in_place=True`` are exempt);
  unwritten  an element of an output's documented extent is still all-0xFF where the reference value is neither NaN nor
             the documented -1 padding (reference None: every element must have been written).

The helper takes the device as an argument and uses plain torch only, so the CPU test can plant each kind of fault and
see it reported.  A store that lands beyond the END_GUARD at either end of the arena cannot be seen.
"""
from collections import namedtuple

import torch

ALIGN = 256
GUARD = 64 << 10
END_GUARD = 4 << 20
GUARD_BYTE, FRESH_BYTE = 0xA5, 0xFF
MAX_REPORTED = 1 << 16      # offending bytes / elements looked at per check (a kernel gone wild changes megabytes)

Finding = namedtuple("Finding", "kind region offset count")


class Region:
    def __init__(self, name, role, start, nbytes, view, in_place):
        self.name, self.role, self.start, self.nbytes, self.view, self.in_place = name, role, start, nbytes, view, in_place
        self.ref = None          # reference values of an output (unwritten check), set by Arena.check(refs)


def _round_up(n, a):
    return (n + a - 1) // a * a


def _extent(shape, strides):
    """elements from the first to one past the last element of a strided view"""
    if any(s == 0 for s in shape):
        return 0
    return 1 + sum((n - 1) * st for n, st in zip(shape, strides))


class Arena:
    """``capacity`` bytes of region space (guards included) between two END_GUARDs on ``device``."""

    def __init__(self, device, capacity=32 << 20, guard=GUARD, end_guard=END_GUARD):
        assert guard >= GUARD and end_guard >= END_GUARD and guard % ALIGN == 0 and end_guard % ALIGN == 0
        self.device = torch.device(device)
        self.guard, self.end_guard = guard, end_guard
        total = end_guard + capacity + end_guard + ALIGN
        self._raw = torch.full((total,), GUARD_BYTE, dtype=torch.uint8, device=self.device)
        skew = -self._raw.data_ptr() % ALIGN                     # (torch.empty is 256-byte aligned on the device already)
        self.buf = self._raw[skew:skew + total - ALIGN]
        # what a byte must still hold after the call, and whether it must (guards, inputs, gaps: 1; live outputs and
        # workspaces: 0)
        self._expect = self.buf.clone()
        self._must = torch.ones_like(self.buf)
        self._at = end_guard
        self._limit = end_guard + capacity
        self.regions = []

    # ---- carving ---------------------------------------------------------------------------------------------------
    def take(self, nbytes, dtype=torch.uint8, shape=None, strides=None, name=None, role="output", data=None, in_place=False):
        """A view of exactly ``nbytes`` bytes as ``dtype`` elements: ``shape`` (default flat) with ``strides`` in elements
        (default dense; the region then spans the view's extent, gaps included, and ``nbytes`` must be that extent).
        ``role``: "output" / "workspace" (prefilled 0xFF) or "input" (``data`` copied into the view, kept for check())."""
        assert role in ("output", "workspace", "input")
        item = torch.empty(0, dtype=dtype).element_size()
        nbytes = int(nbytes)
        assert nbytes % item == 0, (nbytes, dtype)
        shape = (nbytes // item,) if shape is None else tuple(int(s) for s in shape)
        if strides is None:
            strides, acc = [], 1
            for n in reversed(shape):
                strides.append(acc)
                acc *= max(n, 1)
            strides = tuple(reversed(strides))
        strides = tuple(int(s) for s in strides)
        assert _extent(shape, strides) * item == nbytes, f"{name}: a view {shape} x {strides} of {dtype} is not {nbytes} bytes"
        start = self._at
        assert start % ALIGN == 0
        if start + nbytes + self.guard > self._limit:
            raise MemoryError(f"guard arena: {name} of {nbytes} bytes does not fit (capacity {self._limit - self.end_guard})")
        self._at = _round_up(start + nbytes, ALIGN) + self.guard
        raw = self.buf[start:start + nbytes]
        raw.fill_(FRESH_BYTE)
        flat = raw.view(dtype)
        view = flat.as_strided(shape, strides) if nbytes else flat.reshape(shape)
        name = name or f"r{len(self.regions)}"
        if role == "input":
            assert data is not None
            view.copy_(data.to(self.device))
        else:
            assert data is None
        self._expect[start:start + nbytes] = raw
        if role == "output":
            # the live elements may change; the gaps of a strided view may not
            live = torch.zeros(nbytes // item if nbytes else 0, dtype=torch.uint8, device=self.device)
            if nbytes:
                live.as_strided(shape, strides).fill_(1)
            self._must[start:start + nbytes] = 1 - live.repeat_interleave(item)
        elif role == "workspace" or in_place:
            self._must[start:start + nbytes] = 0
        reg = Region(name, role, start, nbytes, view, in_place)
        self.regions.append(reg)
        return view

    def input(self, name, data, strides=None, in_place=False):
        """``data`` placed in the arena (``strides`` in elements: the region spans the strided extent)."""
        shape = tuple(data.shape)
        item = data.element_size()
        if strides is None:
            nbytes = data.numel() * item
        else:
            nbytes = _extent(shape, strides) * item
        return self.take(nbytes, data.dtype, shape, strides, name=name, role="input", data=data, in_place=in_place)

    def output(self, name, dtype, shape, strides=None):
        item = torch.empty(0, dtype=dtype).element_size()
        n = _extent(shape, strides) if strides is not None else int(torch.Size(shape).numel())
        return self.take(n * item, dtype, shape, strides, name=name, role="output")

    def workspace(self, nbytes, name="workspace"):
        return self.take(nbytes, torch.uint8, name=name, role="workspace")

    def region(self, name):
        for r in self.regions:
            if r.name == name:
                return r
        raise KeyError(name)

    # ---- verdict ---------------------------------------------------------------------------------------------------
    def _locate(self, pos):
        """arena byte -> (region, kind): the region that holds it, or the nearest one for a guard byte"""
        best, dist = None, None
        for r in self.regions:
            if r.start <= pos < r.start + r.nbytes:
                return r, ("input" if r.role == "input" else "gap")
            d = r.start - pos if pos < r.start else pos - (r.start + r.nbytes) + 1
            if dist is None or d < dist:
                best, dist = r, d
        return best, "guard"

    def check(self, refs=None, pad=None):
        """-> [Finding].  ``refs``: {output name: reference tensor of the view's shape, or None = every element must be
        written}; outputs not named get no unwritten check.  ``pad``: {output name: value} of the documented padding (the -1
        of a top-k tail): elements whose reference holds it may keep the fresh pattern."""
        refs, pad = refs or {}, pad or {}
        found = {}

        def add(kind, reg, off):
            key = (kind, reg.name if reg is not None else "arena")
            first, count = found.get(key, (off, 0))
            found[key] = (min(first, off), count + 1)

        bad = torch.nonzero((self.buf != self._expect) & (self._must != 0)).flatten()[:MAX_REPORTED].cpu().tolist()
        for pos in bad:
            reg, kind = self._locate(pos)
            add(kind, reg, pos - reg.start if reg is not None else pos)
        for name, ref in refs.items():
            reg = self.region(name)
            assert reg.role == "output", name
            v = reg.view
            if v.numel() == 0:
                continue
            item = v.element_size()
            dense = v.contiguous()
            fresh = (dense.reshape(-1).view(torch.uint8).reshape(-1, item) == FRESH_BYTE).all(dim=1).reshape(dense.shape)
            if ref is not None:
                ref = ref.to(self.device).reshape(dense.shape)
                excused = torch.isnan(ref) if ref.is_floating_point() else torch.zeros_like(fresh)
                if name in pad:
                    excused = excused | (ref == pad[name])
                fresh = fresh & ~excused
            for idx in torch.nonzero(fresh)[:MAX_REPORTED].cpu().tolist():
                add("unwritten", reg, sum(i * s for i, s in zip(idx, v.stride())) * item)
        return [Finding(kind, region, off, count) for (kind, region), (off, count) in sorted(found.items())]


def guarded_workspace(monkeypatch, arena, scale=1, skew=0):
    """Replace ``anyloc_amd._lib.workspace`` for the rest of the test: every request gets a FRESH region of exactly the
    requested bytes (times ``scale``) carved from ``arena`` and prefilled with 0xFF.  Every caller passes ``ws.numel()`` as
    ``workspace_bytes``, so the library sees the documented size -- through ops.*, retrieval.py, kmeans.py, vlad.py and
    extractor.py alike.  ``skew``: the workspace starts that many bytes behind a 256-byte boundary (the region is that much
    longer in front) -- what alignment of the base does the library need?  -> the list the handed-out (tag, bytes) pairs
    are appended to."""
    from anyloc_amd import _lib
    handed = []

    def workspace(nbytes, device, tag="default"):
        handed.append((tag, int(nbytes)))
        return arena.workspace(int(nbytes) * scale + skew, name=f"workspace:{tag}:{len(handed)}")[skew:]

    monkeypatch.setattr(_lib, "workspace", workspace)
    return handed
