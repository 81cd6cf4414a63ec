"""The call-history harness must fail on what it exists to catch (no GPU): fake ops on CPU tensors, each with one planted defect of
the kind profiles/workspace_state_audit.md is about, run through tests/_history.py exactly as tests/test_gpu_history.py runs the
library.  Every planted defect is reported, with the offending case named; the sound twin of each op passes.  Then the lists of
the GPU module: every donor and every sequence step is a case that exists."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _history as H  # noqa: E402

CPU = torch.device("cpu")


# ---- fake library: ops that carve int32 words from the workspace of fake_lib.workspace --------------------------------------------
fake_lib = types.SimpleNamespace(workspace=None)


def _words(n, tag="fake"):
    return fake_lib.workspace(4 * n, CPU, tag).view(torch.int32)


def sound_sum(x):
    """acc is zeroed by the call: any leftover is overwritten."""
    w = _words(4)
    w[0] = 0
    w[0] += int(x.sum())
    return w[:1].clone()


def read_before_write(x):
    """acc is NOT zeroed: the sum starts from whatever the word held."""
    w = _words(4)
    w[0] += int(x.sum())
    return w[:1].clone()


def plausible_ticket(x):
    """A reduction 'by the last arrival': the arrival counter (one byte) is never reset in front of the launch, and the call goes
    wrong only when it starts from a small plausible count (0 < n <= 64: some arrivals of an earlier launch).  0xFF, like zero,
    happens to work: the loud pattern does not find it."""
    w = fake_lib.workspace(16, CPU, "fake")
    start = int(w[4])
    w[4] = 0
    out = x.sum().reshape(1).clone()
    if 0 < start <= 64:
        out += 1.0                      # 'the last arrival came early and reduced partials that were not there yet'
    return out


def leaves_small_count(x):
    """A sound op that leaves a few arrivals in that byte of the shared buffer."""
    w = fake_lib.workspace(16, CPU, "fake")
    w[4] = 3
    return x.sum().reshape(1).clone()


def short_memset(n_read):
    """Zeroes n_small = min(n, 8) words where it accumulates into, and reads, n words."""
    def op(x):
        w = _words(64)
        w[:min(n_read, 8)] = 0
        w[:n_read] += 1
        return w[:n_read].clone()
    return op


def full_memset(n_read):
    def op(x):
        w = _words(64)
        w[:n_read] = 0
        w[:n_read] += 1
        return w[:n_read].clone()
    return op


X = torch.arange(5, dtype=torch.float32)
CASES = {
    "sound_sum": dict(op=sound_sum, inputs=[X]),
    "read_before_write": dict(op=read_before_write, inputs=[X]),
    "plausible_ticket": dict(op=plausible_ticket, inputs=[X]),
    "leaves_small_count": dict(op=leaves_small_count, inputs=[X]),
    "short_memset_32": dict(op=short_memset(32), inputs=[X]),
    "short_memset_4": dict(op=short_memset(4), inputs=[X]),
    "short_memset_16": dict(op=short_memset(16), inputs=[X]),
    "full_memset_32": dict(op=full_memset(32), inputs=[X]),
    "full_memset_16": dict(op=full_memset(16), inputs=[X]),
}


@pytest.fixture
def hist(monkeypatch):
    ws = H.OwnedWorkspace(CPU).install(monkeypatch, owner=fake_lib)
    return H.History(ws, CASES)


def _reported(fn, *names):
    """``fn()`` fails, and the failure names every one of ``names``."""
    with pytest.raises(AssertionError) as e:
        fn()
    assert not isinstance(e.value, H.Irreproducible), e.value
    for n in names:
        assert n in str(e.value), (n, str(e.value))
    return str(e.value)


# ---- the planted defects -------------------------------------------------------------------------------------------------------
def test_owned_workspace_hands_out_one_buffer_per_tag_and_fills_all_of_it(hist):
    ws = hist.ws
    a = fake_lib.workspace(100, CPU, "a")
    b = fake_lib.workspace(40, CPU, "a")
    c = fake_lib.workspace(8, CPU, "b")
    assert a.numel() == 100 and b.numel() == 40 and a.data_ptr() == b.data_ptr() != c.data_ptr()
    assert ws.handed == [("a", 100), ("a", 40), ("b", 8)] and ws.grown == 2
    for pattern, byte in (("zero", 0), ("ones", 1), ("ff", 0xFF)):
        ws.fill(pattern)
        assert all(bool((buf == byte).all()) for buf in ws.buffers.values())         # the whole buffer, not the 40 bytes last asked for
    ws.fill("one_f32")
    assert bool((a.view(torch.float32) == 1.0).all())
    ws.fill("random", 1)
    r1 = a.clone()
    snap = ws.snapshot()
    ws.fill("random", 2)
    assert not torch.equal(a, r1) and len(torch.unique(a)) > 32
    ws.restore(snap)
    assert torch.equal(a, r1)
    ws.fill("random", 1)
    assert torch.equal(a, r1)                                                       # seeded
    fake_lib.workspace(4096, CPU, "a")
    assert ws.grown == 3
    assert H.PATTERNS == ("zero", "ones", "one_f32", "random", "ff")


def test_read_before_write_is_reported_under_every_pattern_but_zero(hist):
    hist.check_pattern("read_before_write", "zero")
    for pattern in H.PATTERNS[1:]:
        _reported(lambda: hist.check_pattern("read_before_write", pattern), "read_before_write", repr(pattern))
        hist.check_pattern("sound_sum", pattern)


def test_a_defect_that_needs_a_plausible_count_passes_ff_and_is_reported_under_ones_and_behind_a_donor(hist):
    hist.check_pattern("plausible_ticket", "zero")
    hist.check_pattern("plausible_ticket", "ff")                  # loud garbage does not find it: the reason for the pattern list
    hist.check_pattern("plausible_ticket", "one_f32")
    _reported(lambda: hist.check_pattern("plausible_ticket", "ones"), "plausible_ticket", "'ones'")
    _reported(lambda: hist.check_behind("leaves_small_count", "plausible_ticket"), "plausible_ticket", "leaves_small_count")
    hist.check_behind("leaves_small_count", "sound_sum")
    hist.check_behind("plausible_ticket", "leaves_small_count")


def test_a_short_memset_is_found_by_the_larger_then_smaller_sequence(hist):
    # on zeros, and behind a SMALLER call, the short memset is enough
    hist.check_sequence(["short_memset_4", "short_memset_16"])
    # behind a larger call the words 8 .. 15 still hold its counts
    msg = _reported(lambda: hist.check_sequence(["short_memset_32", "short_memset_4", "short_memset_16"], label="short memset"),
                    "short_memset_16", "short_memset_32 -> short_memset_4", "call 3")
    assert "first at flat index 8" in msg
    hist.check_sequence(["full_memset_32", "short_memset_4", "full_memset_16"])


def test_a_sequence_that_reallocates_is_refused(hist):
    hist.baseline("sound_sum")
    big = dict(op=lambda x: fake_lib.workspace(1 << 16, CPU, "fake")[:1].clone(), inputs=[X])
    hist.cases = dict(CASES, grows=big)
    hist._base["grows"] = torch.zeros(1, dtype=torch.uint8)       # (a baseline that did not size the buffer)
    _reported(lambda: hist.check_sequence(["sound_sum", "grows"]), "grows", "grew")


def test_an_irreproducible_case_is_told_from_a_history_dependent_one(hist):
    n = [0]

    def drifts(x):
        n[0] += 1
        return x + n[0]
    hist.cases = dict(CASES, drifts=dict(op=drifts, inputs=[X]))
    with pytest.raises(H.Irreproducible) as e:
        hist.baseline("drifts")
    assert "drifts" in str(e.value)


def test_state_on_a_handle_is_found_by_the_fresh_model_comparison():
    class Handle:
        """A fake ViT handle: ``exact`` is a per-block switch a call may set and must clear again."""
        def __init__(self, leaky):
            self.exact, self.leaky = False, leaky

        def tripping_call(self, x):
            self.exact = True
            out = self.forward(x)
            if not self.leaky:
                self.exact = False
            return out

        def forward(self, x):
            return x * (3.0 if self.exact else 2.0)

    for leaky in (False, True):
        used, fresh = Handle(leaky), Handle(leaky)
        used.tripping_call(X)
        diff = H.first_difference(used.forward(X), fresh.forward(X))
        assert (diff is not None) == leaky, diff


def test_bits_equal_tells_nan_payloads_signed_zeros_and_int64_apart():
    nan = torch.tensor([0x7FC00000, 0x7FC00001, 0xFFC00000 - (1 << 32)], dtype=torch.int32).view(torch.float32)
    assert H.bits_equal(nan, nan.clone())                                            # NaN-safe
    assert not H.bits_equal(nan[:1], nan[1:2]) and not H.bits_equal(nan[:1], nan[2:])
    assert not H.bits_equal(torch.tensor([0.0]), torch.tensor([-0.0])) and torch.equal(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not H.bits_equal(torch.tensor([-1], dtype=torch.int64), torch.tensor([0xFFFFFFFF], dtype=torch.int64))
    assert not H.bits_equal(torch.tensor([-1], dtype=torch.int64), torch.tensor([-1], dtype=torch.int32))
    assert not H.bits_equal(torch.zeros(2, 3), torch.zeros(3, 2))
    half = torch.tensor([0x7E00, 0x7E01], dtype=torch.int16).view(torch.float16)
    assert not H.bits_equal(half[:1], half[1:]) and H.bits_equal(half, half.clone())
    d = torch.tensor([float("nan")], dtype=torch.float64)
    assert H.bits_equal(d, d.clone()) and not H.bits_equal(d, -d)
    # nested results: outputs, labels, scales, index lists, and the model's record of an FFN-checked forward
    import numpy as np
    a = (torch.ones(2), [torch.arange(3), None], np.array([1.5, float("nan")]), {3, 1}, 2)
    b = (torch.ones(2), [torch.arange(3), None], np.array([1.5, float("nan")]), {1, 3}, 2)
    assert H.bits_equal(a, b)
    assert not H.bits_equal(a, b[:4] + (3,)) and not H.bits_equal(a, b[:3] + ({1}, 2)) and not H.bits_equal(a, b[:4])
    assert "out[1][0]" in H.first_difference(a, (b[0], [torch.arange(3) + 1, None]) + b[2:])
    assert not H.values_equal(torch.tensor([1.0]), torch.tensor([2.0])) and H.values_equal(torch.tensor([0.0]), torch.tensor([-0.0]))


# ---- the lists of tests/test_gpu_history.py --------------------------------------------------------------------------------------
def test_donors_sequences_and_not_bitwise_name_cases_that_exist():
    import test_gpu_history as G
    import test_gpu_streams as S
    catalogue = set(S.ASYNC_OPS) | set(S.SYNCING_OPS)          # (test_every_case_is_in_exactly_one_list ties the lists to _cases())
    assert set(G.CATALOGUE) == catalogue and len(G.CATALOGUE) == len(catalogue)
    assert len(set(G.DONORS)) == len(G.DONORS) == 16 and set(G.DONORS) <= catalogue
    extra = set(G.EXTRA_CASES)
    assert not extra & catalogue
    used = set()
    for label, steps in G.SEQUENCES.items():
        assert len(steps) >= 2, label
        for s in steps:
            assert s in catalogue or s in extra, (label, s)
            used.add(s)
    assert extra <= used | set(G.EXTRA_ELSEWHERE), sorted(extra - used)
    for name, where in H.NOT_BITWISE:
        assert name in catalogue, name
        path, line = where.rsplit(":", 1)
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        assert os.path.isfile(os.path.join(root, path)) and int(line) > 0, where
    for option, (value, donor, victim) in G.OPTION_HISTORY.items():
        assert donor in catalogue and victim in catalogue, option


def test_every_option_of_the_header_has_a_history_case():
    import re
    import test_gpu_history as G
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "anyloc_amd", "csrc", "runtime.hip")).read()
    table = src[src.index("kOptDefs[OPT_COUNT] = {"):]
    names = re.findall(r'\{"([a-z0-9_]+)",', table[:table.index("};")])
    header = open(os.path.join(root, "include", "anyloc_hip.h")).read()
    listed = header[header.index("option is looked up"):header.index("Unknown names are rejected")]
    assert all(re.search(rf"\b{n}\b", listed) for n in names), [n for n in names if not re.search(rf"\b{n}\b", listed)]
    assert len(names) > 10, names
    assert set(G.OPTION_HISTORY) | set(G.OPTIONS_EXCLUDED) == set(names), sorted(set(names) ^ (set(G.OPTION_HISTORY) | set(G.OPTIONS_EXCLUDED)))
