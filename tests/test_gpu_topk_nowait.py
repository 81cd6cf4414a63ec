"""ANYLOC_TOPK_NO_WAIT (``pytest -m gpu``; ``no_wait=True`` of ops.topk / ops.topk_indexed / retrieval.FlatIndex.search): the
screened search without its read-back.  What the host decides from the overflow flag of a waiting call is decided on the device
(csrc/topk.hip, device_fallback): up to 64 overflowed queries are searched unscreened as a batch of their own and only THEIR
lists are replaced; more than 64 run the unscreened search for every query, as the waiting call does.

Data recipe and list check are those of tests/_retrieval_refs.py: bars 3e-6 (inner product) / 1e-5 (L2) against a float64 flat
search, a differing index only at a float64 near-tie, and (cap="gaps") at most 2 x the near-ties of the float64 lists
themselves.  The overflow recipes are those of tests/test_gpu_screen.py: a zero query (every row ties inside its bound) and 700
copies of one query's best row (more than the 512 candidates a query may have per column range).

Whether a WAITING call overflowed is read from its profile: it runs the exact score GEMM (tag topk_scores_gemm) only in its
fallback.  The flagged call enqueues those GEMMs always, behind gates, so its own profile says nothing about that."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _retrieval_refs as R
from _retrieval_refs import _screened_then_fallback, _screened_without_fallback

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCREEN = dict(topk_screen=1, topk_h3=1)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 1. no overflow: the bits of the waiting call -----------------------------------------------------------------------------
@pytest.mark.parametrize("nq,ndb,dim,k,metric", [(600, 20000, 4096, 20, "ip"), (600, 20000, 4096, 20, "l2"),
                                                 (257, 9000, 1024, 5, "ip"),         # a short last panel
                                                 (300, 140000, 512, 10, "ip"),       # two column ranges
                                                 (70, 12, 256, 20, "l2")])           # k > ndb
def test_without_overflow_the_flag_changes_no_bit(nq, ndb, dim, k, metric):
    """One exception, found when the test first ran: on RAW rows under L2 the bound scales with the largest raw norm (5.5 here) and
    the 600 x 20 000 x 4096 shape has a few queries with more than 512 rows inside it, so the waiting call falls back there.
    "No overflow" is then not the case under test; the flagged call gives those queries a side batch, and its lists are held to
    the float64 search over the raw rows with the scaled bars of tests/test_gpu_screen.py::test_screened_search_on_raw_rows."""
    from anyloc_amd import ops, retrieval
    qu, db = R.planted_rows(nq, ndb, dim, nq + ndb + dim)
    method = "cosine" if metric == "ip" else "l2"
    with ops.options(**SCREEN):
        for normalize in (True, False):
            want, prof = R.profiled(lambda: ops.topk(qu, db, k, metric, normalize_db=normalize))
            got = ops.topk(qu, db, k, metric, normalize_db=normalize, no_wait=True)
            if not normalize and _screened_then_fallback(prof):
                scale = float(db.double().norm(dim=1).max()) ** (2 if metric == "l2" else 1)
                R.check_lists(got[0], got[1], R.exact_scores64(qu, db, metric, normalize=False), k, metric, f"raw rows, overflow, {nq}x{ndb}x{dim} {metric}", scale=scale, cap="gaps")
                print(f"raw rows {nq}x{ndb}x{dim} {metric}: the waiting call fell back; {int((got[1] != want[1]).any(1).sum())} lists differ from it")
                continue
            assert _screened_without_fallback(prof), (normalize, sorted(prof))
            assert _same(got, want), ("ops.topk", normalize)
        want = ops.topk(qu, db, k, metric, index_base=5000, normalize_db=True)
        assert _same(ops.topk(qu, db, k, metric, index_base=5000, normalize_db=True, no_wait=True), want), "index_base"
        for name, index in (("rows kept", retrieval.FlatIndex(db, method, True, planes=True)),
                            ("rows free", retrieval.FlatIndex(db, method, True, keep_fp32=False, rescore="planes"))):
            want, prof = R.profiled(lambda: index.search(qu, k))
            assert _screened_without_fallback(prof), (name, sorted(prof))
            assert _same(index.search(qu, k, no_wait=True), want), name
            assert _same(retrieval.search(index, qu, k, method, True, no_wait=True), want), name


# ---- 2., 3., 7. a few overflowed queries: a side batch, and nobody else's list moves --------------------------------------------
def _search(how, qu, db, planes, k, metric, **kw):
    from anyloc_amd import ops
    if how == "one-shot":
        return ops.topk(qu, db, k, metric, normalize_db=True, **kw)
    if how == "rows kept":
        return ops.topk_indexed(qu, planes, db.shape[0], k, metric, normalize_db=True, db=db, **kw)
    return ops.topk_indexed(qu, planes, db.shape[0], k, metric, normalize_db=True, rescore_planes=True, **kw)


def _few_overflowed(qu, db, how, k, metric, zero, dup_q, first, tag):
    """``zero``: queries that are zero rows; ``dup_q``: the query whose best row ``first[0]`` has 700 copies from row
    ``first[1]`` on.  -> the flagged call's lists, after every assertion of the issue's case 2."""
    from anyloc_amd import ops
    nq = qu.shape[0]
    over = sorted(set(zero) | {dup_q})
    with ops.options(**SCREEN):
        planes = None if how == "one-shot" else ops.topk_index_build(db)
        d, i = _search(how, qu, db, planes, k, metric, no_wait=True)
        # the waiting call on the same input falls back for everyone: screened first, then the unscreened bits
        (d_w, i_w), prof = R.profiled(lambda: _search(how, qu, db, planes, k, metric))
        assert _screened_then_fallback(prof), (tag, sorted(prof))
        # ... so the lists nobody should have touched come from a waiting call WITHOUT the overflowing queries
        calm = qu.clone()
        other = next(q for q in range(nq) if q not in over)
        calm[over] = qu[other]
        (d_c, i_c), prof = R.profiled(lambda: _search(how, calm, db, planes, k, metric))
        assert _screened_without_fallback(prof), (tag, sorted(prof))
    R.check_lists(d, i, R.exact_scores64(qu, db, metric), k, metric, tag, cap="gaps")
    keep = torch.ones(nq, dtype=torch.bool, device=DEV)
    keep[over] = False
    assert torch.equal(d[keep], d_c[keep]) and torch.equal(i[keep], i_c[keep]), (tag, "a list outside the side batch moved")
    # the side batch ran the unscreened search of the entry point: a zero query scores exactly 0 against every row and the
    # copies score alike in any arithmetic, so these lists are the waiting call's fallback lists whatever tiles scored them
    for q in zero:
        assert torch.equal(i[q], i_w[q]) and torch.equal(d[q], d_w[q]), (tag, q)
        if metric == "ip":                                   # every row ties at 0: lower index first
            assert torch.equal(i[q], torch.arange(k, device=DEV)), (tag, q, i[q])
    want = torch.cat([torch.tensor([first[0]], device=DEV), torch.arange(first[1], first[1] + k - 1, device=DEV)])
    assert torch.equal(i[dup_q], want), (tag, i[dup_q])
    return d, i


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("how", ["one-shot", "rows free"])
def test_a_few_overflowed_queries_go_through_the_side_batch(how, metric):
    qu, db = R.planted_rows(300, 17000, 4096, 77)
    qu[3] = 0.0
    db[100] = 3.0 * qu[0]
    db[3000:3700] = db[100].clone().expand(700, -1)
    _few_overflowed(qu, db, how, 20, metric, [3], 0, (100, 3000), f"side batch, {how}, {metric}")


@pytest.mark.parametrize("where", ["first range only", "second range only"])
def test_the_overflow_mark_of_a_query_is_sticky_across_column_ranges(where):
    """140 000 rows are two column ranges (131 072 + 8928); the candidate count of a query is per range and overwritten by the
    next one, the mark is not.  The issue asks for the second range; the first is where forgetting would show."""
    qu, db = R.planted_rows(300, 140000, 512, 300 + 140000 + 512)
    at = 2000 if where == "first range only" else 131100
    db[at] = 3.0 * qu[0]
    db[at + 900:at + 1600] = db[at].clone().expand(700, -1)
    _few_overflowed(qu, db, "rows kept", 10, "ip", [], 0, (at, at + 900), f"sticky mark, {where}")


def test_the_side_batch_is_reproducible():
    from anyloc_amd import ops
    qu, db = R.planted_rows(300, 17000, 4096, 77)
    qu[3] = 0.0
    db[100] = 3.0 * qu[0]
    db[3000:3700] = db[100].clone().expand(700, -1)
    with ops.options(**SCREEN):
        first = ops.topk(qu, db, 20, "ip", normalize_db=True, no_wait=True)
        for run in range(9):
            assert _same(ops.topk(qu, db, 20, "ip", normalize_db=True, no_wait=True), first), run


# ---- 4., 5. many overflowed queries: the unscreened search for everyone, as after the wait ---------------------------------------
@pytest.mark.parametrize("n_zero", [64, 65, 200])
def test_the_boundary_between_side_batch_and_full_fallback(n_zero):
    """64 overflowed queries still fit the side batch; 65 (and 200) run the unscreened search for every query, which is what the
    waiting call does for them: the same bits."""
    from anyloc_amd import ops
    qu, db = R.planted_rows(300, 17000, 4096, 77)
    zero = torch.arange(300, device=DEV)[torch.randperm(300, generator=torch.Generator(device=DEV).manual_seed(n_zero), device=DEV)[:n_zero]]
    qu[zero] = 0.0
    with ops.options(**SCREEN):
        d, i = ops.topk(qu, db, 20, "ip", normalize_db=True, no_wait=True)
        (d_w, i_w), prof = R.profiled(lambda: ops.topk(qu, db, 20, "ip", normalize_db=True))
    assert _screened_then_fallback(prof), sorted(prof)
    R.check_lists(d, i, R.exact_scores64(qu, db, "ip"), 20, "ip", f"{n_zero} zero queries", cap="gaps")
    assert torch.equal(i[zero], torch.arange(20, device=DEV).expand(n_zero, -1))
    if n_zero > 64:
        assert torch.equal(d, d_w) and torch.equal(i, i_w)
    else:                                                  # the others kept their screened lists: not the fallback's bits
        assert torch.equal(i[zero], i_w[zero]) and torch.equal(d[zero], d_w[zero])


# ---- 6. asynchrony: the poison harness of tests/test_gpu_streams.py ---------------------------------------------------------------
def _unit(*shape, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(*shape, generator=g, device=DEV), dim=-1)


def _stream_data(ndb, seed, overflow_for=None):
    g = torch.Generator(device=DEV).manual_seed(seed)
    db = torch.randn(ndb, 256, generator=g, device=DEV) * (0.3 + 2.0 * torch.rand(ndb, 1, generator=g, device=DEV))
    if overflow_for is not None:
        db[200:800] = (3.0 * overflow_for).expand(600, -1)    # > 512 candidates inside one query's bound
    return db


def _with(op):
    def run(*a):
        from anyloc_amd import ops
        with ops.options(**SCREEN):
            return op(*a)
    return run


@pytest.mark.parametrize("overflow", [False, True], ids=["calm", "overflow"])
@pytest.mark.parametrize("how", ["one-shot", "rows kept", "rows free"])
def test_a_flagged_call_returns_while_its_inputs_are_pending(how, overflow):
    import _stream_harness as H
    from anyloc_amd import ops
    q70 = _unit(70, 256, seed=130)
    db = _stream_data(900, 131, q70[0] if overflow else None)
    with ops.options(**SCREEN):
        planes = ops.topk_index_build(db)
    torch.cuda.synchronize()
    if how == "one-shot":
        inputs = [q70, db]
        flagged = _with(lambda q, d: ops.topk(q, d, 5, "ip", normalize_db=True, no_wait=True))
        waiting = _with(lambda q, d: ops.topk(q, d, 5, "ip", normalize_db=True))
    elif how == "rows kept":
        inputs = [q70, planes, db]
        flagged = _with(lambda q, p, d: ops.topk_indexed(q, p, 900, 5, normalize_db=True, db=d, no_wait=True))
        waiting = _with(lambda q, p, d: ops.topk_indexed(q, p, 900, 5, normalize_db=True, db=d))
    else:
        inputs = [q70, planes]
        flagged = _with(lambda q, p: ops.topk_indexed(q, p, 900, 5, normalize_db=True, rescore_planes=True, no_wait=True))
        waiting = _with(lambda q, p: ops.topk_indexed(q, p, 900, 5, normalize_db=True, rescore_planes=True))
    tags = H.tags_of(waiting, inputs)                        # the waiting call tells whether this input overflows
    assert "topk_screen_gemm" in tags and ("topk_scores_gemm" in tags) == overflow, sorted(tags)
    assert "topk_screen_gemm" in H.tags_of(flagged, inputs)
    H.run_case(f"topk_nowait_{how}_{'overflow' if overflow else 'calm'}", flagged, inputs, asynchronous=True)


def test_two_flagged_flat_indexes_on_two_streams():
    import _stream_harness as H
    from anyloc_amd import ops, retrieval
    q1, q2 = _unit(70, 256, seed=130), _unit(70, 256, seed=170)
    d1, d2 = _stream_data(900, 131, q1[0]), _stream_data(300, 171)      # one overflows, one does not
    with ops.options(**SCREEN):
        i1, i2 = retrieval.FlatIndex(d1, "cosine", True, planes=True), retrieval.FlatIndex(d2, "cosine", True, planes=True)
    torch.cuda.synchronize()
    op_a, op_b = _with(lambda q: i1.search(q, 5, no_wait=True)), _with(lambda q: i2.search(q, 5, no_wait=True))
    assert "topk_screen_gemm" in H.tags_of(op_a, [q1]) and "topk_screen_gemm" in H.tags_of(op_b, [q2])
    H.run_two_streams("two_flat_indexes_screened_nowait", op_a, [q1], op_b, [q2], asynchronous=True)


# ---- 8. guard bands ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overflow", [False, True], ids=["calm", "overflow"])
def test_a_flagged_call_writes_only_its_lists_and_its_workspace(overflow):
    """dist, idx and a workspace of exactly anyloc_topk_workspace_bytes inside the arena of tests/_guard_arena.py: no guard
    byte moves, every list entry is written, and the lists are those of the ordinary call."""
    from _guard_arena import ALIGN, GUARD, Arena
    from anyloc_amd import _lib, ops
    lib = _lib.load()
    nq, ndb, dim, k = 300, 17000, 4096, 20
    qu, db = R.planted_rows(nq, ndb, dim, 77)
    if overflow:
        qu[3] = 0.0
        db[100] = 3.0 * qu[0]
        db[3000:3700] = db[100].clone().expand(700, -1)
    qu0, db0 = qu.clone(), db.clone()

    def ptr(t):
        return C.c_void_p(t.data_ptr())
    with ops.options(**SCREEN):
        want_d, want_i = ops.topk(qu, db, k, "ip", normalize_db=True, no_wait=True)
        ws_bytes = lib.anyloc_topk_workspace_bytes(nq, ndb, dim, k)
        guard = max(GUARD, (256 * 8 * k + ALIGN) // ALIGN * ALIGN)       # more than one 256-row tile row of the widest output
        ar = Arena(DEV, ws_bytes + (8 << 20) + 4 * (guard + ALIGN), guard=guard)
        dist, idx = ar.output("dist", torch.float32, (nq, k)), ar.output("idx", torch.int64, (nq, k))
        ws = ar.workspace(ws_bytes)
        st = lib.anyloc_topk(ptr(qu), nq, ptr(db), ndb, dim, k, 0, ops.TOPK_NORMALIZE_DB | ops.TOPK_NO_WAIT, 0, ptr(dist), ptr(idx),
                             ptr(ws), ws.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert st == 0, lib.anyloc_last_error()
    assert ar.check({"dist": want_d, "idx": want_i}, {"idx": -1}) == []
    assert torch.equal(dist, want_d) and torch.equal(idx, want_i)
    assert torch.equal(qu, qu0) and torch.equal(db, db0)
