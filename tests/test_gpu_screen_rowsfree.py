"""Screened retrieval on an index that no longer keeps its fp32 rows (``pytest -m gpu``; ANYLOC_TOPK_RESCORE_PLANES,
``screen_rescore_planes_kernel`` of csrc/scores_screen.hip, ``retrieval.FlatIndex(rescore="planes")``,
``anyloc_topk_index_build_range`` / ``FlatIndex.from_chunks``).  The candidates of the screened search are re-scored from the
two fp16 planes of the index in float64: the lists are the float64-exact ones over the 22-bit rows the index holds, which lie
within 1e-7 (normalised score; tests/test_screen_rowsfree_cpu.py) of the fp32 rows -- so they are checked against a float64
flat search over the fp32 rows with the bars and the near-tie rule of tests/_retrieval_refs.py (3e-6 inner product, 1e-5 L2; a
differing index only where the two float64 scores are closer than the bar).

A cap on what the near-tie rule may excuse (check_lists' cap="gaps"): the excused entries of a case are counted and must not exceed
2 x (adjacent gaps below g in the exact float64 top-(k+1) lists), g = 3e-7 (inner product) / 1e-6 (L2), times the scale of
the queries where they are not unit vectors.  Why: a rows-free score is within 1e-7 of the fp32-exact one, the compared value
is rounded to fp32 once (6e-8 at 1; a few such roundings on values up to 4 for L2), and one swapped pair is two entries."""
import os

import numpy as np
import pytest
import torch

import _ranks
import _retrieval_refs as R
from _retrieval_refs import _rows_free

pytestmark = pytest.mark.gpu
DEV = "cuda"

# the shapes of test_screened_search_gives_the_exact_lists (seed nq + ndb + dim) and of
# test_screened_search_chunk_edges_and_query_norms (seed nq + dim, scaled queries) of tests/test_gpu_screen.py
SHAPES = [(600, 20000, 4096, 20, "ip", 1.0, None), (600, 20000, 4096, 20, "l2", 1.0, None), (257, 9000, 1024, 5, "ip", 1.0, None),
          (300, 140000, 512, 10, "ip", 1.0, None), (130, 300, 2048, 20, "ip", 1.0, None), (70, 12, 256, 20, "l2", 1.0, None),
          (1000, 10000, 49152, 20, "ip", 1.0, None),
          (300, 20000, 4112, 20, "ip", 1.0, "edge"), (300, 20000, 24592, 10, "l2", 1.0, "edge"),
          (260, 18000, 8192, 20, "l2", 7.5, "edge"), (260, 18000, 8192, 128, "ip", 0.01, "edge")]


@pytest.mark.parametrize("nq,ndb,dim,k,metric,qscale,kind", SHAPES)
def test_rows_free_screened_search_gives_the_exact_lists(nq, ndb, dim, k, metric, qscale, kind):
    """``FlatIndex(db, ..., keep_fp32=False, rescore="planes")`` under topk_screen = 1: no rows kept, the search runs screened
    and re-scores from the planes, without fallback; its lists pass the float64 check over the fp32 rows; deterministic;
    ``index_base`` shifts the indices and nothing else.  Every shape class: several panels, a short last panel, two column
    ranges (140 000 rows), fewer rows than k, k = 128, queries that are not unit vectors, L2, 1 000 x 10 000 x 49 152."""
    from anyloc_amd import ops, retrieval
    qu, db = R.planted_rows(nq, ndb, dim, nq + dim if kind == "edge" else nq + ndb + dim)
    method = "cosine" if metric == "ip" else "l2"
    with ops.options(topk_screen=1, topk_h3=1):
        index = retrieval.FlatIndex(db, method, True, planes=True, keep_fp32=False, rescore="planes")
        assert index.db is None and index.has_planes and index.planes.numel() == ops.topk_index_bytes(ndb, dim)
        if qscale == 1.0:
            q = ops.l2norm_rows(qu)                        # the queries FlatIndex.search scores (F.normalize of the reference)
            (d, i), prof = R.profiled(lambda: index.search(qu, k))
        else:                                              # FlatIndex normalises its queries: scaled ones go through ops
            q = qu * qscale
            (d, i), prof = R.profiled(lambda: ops.topk_indexed(q, index.planes, ndb, k, metric, normalize_db=True, rescore_planes=True))
        assert _rows_free(prof), sorted(prof)
        d_again, i_again = ops.topk_indexed(q, index.planes, ndb, k, metric, normalize_db=True, rescore_planes=True)
        assert torch.equal(d, d_again) and torch.equal(i, i_again)                              # deterministic, and one path
        d_b, i_b = ops.topk_indexed(q, index.planes, ndb, k, metric, index_base=5000, normalize_db=True, rescore_planes=True)
        assert torch.equal(torch.where(i_b >= 0, i_b - 5000, i_b), i) and torch.equal(d_b, d)
    scale = (max(1.0, qscale * qscale) if metric == "l2" else qscale)                           # (as the existing file scales its bars)
    R.check_lists(d, i, R.exact_scores64(q, db, metric), k, metric, f"rows-free {nq}x{ndb}x{dim} k={k} {metric} x{qscale}", scale=scale, cap="gaps")


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_rows_free_screened_search_on_raw_rows(metric):
    """Without ANYLOC_TOPK_NORMALIZE_DB (``norm_descs=False``): the rows count with their raw norms (0.3 ... 5.5); bars and gap
    scale with the largest one (squared for L2), as tests/test_gpu_screen.py::test_screened_search_on_raw_rows.  (Raw row norms
    reach 150 here, so for L2 the scaled gap is wide and the cap on excused entries says little on this shape; the normalised
    shapes above are where it bites.)"""
    from anyloc_amd import ops, retrieval
    qu, db = R.planted_rows(400, 20000, 4096, 21)
    with ops.options(topk_screen=1, topk_h3=1):
        index = retrieval.FlatIndex(db, "cosine" if metric == "ip" else "l2", False, keep_fp32=False, rescore="planes")
        assert index.db is None
        (d, i), prof = R.profiled(lambda: index.search(qu, 20))
    assert _rows_free(prof), sorted(prof)
    scale = float(db.double().norm(dim=1).max()) ** (2 if metric == "l2" else 1)
    R.check_lists(d, i, R.exact_scores64(qu, db, metric, normalize=False), 20, metric, f"rows-free raw rows {metric}", scale=scale, cap="gaps")


@pytest.mark.parametrize("nq,ndb,dim,k,metric", [(600, 20000, 4096, 20, "ip"), (600, 20000, 4096, 20, "l2"), (1000, 10000, 49152, 20, "ip")])
def test_rows_free_against_the_rows_kept_screened_search(nq, ndb, dim, k, metric):
    """The two re-scorings on ONE index: distances within the bar, indices equal except at float64 near-ties (capped)."""
    from anyloc_amd import ops
    qu, db = R.planted_rows(nq, ndb, dim, nq + ndb + dim)
    planes = ops.topk_index_build(db)
    with ops.options(topk_screen=1, topk_h3=1):
        (d_r, i_r), prof_r = R.profiled(lambda: ops.topk_indexed(qu, planes, ndb, k, metric, normalize_db=True, db=db))
        (d_p, i_p), prof_p = R.profiled(lambda: ops.topk_indexed(qu, planes, ndb, k, metric, normalize_db=True, rescore_planes=True))
    assert "topk_screen_rescore" in prof_r and "topk_screen_rescore_planes" not in prof_r and "topk_scores_gemm" not in prof_r
    assert _rows_free(prof_p), sorted(prof_p)
    diff = float((d_r - d_p).abs().max())
    print(f"rows-free vs rows-kept {nq}x{ndb}x{dim} {metric}: max |distance difference| {diff:.3e}, {int((i_r != i_p).sum())} indices differ")
    assert diff <= R.BAR[metric]
    s = R.exact_scores64(qu, db, metric)
    n_r = R.check_lists(d_r, i_r, s, k, metric, "rows-kept", cap="gaps")
    n_p = R.check_lists(d_p, i_p, s, k, metric, "rows-free", cap="gaps")
    assert int((i_r != i_p).sum()) <= n_r + n_p                    # a differing pair differs from the float64 list on one side at least


def test_the_flag_with_the_rows_at_hand_reads_the_planes():
    """``anyloc_topk_search_index_rows`` + ANYLOC_TOPK_RESCORE_PLANES through the C ABI: the rows are given and not read -- the
    kernel and the bits of the rows-free call."""
    from anyloc_amd import _lib, ops
    nq, ndb, dim, k = 520, 17000, 4096, 20
    qu, db = R.planted_rows(nq, ndb, dim, 9)
    planes = ops.topk_index_build(db)
    lib = _lib.load()
    with ops.options(topk_screen=1, topk_h3=1):
        d0, i0 = ops.topk_indexed(qu, planes, ndb, k, "ip", normalize_db=True, rescore_planes=True)
        ws = torch.empty(lib.anyloc_topk_index_workspace_bytes(nq, ndb, dim, k), dtype=torch.uint8, device=DEV)
        out = {}
        for name, rows in (("search_index_rows", db), ("search_index", None)):
            d = torch.empty(nq, k, dtype=torch.float32, device=DEV)
            i = torch.empty(nq, k, dtype=torch.int64, device=DEV)
            common = (ndb, dim, k, 0, ops.TOPK_NORMALIZE_DB | ops.TOPK_RESCORE_PLANES, 0, _lib.ptr(d), _lib.ptr(i), _lib.ptr(ws), ws.numel(),
                      _lib.stream_ptr())

            def call():
                if rows is None:
                    return lib.anyloc_topk_search_index(_lib.ptr(qu), nq, _lib.ptr(planes), *common)
                return lib.anyloc_topk_search_index_rows(_lib.ptr(qu), nq, _lib.ptr(rows), _lib.ptr(planes), *common)
            st, prof = R.profiled(call)
            assert st == 0, lib.anyloc_last_error()
            assert _rows_free(prof), (name, sorted(prof))
            out[name] = (d, i)
    for name, (d, i) in out.items():
        assert torch.equal(d, d0) and torch.equal(i, i0), name
    st = lib.anyloc_topk(_lib.ptr(qu), nq, _lib.ptr(db), ndb, dim, k, 0, ops.TOPK_NORMALIZE_DB | ops.TOPK_RESCORE_PLANES, 0, _lib.ptr(d0),
                         _lib.ptr(i0), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    assert st == -1 and b"ANYLOC_TOPK_RESCORE_PLANES" in lib.anyloc_last_error()


def test_rows_free_ties_and_overflow():
    """Exact duplicates of a query's best rows: lower index first; 40 copies fit the candidate list.  700 copies do not: the
    call falls back to the unscreened indexed search and gives the bits of ``FlatIndex(keep_fp32=False)`` without the flag."""
    from anyloc_amd import ops, retrieval
    qu, db = R.planted_rows(300, 12000, 2048, 5, planted=False)
    db[100] = 3.0 * qu[0]
    copies = torch.arange(200, 240, device=DEV)
    db[copies] = db[100].clone().expand(len(copies), -1)
    q = ops.l2norm_rows(qu)
    with ops.options(topk_screen=1, topk_h3=1):
        index = retrieval.FlatIndex(db, "cosine", True, keep_fp32=False, rescore="planes")
        (d, i), prof = R.profiled(lambda: index.search(qu, 20))
    assert _rows_free(prof), sorted(prof)
    assert i[0, 0] == 100 and torch.equal(i[0, 1:20], copies[:19])
    R.check_lists(d, i, R.exact_scores64(q, db, "ip"), 20, "ip", "rows-free duplicates", cap="gaps")
    db[3000:3700] = db[100].clone().expand(700, -1)
    with ops.options(topk_screen=1, topk_h3=1):
        index = retrieval.FlatIndex(db, "cosine", True, keep_fp32=False, rescore="planes")
        (d, i), prof = R.profiled(lambda: index.search(qu, 20))
        assert "topk_screen_gemm" in prof and "topk_scores_gemm" in prof, sorted(prof)            # screened first, then the fallback
        bare = retrieval.FlatIndex(db, "cosine", True, planes=True, keep_fp32=False)
        d0, i0 = bare.search(qu, 20)
    assert torch.equal(d, d0) and torch.equal(i, i0)


def _build_zeroed(db):
    """anyloc_topk_index_build into a ZERO-FILLED buffer (slot and array padding defined: buffers can be compared whole)."""
    from anyloc_amd import _lib, ops
    ndb, dim = db.shape
    index = torch.zeros(ops.topk_index_bytes(ndb, dim), dtype=torch.uint8, device=db.device)
    _lib.check(_lib.load().anyloc_topk_index_build(_lib.ptr(db), ndb, dim, _lib.ptr(index), index.numel(), _lib.stream_ptr()), "build")
    return index


@pytest.mark.parametrize("ndb,dim,pieces", [(20000, 4096, [(0, 8192), (8192, 11808)]),            # one panel; a panel and the short tail
                                            (20000, 4096, [(16384, 3616), (0, 16384)]),           # the tail first; several panels
                                            (9001, 1024, [(0, 8192), (8192, 809)]),
                                            (9001, 1024, [(0, 9001)])])
def test_index_built_by_ranges_is_the_index_built_at_once(ndb, dim, pieces):
    from anyloc_amd import ops
    qu, db = R.planted_rows(300, ndb, dim, ndb + dim)
    assert ops.topk_index_panel(dim) == 8192
    whole = _build_zeroed(db)
    parts = torch.zeros_like(whole)
    for row0, n in pieces:
        ops.topk_index_build_range(parts, db[row0:row0 + n], row0, ndb)
    torch.cuda.synchronize()
    assert torch.equal(whole, parts)
    for screen, flag in ((0, False), (1, True)):
        with ops.options(topk_screen=screen, topk_h3=1):
            (d0, i0), prof = R.profiled(lambda: ops.topk_indexed(qu, whole, ndb, 20, "ip", normalize_db=True, rescore_planes=flag))
            d1, i1 = ops.topk_indexed(qu, parts, ndb, 20, "ip", normalize_db=True, rescore_planes=flag)
        assert _rows_free(prof) if screen else ("topk_scores_gemm" in prof and "topk_screen_gemm" not in prof), sorted(prof)
        assert torch.equal(d0, d1) and torch.equal(i0, i1), screen
    for bad in ((100, 8192), (8192, 5000), (16384, 8192)):             # the C ABI's range rules, with real pointers
        with pytest.raises(Exception):
            ops.topk_index_build_range(parts, db[:bad[1]], bad[0], ndb)


@pytest.mark.parametrize("ndb,dim,where", [(20000, 4096, "cpu"), (20000, 4096, "cuda"), (9001, 1024, "mixed")])
def test_flat_index_from_chunks(ndb, dim, where):
    """Ragged chunks, on the host or the device: the rows-free index of the whole database, bit for bit."""
    from anyloc_amd import ops, retrieval
    qu, db = R.planted_rows(300, ndb, dim, ndb + dim + 1)
    lens = [1, 5000, 3191, 8192, 17, ndb]                               # cut points: inside panels, on a boundary, across two
    chunks, r0 = [], 0
    for n, ln in enumerate(lens):
        c = db[r0:r0 + ln]
        if c.shape[0]:
            chunks.append(c.cpu() if where == "cpu" or (where == "mixed" and n % 2) else c)
        r0 += ln
    before = torch.cuda.memory_allocated()
    index = retrieval.FlatIndex.from_chunks(iter(chunks), ndb, dim)
    held = torch.cuda.memory_allocated() - before
    assert index.db is None and index.rescore == "planes" and index.ntotal == ndb and index.dim == dim
    assert held <= ops.topk_index_bytes(ndb, dim) + (1 << 20)          # the stage is gone: 4 bytes per element
    ref = retrieval.FlatIndex(db, "cosine", True, keep_fp32=False, rescore="planes")
    for screen in (1, 0):
        with ops.options(topk_screen=screen, topk_h3=1):
            (d, i), prof = R.profiled(lambda: index.search(qu, 20))
            d0, i0 = ref.search(qu, 20)
        assert ("topk_screen_rescore_planes" in prof) == bool(screen)
        assert torch.equal(d, d0) and torch.equal(i, i0), screen
    R.check_lists(d, i, R.exact_scores64(ops.l2norm_rows(qu), db, "ip"), 20, "ip", "from_chunks, unscreened", cap="gaps")
    with pytest.raises(ValueError):
        retrieval.FlatIndex.from_chunks(iter(chunks[:-1]), ndb, dim)    # rows missing
    with pytest.raises(ValueError):
        retrieval.FlatIndex.from_chunks(iter(chunks + [db[:3]]), ndb, dim)
    with pytest.raises(ValueError):
        retrieval.FlatIndex(db[:, :24], "cosine", True, rescore="planes")


def test_default_index_without_rows_still_searches_unscreened():
    """``rescore`` defaults to "rows": today's object -- without its rows it scores on the three-product panels."""
    from anyloc_amd import ops, retrieval
    qu, db = R.planted_rows(520, 17000, 4096, 9)
    with ops.options(topk_screen=1):
        bare = retrieval.FlatIndex(db, "cosine", True, planes=True, keep_fp32=False)
        assert bare.rescore == "rows" and bare.db is None
        (d, i), prof = R.profiled(lambda: bare.search(qu, 20))
    assert "topk_scores_gemm" in prof and "topk_screen_gemm" not in prof and "topk_screen_rescore_planes" not in prof, sorted(prof)
    with ops.options(topk_screen=0):
        d0, i0 = retrieval.search(db, qu, 20)
    assert torch.equal(d, d0) and torch.equal(i, i0)


# ------------------------------------------------------------------------------------------------------------- sharded
def _rows_free_job(rank, world, out_dir):
    """The screened shard job of the overlapped sharded step (test_overlapped_sharded_step_with_the_screened_shard_search), with
    shards that keep no rows."""
    from anyloc_amd import ops, retrieval
    dev = torch.device("cuda", 0)
    dim = 4096
    db, qu = R.spread_rows(36000, dim, 7), R.spread_rows(600, dim, 8)
    bounds = [0, 17000, 36000]
    with ops.options(topk_screen=1, topk_h3=1):
        shard = retrieval.FlatIndex(db[bounds[rank]:bounds[rank + 1]].to(dev), "cosine", keep_fp32=False, rescore="planes")
        assert shard.db is None
        q_loc = qu[300 * rank:300 * (rank + 1)].to(dev)
        outs = [retrieval.sharded_search(shard, bounds[rank], q_loc, 20, counts=[300, 300], overlap=ov) for ov in (True, False)]
        _, prof = R.profiled(lambda: retrieval.sharded_search(shard, bounds[rank], q_loc, 20, counts=[300, 300], overlap=True))
    assert _rows_free(prof), sorted(prof)
    if rank == 0:
        s = R.exact_scores64(ops.l2norm_rows(qu.to(dev)), db.to(dev), "ip")
        for (d, i), tag in zip(outs, ("overlapped", "plain")):
            R.check_lists(torch.as_tensor(d, device=dev), torch.as_tensor(i, device=dev), s, 20, "ip", f"rows-free shards, {tag}", cap="gaps")
        assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][0], outs[1][0])
        open(os.path.join(out_dir, "ok_rows_free"), "w").write("1")


def test_sharded_step_on_rows_free_shards_two_ranks_one_gpu(tmp_path):
    _ranks.run_ranks(_rows_free_job, 2, tmp_path)
    assert (tmp_path / "ok_rows_free").exists()
