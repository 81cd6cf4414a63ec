"""Screened retrieval on rows wider than 49 152 columns (``pytest -m gpu``; ``screen_rescore_sliced_kernel`` and
``screen_rescore_planes_sliced_kernel`` of csrc/scores_screen.hip, option ``topk_rescore_cols``): the re-scoring kernels take
the query in column slices and add the slices' float64 totals in LDS, so the screened search serves every width the fp16 panels
serve.  Data recipe and float64 checker are those of tests/_retrieval_refs.py: planted neighbours at graded distances, a
float64 flat search (computed in blocks of 512 rows), distances within 3e-6 (inner product) / 1e-5 (L2) of it, a differing
index only where the two float64 scores are closer than that bar -- and (cap=0.001) at most 0.1 % of a case's list entries may
differ at all (a float64 search against itself gives 0; under fp32 rounding far less than one entry per case is expected).  Every case
asserts from the profile that the leading-plane GEMM ran and the exact one did not: no silent fallback.

The multi-slice path is reached at small shapes with ``topk_rescore_cols = 4096`` (8 208 columns: two slices and a 16-column
third) and by every shape above 49 152 columns under the default slice; ``topk_rescore_cols`` = 8 192 ... 45 056 reaches the
remaining instantiations of the two sliced kernels (test_every_slice_width_gives_the_lists_of_one_slice).  What no test here
reaches: TWO column ranges at > 65 535 columns -- more than 130 000 rows of >= 256 KiB each do not fit a seconds-long test; the sizes of that path are pinned
by tests/test_topk_wide_screen_cpu.py and it was run once by tools/time_wide_screen.py (profiles/wide_screen_timing.md)."""
import pytest
import torch

import _retrieval_refs as R
from _retrieval_refs import BAR

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCREEN = dict(topk_screen=1, topk_h3=1)


_CASE = {}


def _case(nq, ndb, dim, metric):
    """(queries, rows, float64 scores) of a shape, made once and shared by the tests that follow each other on it (one shape is
    kept: the widest holds 2.1 GB of rows)."""
    key = (nq, ndb, dim, metric)
    if key not in _CASE:
        _CASE.clear()
        qu, db = R.planted_rows(nq, ndb, dim, nq + ndb + dim)
        _CASE[key] = (qu, db, R.exact_scores64(qu, db, metric, block=512))
    return _CASE[key]


def _as_flat_index_scores_them(qu, db, s, metric):
    """FlatIndex.search normalises its queries (ops.l2norm_rows, which may move the last bit of a unit row): the queries it
    scores and their float64 scores"""
    from anyloc_amd import ops
    q = ops.l2norm_rows(qu)
    return q, (s if torch.equal(q, qu) else R.exact_scores64(q, db, metric, block=512))


def _screened(prof, rescore="topk_screen_rescore"):
    """the leading-plane GEMM ran, the exact one did not, and the candidates were re-scored by the kernel named"""
    other = {"topk_screen_rescore": "topk_screen_rescore_planes", "topk_screen_rescore_planes": "topk_screen_rescore"}[rescore]
    return "topk_screen_gemm" in prof and "topk_scores_gemm" not in prof and rescore in prof and other not in prof


def _three_searches(qu, db, k, metric):
    """the one-shot call, FlatIndex with its rows, FlatIndex without them -> [(tag, (d, i), profile)] under the options in force"""
    from anyloc_amd import ops, retrieval
    method = "cosine" if metric == "ip" else "l2"
    kept = retrieval.FlatIndex(db, method, True, planes=True)
    bare = retrieval.FlatIndex(db, method, True, keep_fp32=False, rescore="planes")
    assert kept.has_planes and kept.db is not None and bare.db is None
    out = []
    for tag, fn, rescore in (("one-shot", lambda: ops.topk(qu, db, k, metric, normalize_db=True), "topk_screen_rescore"),
                             ("rows kept", lambda: kept.search(qu, k), "topk_screen_rescore"),
                             ("rows free", lambda: bare.search(qu, k), "topk_screen_rescore_planes")):
        res, prof = R.profiled(fn)
        assert _screened(prof, rescore), (tag, sorted(prof))
        out.append((tag, res))
    return out


@pytest.mark.parametrize("nq,ndb,dim,k,metric", [(130, 9000, 8208, 20, "ip"),      # two slices and a 16-column third; two panels
                                                  (130, 9000, 8192, 10, "l2"),      # exactly two slices
                                                  (70, 300, 12304, 20, "ip")])      # fewer rows than a panel; four slices, the last 16 columns
def test_slices_of_4096_columns_give_the_lists_of_one_slice(nq, ndb, dim, k, metric):
    """``topk_rescore_cols = 4096`` sends narrow rows through the sliced kernels: against float64, and against the same call on
    the single-slice kernels (option 0) -- identical lists, distances within the bar (the float64 totals of the slices are added
    in another order than one pass adds them: the last bit of the fp32 value may differ)."""
    from anyloc_amd import ops
    qu, db, s = _case(nq, ndb, dim, metric)
    s_index = _as_flat_index_scores_them(qu, db, s, metric)[1]
    with ops.options(topk_rescore_cols=4096, **SCREEN):
        assert ops.get_option("topk_rescore_cols") == 4096
        sliced = _three_searches(qu, db, k, metric)
    assert ops.get_option("topk_rescore_cols") == 0
    with ops.options(**SCREEN):
        whole = _three_searches(qu, db, k, metric)
    for (tag, (d, i)), (_, (d1, i1)) in zip(sliced, whole):
        ref = s if tag == "one-shot" else s_index
        R.check_lists(d, i, ref, k, metric, f"{tag}, slices of 4096, {nq}x{ndb}x{dim} {metric}", cap=0.001)
        R.check_lists(d1, i1, ref, k, metric, f"{tag}, one slice, {nq}x{ndb}x{dim} {metric}", cap=0.001)
        assert torch.equal(i, i1), tag
        assert float((d - d1).abs().max()) <= BAR[metric], (tag, float((d - d1).abs().max()))


def _graded(nq, ndb, dim, seed):
    """(queries, rows) drawn with a CPU generator whose float64 cosines are PRESCRIBED: row r is Q^+ t_r plus a unit vector
    orthogonal to every query, so that q_i . d_r = t_r[i] -- per query a permutation of a ladder of ndb values, the best eight
    4e-5 apart (true neighbours closer to each other than the screening bound), the rest 6e-4 apart, all in [-0.09, 0.09] (the
    70 prescribed cosines of a row then take a quarter of its unit length).  No two scores of a query are closer than 4e-5
    (8e-5 under L2): 13 x / 8 x the bar, so no float64 near-tie can excuse a differing entry -- _no_near_ties asserts it on the
    fp32 data.  Rows are then scaled by 0.3 ... 2.3 as in _data (the search normalises them)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.nn.functional.normalize(torch.randn(nq, dim, generator=g, dtype=torch.float64))
    ladder = 0.09 - torch.cat([4e-5 * torch.arange(8, dtype=torch.float64), 4e-5 * 8 + 6e-4 * torch.arange(ndb - 8, dtype=torch.float64)])
    t = torch.stack([ladder[torch.randperm(ndb, generator=g)] for _ in range(nq)])         # [nq, ndb]: t[i, r] = q_i . d_r
    gram = q @ q.t()
    in_span = torch.linalg.solve(gram, t).t() @ q                                          # [ndb, dim]: Q^+ t_r
    n = torch.randn(ndb, dim, generator=g, dtype=torch.float64)
    n = torch.nn.functional.normalize(n - torch.linalg.solve(gram, q @ n.t()).t() @ q)    # unit, orthogonal to every query
    left = 1.0 - (in_span * in_span).sum(1, keepdim=True)
    assert float(left.min()) > 0.5
    d = (in_span + left.sqrt() * n) * (0.3 + 2.0 * torch.rand(ndb, 1, generator=g, dtype=torch.float64))
    return q.float().to(DEV), d.float().to(DEV)


def _no_near_ties(s, k, metric):
    """the best k + 1 float64 scores of every query lie further apart than four bars -> the smallest gap"""
    top = torch.sort(s, dim=1, descending=True).values[:, :k + 1]
    gap = float((top[:, :-1] - top[:, 1:]).min())
    assert gap > 4 * BAR[metric], gap
    return gap


# option value -> the instantiations it selects: NJ of screen_rescore_sliced_kernel (2 048 columns per register group; 12 288 is
# six groups in the <8> kernel, 20 480 ten in the <16>, 45 056 twenty-two in the <24>) and NU of
# screen_rescore_planes_sliced_kernel (4 096 columns per group, slices capped at 32 768)
SLICE_WIDTHS = {8192: (4, 2), 12288: (8, 4), 16384: (8, 4), 20480: (16, 8), 32768: (16, 8), 45056: (24, 8)}
SLICED = [(cols, cols + 16, "ip") for cols in SLICE_WIDTHS] + [(cols, 2 * cols, "l2") for cols in (8192, 16384)]


@pytest.mark.parametrize("cols,dim,metric", SLICED)
def test_every_slice_width_gives_the_lists_of_one_slice(cols, dim, metric):
    """``topk_rescore_cols`` from 8 192 to 45 056: every instantiation of the two sliced re-scoring kernels that the 4 096-column
    and default slices of the tests above leave out (SLICE_WIDTHS), on 70 queries x 300 rows: one full slice and a 16-column one
    (inner product), exactly two slices (L2).  One-shot, rows kept and rows free, each against float64 under the bars of
    test_slices_of_4096_columns_give_the_lists_of_one_slice and against the same call on the single-slice kernels (option 0):
    identical index lists, distances within the bar.  The data (_graded) has no float64 near-tie, so _check's allowance for
    differing entries is not drawn on: not one entry may differ."""
    from anyloc_amd import ops
    nq, ndb, k = 70, 300, 20
    nj, nu = SLICE_WIDTHS[cols]
    assert (cols // 4 + 511) // 512 in range(nj // 2 + 1, nj + 1) and (min(cols, 32768) // 8 + 511) // 512 in range(nu // 2 + 1, nu + 1)
    _CASE.clear()
    qu, db = _graded(nq, ndb, dim, 1000 + cols // 4096 + (0 if metric == "ip" else 50))
    s = R.exact_scores64(qu, db, metric, block=512)
    s_index = _as_flat_index_scores_them(qu, db, s, metric)[1]
    print(f"smallest gap among the best {k + 1}: {_no_near_ties(s, k, metric):.2e}, as the index scores them {_no_near_ties(s_index, k, metric):.2e}")
    with ops.options(topk_rescore_cols=cols, **SCREEN):
        assert ops.get_option("topk_rescore_cols") == cols
        sliced = _three_searches(qu, db, k, metric)
    assert ops.get_option("topk_rescore_cols") == 0
    with ops.options(**SCREEN):
        whole = _three_searches(qu, db, k, metric)
    for (tag, (d, i)), (_, (d1, i1)) in zip(sliced, whole):
        ref = s if tag == "one-shot" else s_index
        assert R.check_lists(d, i, ref, k, metric, f"{tag}, slices of {cols}, {nq}x{ndb}x{dim} {metric}", cap=0.001) == 0
        assert R.check_lists(d1, i1, ref, k, metric, f"{tag}, one slice, {nq}x{ndb}x{dim} {metric}", cap=0.001) == 0
        assert torch.equal(i, i1), tag
        assert float((d - d1).abs().max()) <= BAR[metric], (tag, float((d - d1).abs().max()))


WIDE = [(130, 4000, 131072, 20, "ip"),                     # a full 3 840-row panel and a ragged one; three slices
        (130, 4000, 131072, 20, "l2"),
        (70, 3000, 65536, 5, "ip"),                        # one ragged 7 936-row panel; two slices, the second 16 384 columns
        (100, 2700, 196608, 20, "ip"),                     # a 2 560-row panel and a ragged one; exactly four slices
        (100, 4000, 81920, 20, "ip")]                      # one ragged 6 400-row panel


@pytest.mark.parametrize("nq,ndb,dim,k,metric", WIDE)
def test_wide_rows_screened_give_the_exact_lists(nq, ndb, dim, k, metric):
    """Default slice (49 152 columns), topk_screen = 1: against float64 and against the unscreened panels; a second call gives
    the same bits; ``index_base`` shifts the indices and nothing else."""
    from anyloc_amd import ops
    qu, db, s = _case(nq, ndb, dim, metric)
    with ops.options(**SCREEN):
        (d, i), prof = R.profiled(lambda: ops.topk(qu, db, k, metric, normalize_db=True))
        assert _screened(prof), sorted(prof)
        d_again, i_again = ops.topk(qu, db, k, metric, normalize_db=True)
        assert torch.equal(d, d_again) and torch.equal(i, i_again)
        d_b, i_b = ops.topk(qu, db, k, metric, normalize_db=True, index_base=5000)
        assert torch.equal(torch.where(i_b >= 0, i_b - 5000, i_b), i) and torch.equal(d_b, d)
    with ops.options(topk_screen=0, topk_h3=1):
        (d0, i0), prof0 = R.profiled(lambda: ops.topk(qu, db, k, metric, normalize_db=True))
    assert "topk_scores_gemm" in prof0 and "topk_screen_gemm" not in prof0, sorted(prof0)
    n = R.check_lists(d, i, s, k, metric, f"screened {nq}x{ndb}x{dim} {metric}", cap=0.001)
    n0 = R.check_lists(d0, i0, s, k, metric, f"unscreened {nq}x{ndb}x{dim} {metric}", cap=0.001)
    assert float((d - d0).abs().max()) <= BAR[metric]
    assert int((i != i0).sum()) <= n + n0                  # a differing pair differs from the float64 list on one side at least


def test_wide_rows_screened_on_an_index_without_its_rows():
    """(130, 4000, 131 072) through ``FlatIndex(rescore="planes", keep_fp32=False)``: the planes variant, in four slices of 32 768
    columns, against float64 and against the one-shot call on the rows."""
    from anyloc_amd import ops, retrieval
    nq, ndb, dim, k = WIDE[0][:4]
    qu, db, s = _case(nq, ndb, dim, "ip")
    q, s = _as_flat_index_scores_them(qu, db, s, "ip")
    with ops.options(**SCREEN):
        bare = retrieval.FlatIndex(db, "cosine", True, keep_fp32=False, rescore="planes")
        assert bare.db is None
        (d, i), prof = R.profiled(lambda: bare.search(qu, k))
        assert _screened(prof, "topk_screen_rescore_planes"), sorted(prof)
        d_again, i_again = bare.search(qu, k)
        assert torch.equal(d, d_again) and torch.equal(i, i_again)
        d1, i1 = ops.topk(q, db, k, "ip", normalize_db=True)
    n = R.check_lists(d, i, s, k, "ip", "rows free, 131 072 columns", cap=0.001)
    n1 = R.check_lists(d1, i1, s, k, "ip", "one-shot, 131 072 columns", cap=0.001)
    assert float((d - d1).abs().max()) <= BAR["ip"] and int((i != i1).sum()) <= n + n1


def test_wide_rows_without_the_wait():
    """ANYLOC_TOPK_NO_WAIT at 131 072 columns with one all-zero query (every row ties inside its bound: more than 512
    candidates): its list is the unscreened call's, from the side batch of 64 x 131 072 floats; every other query keeps the
    bits the screened search gives it in a call without the zero query."""
    from anyloc_amd import ops
    nq, ndb, dim, k = WIDE[0][:4]
    clean, db, s = _case(nq, ndb, dim, "ip")
    qu = clean.clone()
    qu[7] = 0.0
    with ops.options(**SCREEN):
        d, i = ops.topk(qu, db, k, "ip", normalize_db=True, no_wait=True)
        (d_w, i_w), prof = R.profiled(lambda: ops.topk(qu, db, k, "ip", normalize_db=True))
        assert "topk_screen_gemm" in prof and "topk_scores_gemm" in prof, sorted(prof)     # the waiting call falls back for everyone
        (d_c, i_c), prof_c = R.profiled(lambda: ops.topk(clean, db, k, "ip", normalize_db=True))
        assert _screened(prof_c), sorted(prof_c)
    with ops.options(topk_screen=0, topk_h3=1):
        d0, i0 = ops.topk(qu, db, k, "ip", normalize_db=True)
    assert torch.equal(i[7], i0[7]) and torch.equal(d[7], d0[7])
    assert torch.equal(i[7], torch.arange(k, device=DEV)) and bool((d[7] == 0).all())       # every row ties at 0: lower index first
    keep = torch.ones(nq, dtype=torch.bool, device=DEV)
    keep[7] = False
    assert torch.equal(d[keep], d_c[keep]) and torch.equal(i[keep], i_c[keep])
    s_z = s.clone()
    s_z[7] = 0.0
    R.check_lists(d, i, s_z, k, "ip", "no wait, one zero query", cap=0.001)


def test_narrow_rows_under_default_options_are_unchanged():
    """(300, 20 000, 4096) screens by default, on the single-slice kernels as before: the same checks; and the slice option is
    back at 0 once its context has exited."""
    from anyloc_amd import ops
    nq, ndb, dim, k = 300, 20000, 4096, 20
    with ops.options(topk_rescore_cols=4096):
        assert ops.get_option("topk_rescore_cols") == 4096
    assert ops.get_option("topk_rescore_cols") == 0
    qu, db, s = _case(nq, ndb, dim, "ip")
    (d, i), prof = R.profiled(lambda: ops.topk(qu, db, k, "ip", normalize_db=True))
    assert _screened(prof), sorted(prof)
    d_again, i_again = ops.topk(qu, db, k, "ip", normalize_db=True)
    assert torch.equal(d, d_again) and torch.equal(i, i_again)
    with ops.options(topk_screen=0):
        d0, i0 = ops.topk(qu, db, k, "ip", normalize_db=True)
    n = R.check_lists(d, i, s, k, "ip", "narrow rows, defaults", cap=0.001)
    n0 = R.check_lists(d0, i0, s, k, "ip", "narrow rows, unscreened", cap=0.001)
    assert float((d - d0).abs().max()) <= BAR["ip"] and int((i != i0).sum()) <= n + n0
    _CASE.clear()
