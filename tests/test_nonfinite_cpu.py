"""tests/_nonfinite_cases.py tested on the CPU, in the way tests/test_refs_cpu.py tests the list checker: every checker passes
the float64 reference itself and fails on each planted defect -- a leak into one clean element, a missing NaN, an extra NaN, a
label of -1, an index out of range, a NaN row listed first -- and the generators put their value where they say."""
import math

import pytest
import torch

import _nonfinite_cases as NF
import _retrieval_refs as R

METRICS = ["ip", "l2"]


# ------------------------------------------------------------------------------------------------------- generators
@pytest.mark.parametrize("value", list(NF.VALUES))
@pytest.mark.parametrize("where,col", [("first", 0), ("last", 63), ("col16", 16)])
def test_plant_and_twin_differ_in_one_element(value, where, col):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(70, 64, generator=g)
    bad, twin = NF.plant(x, 15, where, value), NF.clean_twin(x, 15, where)
    diff = NF.bits(bad) != NF.bits(twin)
    assert diff.nonzero().tolist() == [[15, col]]
    assert float(twin[15, col]) == NF.FILL
    v = float(bad[15, col])
    assert math.isnan(v) if value == "nan" else v == NF.VALUES[value]
    assert NF.same_bits(x, NF.plant(x, 15, where, float(x[15, col])))          # the input itself is not written


def test_plant_in_a_column_block_of_one_token():
    """the attention cases: q, k or v of one token of image 1 -- a unit that is not contiguous in the batch"""
    x = torch.zeros(3, 40, 3 * 128)
    for part, (first, last) in enumerate([(0, 127), (128, 255), (256, 383)]):
        unit = (1, 7, slice(128 * part, 128 * (part + 1)))
        assert torch.isnan(NF.plant(x, unit, "first", "nan")).nonzero().tolist() == [[1, 7, first]]
        assert torch.isinf(NF.plant(x, unit, "last", "+inf")).nonzero().tolist() == [[1, 7, last]]
        assert torch.isinf(NF.plant(x, unit, "col16", "-inf")).nonzero().tolist() == [[1, 7, first + 16]]


def test_split_view_turns_infinities_into_nan():
    x = torch.tensor([1.0, float("inf"), float("-inf"), float("nan"), -2.0])
    assert torch.isnan(NF.split_view(x)).tolist() == [False, True, True, True, False]
    assert NF.same_bits(NF.split_view(x)[[0, 4]], x[[0, 4]])


# -------------------------------------------------------------------------------------------------------- contained
def _gemm_case(value="nan"):
    """a [70, 64] x [200, 64]^T product whose row 15 holds ``value``: -> (fp32 'kernel' output, twin's, float64, mask)"""
    g = torch.Generator().manual_seed(2)
    a, w = torch.randn(70, 64, generator=g), torch.randn(200, 64, generator=g)
    bad, twin = NF.plant(a, 15, "col16", value), NF.clean_twin(a, 15, "col16")
    ref = bad.double() @ w.double().t()
    mask = torch.zeros(70, 1, dtype=torch.bool)
    mask[15] = True
    got = ref.float()
    clean = (twin.double() @ w.double().t()).float()
    return got, clean, ref, mask


@pytest.mark.parametrize("value", list(NF.VALUES))
def test_contained_passes_the_reference_itself(value):
    got, twin, ref, mask = _gemm_case(value)
    assert NF.contained(got, twin, ref, mask, tag=value) == 0.0
    n_bad = int((torch.isnan(ref) | torch.isinf(ref)).sum())
    assert n_bad == 200                                                     # the whole row, and nothing else


def test_contained_fails_on_a_leak_into_one_clean_element():
    got, twin, ref, mask = _gemm_case()
    got[16, 3] = torch.nextafter(got[16, 3], torch.tensor(float("inf")))    # one ulp, one element of the next row
    with pytest.raises(AssertionError, match="clean outputs differ"):
        NF.contained(got, twin, ref, mask, tag="leak")
    got, twin, ref, mask = _gemm_case()
    got[0, 0] = float("nan")
    with pytest.raises(AssertionError, match="clean outputs differ"):
        NF.contained(got, twin, ref, mask, tag="NaN leak")


def test_contained_fails_on_a_missing_nan():
    got, twin, ref, mask = _gemm_case()
    got[15, 199] = 1e12                                                     # x / eps instead of NaN
    with pytest.raises(AssertionError, match="not NaN where float64 is"):
        NF.contained(got, twin, ref, mask, tag="missing")


def test_contained_fails_on_an_extra_nan():
    got, twin, ref, mask = _gemm_case("+inf")
    assert not bool(torch.isnan(ref).any())
    got[15, 7] = float("nan")                                               # inf - inf where the formula has +-inf
    with pytest.raises(AssertionError, match="NaN where float64 is not"):
        NF.contained(got, twin, ref, mask, tag="extra")
    got, twin, ref, mask = _gemm_case("+inf")
    got[15, 7] = -got[15, 7]
    with pytest.raises(AssertionError, match="not the same infinity"):
        NF.contained(got, twin, ref, mask, tag="sign of an infinity")


def test_contained_holds_the_finite_spoiled_outputs_to_the_tolerance():
    g = torch.Generator().manual_seed(3)
    ref = torch.randn(6, 8, generator=g, dtype=torch.float64)
    ref[2, 0] = float("nan")
    mask = torch.zeros(6, 1, dtype=torch.bool)
    mask[2] = True
    got = ref.float()
    assert NF.contained(got, got.clone(), ref, mask, atol=1e-6, tag="within") <= 1e-6
    off = got.clone()
    off[2, 5] += 1e-3
    with pytest.raises(AssertionError):
        NF.contained(off, got, ref, mask, atol=1e-6, tag="finite spoiled output off")


# ----------------------------------------------------------------------------------------------------------- labels
def _scores():
    g = torch.Generator().manual_seed(4)
    s = torch.randn(300, 8, generator=g, dtype=torch.float64)
    s[7] = float("nan")                                                     # a bad row
    s[:, 5] = float("nan")                                                  # a bad centre
    s[11, 2] = float("inf")
    s[12, :5] = float("-inf")
    s[13, 3] = s[13].nan_to_num(-9.0).max()                                 # an exact tie: the first wins
    return s


def test_hard_assign_nan_never_picks_a_nan():
    s = _scores()
    lab = NF.hard_assign_nan(s)
    assert int(lab[7]) == 0 and not bool((lab == 5).any()) and int(lab[11]) == 2 and int(lab[12]) in (6, 7)
    assert int(lab[13]) == min(3, int(s[13].nan_to_num(-9.0).argmax()))
    assert int(torch.max(s, dim=1).indices[0]) == 5                         # torch ranks NaN first: the deliberate difference
    assert NF.check_labels(lab, s, 0.0, "reference") == 0


def test_check_labels_fails_on_a_label_of_minus_one_and_on_a_nan_winner():
    s = _scores()
    lab = NF.hard_assign_nan(s)
    for row, value, what in [(7, -1, "outside"), (20, 8, "outside"), (7, 3, "without label 0"), (20, 5, "NaN score won")]:
        bad = lab.clone()
        bad[row] = value
        with pytest.raises(AssertionError, match=what):
            NF.check_labels(bad, s, 0.0, what)
    bad = lab.clone()
    bad[30] = (int(lab[30]) + 1) % 5                                        # a number, but not the best one
    with pytest.raises(AssertionError):
        NF.check_labels(bad, s, 1e-6, "second best")


# ------------------------------------------------------------------------------------------------------------ lists
NQ, NDB, K = 8, 50, 5


def _ladder(metric, bad_row=None, bad_query=None, value=float("nan")):
    g = torch.Generator().manual_seed(NDB)
    top = 0.9 if metric == "ip" else -0.1
    s = torch.stack([(top - 1e-3 * torch.arange(NDB, dtype=torch.float64))[torch.randperm(NDB, generator=g)] for _ in range(NQ)])
    if bad_row is not None:
        s[:, bad_row] = value
    if bad_query is not None:
        s[bad_query] = float("nan")
    return s


@pytest.mark.parametrize("metric", METRICS)
def test_check_lists_nan_passes_the_reference_itself(metric):
    s = _ladder(metric, bad_row=17, bad_query=3)
    d, i = NF.flat_search_nan_last(s, K, metric)
    assert bool((i[3] == -1).all()) and bool((d[3] == NF.pad_distance(metric)).all())          # the tail rule: all padding
    assert not bool((i == 17).any())
    assert NF.check_lists_nan(d, i, s, K, metric, "reference", cap="gaps") == 0
    assert NF.check_lists_nan(d, torch.where(i >= 0, i + 1000, i), s, K, metric, "index_base", index_base=1000, cap="gaps") == 0
    # without a bad value it is check_lists
    clean = _ladder(metric)
    d, i = NF.flat_search_nan_last(clean, K, metric)
    assert NF.check_lists_nan(d, i, clean, K, metric, "clean", cap="gaps") == R.check_lists(d, i, clean, K, metric, "clean", cap="gaps") == 0


def test_infinite_scores_compare_as_numbers():
    s = _ladder("ip", bad_row=17, value=float("inf"))
    s[1, 17] = float("-inf")
    d, i = NF.flat_search_nan_last(s, K, "ip")
    assert bool((i[[0, 2, 3], 0] == 17).all()) and bool(torch.isinf(d[[0, 2, 3], 0]).all()) and not bool((i[1] == 17).any())
    assert NF.check_lists_nan(d, i, s, K, "ip", "+inf first") == 0
    d[0, 0], i[0, 0] = d[0, 1], i[0, 1]                                     # the +inf row dropped from one list
    with pytest.raises(AssertionError):
        NF.check_lists_nan(d, i, s, K, "ip", "+inf row missing")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("bad", [-2, NDB, NDB + 1000])
def test_check_lists_nan_fails_on_an_index_out_of_range(metric, bad):
    s = _ladder(metric, bad_row=17)
    d, i = NF.flat_search_nan_last(s, K, metric)
    i[4, 2] = bad
    with pytest.raises(AssertionError, match="outside the database"):
        NF.check_lists_nan(d, i, s, K, metric, "range")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("rank", [0, K - 1])
def test_check_lists_nan_fails_on_a_nan_row_that_is_listed(metric, rank):
    s = _ladder(metric, bad_row=17)
    d, i = NF.flat_search_nan_last(s, K, metric)
    i[2, rank], d[2, rank] = 17, float("nan")                               # rank 0: torch.sort's order, NaN first
    with pytest.raises(AssertionError, match="NaN score"):
        NF.check_lists_nan(d, i, s, K, metric, "NaN row listed")


@pytest.mark.parametrize("metric", METRICS)
def test_check_lists_nan_fails_on_a_bad_query_that_lists_a_row_and_on_a_short_list(metric):
    s = _ladder(metric, bad_query=3)
    d, i = NF.flat_search_nan_last(s, K, metric)
    i2 = i.clone()
    i2[3, 0] = 0
    with pytest.raises(AssertionError, match="NaN score"):
        NF.check_lists_nan(d, i2, s, K, metric, "bad query lists a row")
    d2 = d.clone()
    d2[3, 1] = 0.0
    with pytest.raises(AssertionError, match="padding distances"):
        NF.check_lists_nan(d2, i, s, K, metric, "padding distance")
    i3, d3 = i.clone(), d.clone()
    i3[5, K - 1], d3[5, K - 1] = -1, NF.pad_distance(metric)                # every list padding, as a NaN threshold would leave it
    with pytest.raises(AssertionError):
        NF.check_lists_nan(d3, i3, s, K, metric, "a full query with padding")


@pytest.mark.parametrize("nq,ndb,dim,k", [(5, 300, 2048, 20), (130, 300, 2048, 20)])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("metric", METRICS)
def test_fp32_search_over_the_gpu_shapes_stays_inside_the_gaps_cap(nq, ndb, dim, k, metric, normalize):
    """The recipe, the shapes and the near-tie policy (cap="gaps") of the GPU cases, with the bad row planted: a plain fp32
    search passes the checker against the float64 matrix, and the cap is not vacuous (it excuses a handful of entries at most)."""
    qu, db = R.planted_rows(nq, ndb, dim, nq + ndb + dim, device="cpu")
    db = NF.plant(db, 150, "col16", "nan")
    s = R.exact_scores64(qu, db, metric, normalize=normalize)
    assert bool(torch.isnan(s[:, 150]).all()) and int(torch.isnan(s).sum()) == nq
    rows = torch.nn.functional.normalize(db) if normalize else db
    s32 = qu @ rows.t()
    if metric == "l2":
        s32 = -((qu * qu).sum(1, keepdim=True) + (rows * rows).sum(1)[None, :] - 2.0 * s32)
    d, i = NF.flat_search_nan_last(s32.double(), k, metric)
    scale = 1.0 if normalize else float(db[torch.arange(ndb) != 150].double().norm(dim=1).max()) ** (2 if metric == "l2" else 1)
    excused = NF.check_lists_nan(d, i, s, k, metric, f"fp32 {nq}x{ndb}x{dim} {metric} normalize={normalize}", scale=scale, cap="gaps")
    assert excused <= 0.02 * nq * k
