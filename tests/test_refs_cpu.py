"""The shared references of the GPU tests, tested themselves on the CPU: the list checker of tests/_retrieval_refs.py passes the
exact lists and fails on every planted defect, under each of its three caps; the blocked / per-head / slab-wise forms of the
float64 references agree with their whole forms.  The score matrices are built by hand, so that every gap is known exactly:
per query a shuffled ladder with steps of 1e-3 (100 bars and more), into which a test plants the one gap it is about."""
import pytest
import torch

import _attention_refs as A
import _retrieval_refs as R
import _vlad_refs as V

NQ, NDB, K, DIM = 8, 50, 5, 32
CAPS = [None, "gaps", 2 / (NQ * K)]                        # the fraction: one swapped pair (two entries) of the 40
METRICS = ["ip", "l2"]


def _ladder(metric, ndb=NDB):
    """[NQ, ndb] float64 scores (larger = better; L2: minus a squared distance): 0.9, 0.899, ... in another order per query"""
    g = torch.Generator().manual_seed(ndb)
    top = 0.9 if metric == "ip" else -0.1
    return torch.stack([(top - 1e-3 * torch.arange(ndb, dtype=torch.float64))[torch.randperm(ndb, generator=g)] for _ in range(NQ)])


def _lists(s, k, metric):
    """the exact lists of ``s`` as a search returns them: fp32 distances, int64 indices, -1 beyond the database"""
    o = torch.sort(s, dim=1, descending=True, stable=True)
    kk = min(k, s.shape[1])
    d = torch.full((s.shape[0], k), float("inf"))
    i = torch.full((s.shape[0], k), -1, dtype=torch.int64)
    d[:, :kk] = (-o.values[:, :kk] if metric == "l2" else o.values[:, :kk]).float()
    i[:, :kk] = o.indices[:, :kk]
    return d, i


def _swap(d, i, q, a=0, b=1):
    """ranks a and b of query q change places, distances with them (each still the score of ITS row)"""
    for t in (d, i):
        t[q, [a, b]] = t[q, [b, a]]


def _close_pair(s, q, gap):
    """the second-best row of query q scores ``gap`` below the best"""
    best, second = torch.sort(s[q], descending=True, stable=True).indices[:2]
    s[q, second] = s[q, best] - gap


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("metric", METRICS)
def test_exact_lists_pass_with_no_differing_entry(metric, cap):
    s = _ladder(metric)
    d, i = _lists(s, K, metric)
    assert R.check_lists(d, i, s, K, metric, "exact", cap=cap) == 0
    s = _ladder(metric, ndb=3)                              # fewer rows than k: two slots of padding
    d, i = _lists(s, K, metric)
    assert R.check_lists(d, i, s, K, metric, "exact, k > ndb", cap=cap) == 0


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("metric", METRICS)
def test_a_wrong_distance_fails(metric, cap):
    s = _ladder(metric)
    d, i = _lists(s, K, metric)
    d[2, 1] += 2 * R.BAR[metric]
    with pytest.raises(AssertionError):
        R.check_lists(d, i, s, K, metric, "distance off by two bars", cap=cap)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("metric", METRICS)
def test_swapped_entries_ten_bars_apart_fail(metric, cap):
    s = _ladder(metric)
    _close_pair(s, 3, 10 * R.BAR[metric])
    d, i = _lists(s, K, metric)
    assert R.check_lists(d, i, s, K, metric, "before the swap", cap=cap) == 0
    _swap(d, i, 3)
    with pytest.raises(AssertionError):
        R.check_lists(d, i, s, K, metric, "swapped, ten bars apart", cap=cap)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("metric", METRICS)
def test_padding_that_is_not_minus_one_fails(metric, cap):
    s = _ladder(metric)
    d, i = _lists(s, NDB + 10, metric)
    assert R.check_lists(d, i, s, NDB + 10, metric, "k > ndb", cap=cap) == 0
    i[0, NDB + 5] = 0
    with pytest.raises(AssertionError):
        R.check_lists(d, i, s, NDB + 10, metric, "a padding slot holds 0", cap=cap)


@pytest.mark.parametrize("bad", [-1, NDB])
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("metric", METRICS)
def test_an_index_outside_the_database_fails(metric, cap, bad):
    s = _ladder(metric)
    d, i = _lists(s, K, metric)
    i[4, 2] = bad
    with pytest.raises(AssertionError):
        R.check_lists(d, i, s, K, metric, f"index {bad} in front of the padding", cap=cap)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("metric", METRICS)
def test_a_swapped_exact_tie_passes_under_every_cap(metric, cap):
    s = _ladder(metric)
    _close_pair(s, 5, 0.0)                                  # a duplicated row
    d, i = _lists(s, K, metric)
    assert i[5, 0] < i[5, 1]                                # ties -> lower index first
    _swap(d, i, 5)
    assert R.check_lists(d, i, s, K, metric, "swapped duplicate", cap=cap) == 2


@pytest.mark.parametrize("metric", METRICS)
def test_a_swap_between_gap_and_bar_passes_uncapped_and_fails_the_gaps_cap(metric):
    gap = {"ip": 1e-6, "l2": 3e-6}[metric]
    assert R.GAP[metric] <= gap < R.BAR[metric]
    s = _ladder(metric)
    _close_pair(s, 1, gap)
    d, i = _lists(s, K, metric)
    _swap(d, i, 1)
    assert R.check_lists(d, i, s, K, metric, "swapped near-tie", cap=None) == 2
    with pytest.raises(AssertionError):                     # no gap of the top-(k + 1) lists is below GAP: that cap is 0
        R.check_lists(d, i, s, K, metric, "swapped near-tie", cap="gaps")


@pytest.mark.parametrize("metric", METRICS)
def test_the_fraction_cap_counts_entries(metric):
    s = _ladder(metric)
    _close_pair(s, 1, 0.0)
    _close_pair(s, 6, 0.0)
    d, i = _lists(s, K, metric)
    _swap(d, i, 1)
    assert R.check_lists(d, i, s, K, metric, "one swap of 40 entries", cap=2 / 40) == 2
    _swap(d, i, 6)
    assert R.check_lists(d, i, s, K, metric, "two swaps, uncapped", cap=None) == 4
    with pytest.raises(AssertionError):
        R.check_lists(d, i, s, K, metric, "two swaps of 40 entries", cap=2 / 40)


@pytest.mark.parametrize("defect", ["distance", "swap"])
@pytest.mark.parametrize("metric", METRICS)
def test_scale_widens_the_bar(metric, defect):
    """The defects above under scale = 7.5: planted at 7 bars, not at 7.5, so that neither fp32 rounding of the distance nor the
    last bit of 7.5 * BAR decides the outcome: inside the bar of scale = 7.5, outside that of scale = 1."""
    s = _ladder(metric)
    _close_pair(s, 3, 7 * R.BAR[metric])
    d, i = _lists(s, K, metric)
    if defect == "distance":
        d[2, 1] += 7 * R.BAR[metric]
    else:
        _swap(d, i, 3)
    assert R.check_lists(d, i, s, K, metric, f"{defect} at 7 bars, scale 7.5", scale=7.5) == (0 if defect == "distance" else 2)
    with pytest.raises(AssertionError):
        R.check_lists(d, i, s, K, metric, f"{defect} at 7 bars, scale 1")


@pytest.mark.parametrize("metric", METRICS)
def test_scale_widens_the_gap_of_the_gaps_cap(metric):
    """a swapped pair 5 GAP apart (half a bar): a near-tie that cap="gaps" counts under scale = 7.5 and does not under scale = 1"""
    s = _ladder(metric)
    _close_pair(s, 3, 5 * R.GAP[metric])
    d, i = _lists(s, K, metric)
    _swap(d, i, 3)
    assert R.check_lists(d, i, s, K, metric, "swap at 5 GAP, scale 7.5", scale=7.5, cap="gaps") == 2
    assert R.check_lists(d, i, s, K, metric, "swap at 5 GAP, scale 1, uncapped", cap=None) == 2
    with pytest.raises(AssertionError):
        R.check_lists(d, i, s, K, metric, "swap at 5 GAP, scale 1", cap="gaps")


@pytest.mark.parametrize("metric", METRICS)
def test_check_search_on_planted_rows(metric):
    """the wrapper that scores for itself, on the CPU draw of the planted-neighbour recipe"""
    qu, db = R.planted_rows(NQ, 70, DIM, 1, device="cpu")
    assert qu.shape == (NQ, DIM) and db.shape == (70, DIM) and qu.device.type == "cpu"
    d, i = _lists(R.exact_scores64(qu, db, metric), K, metric)
    assert R.check_search(d, i, qu, db, K, metric, "planted rows") == 0
    d[0, 0] += 2 * R.BAR[metric]
    with pytest.raises(AssertionError):
        R.check_search(d, i, qu, db, K, metric, "planted rows, one distance off")


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("metric", METRICS)
def test_exact_scores_in_blocks_are_the_whole_matrix(metric, normalize):
    qu, db = R.planted_rows(NQ, NDB, DIM, 2, planted=False, device="cpu")
    whole = R.exact_scores64(qu, db, metric, normalize)
    blocked = R.exact_scores64(qu, db, metric, normalize, block=16)           # 16 + 16 + 16 + 2 rows
    assert whole.shape == blocked.shape == (NQ, NDB) and whole.dtype == torch.float64
    assert float((whole - blocked).abs().max()) <= 1e-13
    want = qu.double() @ (torch.nn.functional.normalize(db.double()) if normalize else db.double()).t()
    if metric == "ip":
        assert float((whole - want).abs().max()) <= 1e-13


def test_attention_per_head_is_the_vectorised_form():
    B, T, heads = 2, 33, 2
    qkv = A.spiky_qkv(B, T, heads, 4)
    out, smax = A.attention_f64(qkv, heads, want_smax=True)
    out_h, smax_h = A.attention_f64(qkv, heads, per_head=True, want_smax=True)
    assert out.shape == out_h.shape == (B, T, heads * 64) and out.dtype == torch.float64
    assert float((out - out_h).abs().max()) <= 1e-12
    q, k, _ = qkv.double().reshape(B, T, 3, heads, 64).unbind(2)
    logits = torch.einsum("bqhc,bkhc->bhqk", q, k) / 8.0
    assert torch.allclose(smax, logits.abs().amax(dim=(1, 3)), rtol=1e-12, atol=0) and torch.allclose(smax_h, smax, rtol=1e-12, atol=0)
    one = A.spiky_qkv_image(T, heads, 5)                    # a [T, 3 D] input is one image
    assert float((A.attention_f64(one, heads) - A.attention_f64(one[None], heads, per_head=True)[0]).abs().max()) <= 1e-12


@pytest.mark.parametrize("norm_descs,intra_norm", [(True, True), (False, True), (True, False)])
def test_hard_vlad_in_slabs_is_the_whole_image(norm_descs, intra_norm):
    N, K_, D = 40, 3, 16
    g = torch.Generator().manual_seed(6)
    x, c = torch.randn(N, D, generator=g), torch.randn(K_, D, generator=g)
    labels = torch.randint(0, K_, (N,), generator=g)
    whole = V.hard_vlad_f64(x, c, labels, norm_descs, intra_norm)
    slabs = V.hard_vlad_f64(x, c, labels, norm_descs, intra_norm, slab=7)    # five slabs of 7 and one of 5
    assert whole.shape == (K_ * D,) and whole.dtype == torch.float64 and abs(float(whole.norm()) - 1.0) <= 1e-12
    assert float((whole - slabs).abs().max()) <= 1e-13
    assert V.l2rel(whole.float(), whole) < 1e-7 and V.l2rel(2.0 * whole, whole) == pytest.approx(1.0)
