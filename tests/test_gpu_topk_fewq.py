"""Few-query top-k (``pytest -m gpu``; <= 64 queries, option topk_fewq_x6): the database rows split on the fly into three bf16
planes (1, csrc/scores_x6.hip) or into two fp16 planes under a power-of-two scale that runs along each row (2,
csrc/scores_h3.hip), against the flat-index restatement of the oracle and a float64 search on the device."""
import pytest
import torch

from _retrieval_refs import check_topk

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("metric,norm", [("ip", True), ("ip", False), ("l2", True), ("l2", False)])
def test_topk_few_queries_on_the_fly_bf16_split(metric, norm):
    """Option topk_fewq_x6 = 1: <= 64 queries, the database rows split on the fly into three bf16 planes (six bf16 MFMA
    products, csrc/scores_x6.hip) -- ragged row tail (10 000 + 37 rows = 79 tiles, the last one 5 rows), 61 and 3 queries
    (zero-padded query columns), K slices, row norms from the same pass, vs the flat-index restatement and float64."""
    from anyloc_amd import ops
    g = torch.Generator().manual_seed(11)
    dim, ndb = 8192, 10037
    scale = 0.05 + torch.rand(ndb, 1, generator=g) * 20.0
    scale[12] = 25.0                                                # the planted top hit also wins the raw inner product
    db = torch.randn(ndb, dim, generator=g) * scale
    db[5000] = db[12]
    for nq, k in ((61, 20), (3, 7)):
        qu = torch.randn(nq, dim, generator=g)
        pick = torch.arange(min(nq, 30)) * 301 + 12
        qu[: len(pick)] = db[pick] + 0.3 * scale[pick] * torch.randn(len(pick), dim, generator=g)
        qd = (torch.nn.functional.normalize(qu) if norm else qu).to("cuda")
        with ops.options(topk_fewq_x6=1):
            d, i = ops.topk(qd, db.to("cuda"), k, metric, normalize_db=norm)
            d1, i1 = ops.topk(qd, db.to("cuda"), k, metric, normalize_db=norm)
        assert torch.equal(i, i1) and torch.equal(d, d1)
        check_topk(d, i, qu, db, k, metric, norm)
        assert int(i[0, 0]) == 12 and int(i[0, 1]) == 5000          # the duplicated row: lower index first
        with ops.options(topk_fewq_x6=0):
            d0, i0 = ops.topk(qd, db.to("cuda"), k, metric, normalize_db=norm)
        assert float((i0 != i).float().mean()) < 0.003


def _check_vs_float64(d, i, qu, db, k, metric, norm, tol=3e-6):
    """(dist, idx) of ops.topk against the exact float64 search on the device: tie-aware index identity, distance error."""
    q64, d64 = qu.double(), db.double()
    if norm:
        q64, d64 = torch.nn.functional.normalize(q64, dim=1), torch.nn.functional.normalize(d64, dim=1)
    if metric == "ip":
        sc = q64 @ d64.T
        order = torch.sort(-sc, dim=1, stable=True)[1][:, :k]
    else:
        sc = (q64 * q64).sum(1)[:, None] + (d64 * d64).sum(1)[None] - 2 * q64 @ d64.T
        order = torch.sort(sc, dim=1, stable=True)[1][:, :k]
    got, want = torch.gather(sc, 1, i), torch.gather(sc, 1, order)
    scale = float(sc.abs().max()) if not norm else 1.0
    assert int(((i != order) & ((got - want).abs() > tol * scale)).sum()) == 0
    assert float((d.double() - got).abs().max()) <= tol * scale, float((d.double() - got).abs().max())


@pytest.mark.parametrize("metric,norm", [("ip", True), ("ip", False), ("l2", True), ("l2", False)])
def test_topk_few_queries_two_fp16_planes_running_scale(metric, norm):
    """Option topk_fewq_x6 = 2 (csrc/scores_h3.hip): <= 64 queries, database rows split on the fly into two fp16 planes under a
    power-of-two scale that RUNS along each row -- ragged row tail, 61 and 3 queries, row norms from the same pass; rows
    whose magnitude grows along K (a new maximum, i.e. a rescale of the accumulators, in most slabs), rows with one late
    spike, all-zero and tiny rows.  Against float64, and reproducible run to run."""
    from anyloc_amd import ops
    g = torch.Generator(device=DEV)
    g.manual_seed(21)
    dim, ndb = 8192, 10037
    scale = 0.05 + torch.rand(ndb, 1, generator=g, device=DEV) * 20.0
    db = torch.randn(ndb, dim, generator=g, device=DEV) * scale
    ramp = torch.exp2(torch.arange(dim, device=DEV) / dim * 12.0)              # magnitudes grow 4096 x along the row
    db[100:164] *= ramp
    db[200:232, 7000] = 5e3                                                     # one late spike
    db[300:310] = 0.0
    db[320:330] *= 1e-30
    db[5000] = db[12]
    for nq, k in ((61, 20), (3, 7)):
        qu = torch.randn(nq, dim, generator=g, device=DEV)
        pick = torch.arange(min(nq, 30), device=DEV) * 301 + 12
        qu[: len(pick)] = db[pick] + 0.3 * scale[pick] * torch.randn(len(pick), dim, generator=g, device=DEV)
        qu[-1] = db[130]                                                        # a ramp row as the query
        qd = torch.nn.functional.normalize(qu) if norm else qu
        with ops.options(topk_fewq_x6=2):
            d, i = ops.topk(qd, db, k, metric, normalize_db=norm)
            d1, i1 = ops.topk(qd, db, k, metric, normalize_db=norm)
        assert torch.equal(i, i1) and torch.equal(d, d1)
        with ops.options(topk_fewq_x6=2, topk_fewq_qdma=0):                     # queries split per slab by the staging lanes: the same bits
            d2, i2 = ops.topk(qd, db, k, metric, normalize_db=norm)
        assert torch.equal(i, i2) and torch.equal(d, d2)
        _check_vs_float64(d, i, qu, db, k, metric, norm)
        if norm or metric == "l2":                                              # (the raw inner product prefers the huge ramp rows)
            assert int(i[0, 0]) == 12 and int(i[0, 1]) == 5000                  # the duplicated row: lower index first
        with ops.options(topk_fewq_x6=1):
            d0, i0 = ops.topk(qd, db, k, metric, normalize_db=norm)
        assert float((i0 != i).float().mean()) < 0.003


def test_topk_few_queries_running_scale_self_match_long_rows():
    """131 072 columns (the ViT-L two-tap VLAD), queries that ARE database rows, all-positive rows: every product is a
    square, whatever is dropped adds up.  Cosine 1 to 2e-6 and the exact top-5."""
    from anyloc_amd import ops
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    dim, ndb, nq = 131072, 260, 8
    db = torch.nn.functional.normalize(torch.randn(ndb, dim, generator=g, device=DEV).abs() + 0.5, dim=1) * 2.5
    qu = db[:nq].clone()
    with ops.options(topk_fewq_x6=2):
        d, i = ops.topk(torch.nn.functional.normalize(qu), db, 5, "ip", normalize_db=True)
    assert torch.equal(i[:, 0].cpu(), torch.arange(nq))
    _check_vs_float64(d, i, qu, db, 5, "ip", True, tol=2e-6)
