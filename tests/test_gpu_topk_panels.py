"""Many-query top-k on the two-term fp16 score panels (``pytest -m gpu``; option topk_h3, csrc/gemm_h3m.hip for >= 2048 queries,
``anyloc_split_h2`` on retrieval-wide rows) and the prepared flat index on them (``anyloc_topk_index_build`` /
``anyloc_topk_search_index``, ``retrieval.FlatIndex``): against the flat-index restatement of the oracle with per-query tie
proofs, against an exact float64 search at the full BASELINE.json configs[1] size and on one configs[2] panel, and bit for bit
against the one-shot search."""
import pytest
import torch

from _retrieval_refs import check_topk, spread_rows, vlad_like_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------- against the flat-index restatement, per-query tie proofs
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("norm", [False, True])
def test_topk_fp16_score_panels_vs_oracle(metric, norm):
    """Option topk_h3 = 1: the many-query score panels on gemm_h3 (22-bit row-scaled operands, fp32 accumulate) -- uneven
    panel tail (8192 + 1808 rows), a tie across panels, rows of very different magnitude, k above one panel's merge step."""
    from anyloc_amd import ops
    g = torch.Generator().manual_seed(3)
    dim, ndb, nq, k = 2048, 10000, 150, 25
    db = torch.randn(ndb, dim, generator=g) * (0.05 + torch.rand(ndb, 1, generator=g) * 20.0)
    qu = torch.randn(nq, dim, generator=g)
    qu[:40] = db[torch.arange(40) * 211 + 7] + 0.3 * torch.randn(40, dim, generator=g)
    db[9000] = db[12]                                              # identical rows in two panels: lower index first
    with ops.options(topk_h3=1):
        d, i = ops.topk(torch.nn.functional.normalize(qu).to("cuda") if norm else qu.to("cuda"), db.to("cuda"), k, metric,
                        normalize_db=norm)
        d1, i1 = ops.topk(torch.nn.functional.normalize(qu).to("cuda") if norm else qu.to("cuda"), db.to("cuda"), k, metric,
                          normalize_db=norm)
    assert torch.equal(i, i1) and torch.equal(d, d1)               # run-to-run reproducible
    check_topk(d, i, qu, db, k, metric, norm)
    hit = (i.cpu() == 12).nonzero()
    for n, j in hit.tolist():                                      # the duplicated row: index 12 directly before 9000
        if j + 1 < k:
            assert int(i[n, j + 1]) == 9000 and float(d[n, j]) == float(d[n, j + 1])
    # ... and the same lists as the fp32-MFMA panels give (identical except proven near-ties, checked against float64 above)
    with ops.options(topk_h3=0):
        d0, i0 = ops.topk(torch.nn.functional.normalize(qu).to("cuda") if norm else qu.to("cuda"), db.to("cuda"), k, metric,
                          normalize_db=norm)
    assert float((i0 != i).float().mean()) < 0.002


def test_topk_fp16_score_panels_vlad_width():
    """The config-3 row width (49 152) at a size the CPU can score: 300 queries x 3000 unit-block VLADs, cosine with the
    database normalised inside the search."""
    from anyloc_amd import ops
    g = torch.Generator().manual_seed(9)
    K, D = 32, 1536
    db = torch.nn.functional.normalize(torch.randn(3000, K, D, generator=g), dim=-1).reshape(3000, K * D) * 3.0
    qu = torch.nn.functional.normalize(torch.randn(300, K, D, generator=g), dim=-1).reshape(300, K * D)
    qu[:50] = 0.8 * db[torch.arange(50) * 37 + 3] / 3.0 + 0.2 * qu[:50]
    with ops.options(topk_h3=1):
        d, i = ops.topk(torch.nn.functional.normalize(qu).to("cuda"), db.to("cuda"), 20, "ip", normalize_db=True)
    assert torch.equal(i[:50, 0].cpu(), torch.arange(50) * 37 + 3)
    check_topk(d, i, qu, db, 20, "ip", True)


def test_topk_fp16_score_panels_on_the_16x16x32_kernel():
    """>= 2048 queries against a full 8192-row panel of >= 4096 columns: the panel GEMM is gemm_h3m_kernel (256 x 256 tiles,
    v_mfma_f32_16x16x32_f16), first K chunk plain, second chunk accumulating (here on gemm_h3_kernel: 512 columns), the
    600-row tail panel on gemm_h3_kernel -- checked like every other panel path, and against the lists gemm_h3_kernel gives."""
    from anyloc_amd import ops
    g = torch.Generator().manual_seed(11)
    dim, ndb, nq, k = 8192 + 512, 8192 + 600, 2100, 20
    db = torch.randn(ndb, dim, generator=g) * (0.05 + torch.rand(ndb, 1, generator=g) * 20.0)
    qu = torch.randn(nq, dim, generator=g)
    qu[:64] = db[torch.arange(64) * 131 + 5] + 0.3 * torch.randn(64, dim, generator=g)
    qu[-64:] = db[torch.arange(64) * 7 + 8200 - 448] + 0.3 * torch.randn(64, dim, generator=g)   # (rows of both panels)
    qg, dg = torch.nn.functional.normalize(qu).to("cuda"), db.to("cuda")
    d, i = ops.topk(qg, dg, k, "ip", normalize_db=True)
    with ops.options(h3_mfma16=0):
        d0, i0 = ops.topk(qg, dg, k, "ip", normalize_db=True)
    assert float((i0 != i).float().mean()) < 0.002 and float((d0 - d).abs().max()) <= 3e-6
    sel = torch.cat([torch.arange(0, 128), torch.arange(nq - 128, nq)])
    check_topk(d[sel.to("cuda")], i[sel.to("cuda")], qu[sel], db, k, "ip", True)


@pytest.mark.parametrize("nq", [8, 200])
def test_topk_self_match_keeps_the_small_products(nq):
    """A query that IS a database row (cosine 1): every term of the contraction is a square, so products that are dropped or
    absorbed add up instead of averaging out -- the few-query bf16 split keeps its 2^-16-sized plane products in their own
    accumulator, the fp16 panels cut K into chunks.  131 072 columns (the ViT-L two-tap VLAD), vs float64."""
    from anyloc_amd import ops
    g = torch.Generator().manual_seed(5)
    dim, ndb = 131072, 260
    db = torch.nn.functional.normalize(torch.randn(ndb, dim, generator=g).abs() + 0.5, dim=1) * 2.5     # all-positive rows
    qu = db[:nq].clone()
    with ops.options(topk_h3=1):
        d, i = ops.topk(torch.nn.functional.normalize(qu).to("cuda"), db.to("cuda"), 5, "ip", normalize_db=True)
    assert torch.equal(i[:, 0].cpu(), torch.arange(nq))
    check_topk(d, i, qu, db, 5, "ip", True)
    q64 = torch.nn.functional.normalize(qu.double())
    d64 = torch.nn.functional.normalize(db.double())
    exact = (q64 @ d64.t()).topk(5, dim=1)[0]
    assert float((d.cpu().double() - exact).abs().max()) <= 2e-6


def test_split_h2_wide_rows():
    """anyloc_split_h2 above 4096 columns (retrieval rows): 22 bits relative to the row maximum, rows of any magnitude,
    a zero row, a ragged last row group."""
    from anyloc_amd import ops
    g = torch.Generator().manual_seed(1)
    rows, K = 37, 49152
    x = torch.randn(rows, K, generator=g) * torch.pow(10.0, torch.randint(-6, 6, (rows, 1), generator=g).float())
    x[5] = 0.0
    x[7, 100] = 3e4 * float(x[7].abs().max())                      # one element 3e4 above the rest of its row
    img, inv = ops.split_h2(x.to("cuda"))
    back = ops.h2_image_to_f32(img, inv, rows, K).cpu()
    amax = x.double().abs().max(dim=1, keepdim=True)[0]
    err = (back - x.double()).abs() / amax.clamp_min(1e-300)
    assert float(err[torch.arange(rows) != 5].max()) <= 2.0 ** -21 and float(back[5].abs().max()) == 0.0
    # the scale puts the row maximum in [2^14, 2^15)
    top = amax.squeeze(1) / inv.cpu().double()
    ok = (top >= 2.0 ** 14) & (top < 2.0 ** 15)
    assert bool(ok[torch.arange(rows) != 5].all())


# ---------------------------------------------------------------------------- index identity against a float64 search
def _float64_flat(qu, db, k, chunk=128):
    """Exact flat inner-product search of the L2-normalised operands in float64 on the device (the checker): indices with
    faiss' tie rule (lower index first) and the float64 score matrix chunks for tie-aware comparison."""
    dbn = torch.nn.functional.normalize(db.double(), dim=1)
    for s0 in range(0, qu.shape[0], chunk):
        sc = torch.nn.functional.normalize(qu[s0:s0 + chunk].double(), dim=1) @ dbn.T
        yield s0, sc, torch.sort(-sc, dim=1, stable=True)[1][:, :k]


def _assert_identity(qu, db, dist, idx, k, tol=3e-6):
    mism = swaps = 0
    for s0, sc, order in _float64_flat(qu, db, k):
        ours = idx[s0:s0 + order.shape[0]]
        got, want = torch.gather(sc, 1, ours), torch.gather(sc, 1, order)
        diff = ours != order
        near = (got - want).abs() <= tol
        swaps += int((diff & near).sum())
        mism += int((diff & ~near).sum())
        assert float((dist[s0:s0 + order.shape[0]].double() - got).abs().max()) <= tol
        # a swap only ever exchanges near-tied neighbours: as SETS the lists differ at most at the k-th rank
    assert mism == 0, f"{mism} indices differ from the float64 search outside {tol} ties ({swaps} near-tie swaps)"
    return swaps


def test_topk_index_identity_at_the_full_config2_size():
    """1 000 queries x 10 000 rows x 49 152 columns (BASELINE.json configs[1], the reference's utilities.py:433-450 at its
    headline size): every index of the top-20 equals the exact float64 flat search (ties -> lower index), distances within
    3e-6, and a 48-query slice equals the faiss restatement of the oracle on the CPU."""
    from anyloc_amd import retrieval
    from oracle import faiss_flat
    db = vlad_like_rows(10000, 32, 1536, 1)
    qu = vlad_like_rows(1000, 32, 1536, 2)
    src = torch.arange(1000, device=DEV) * 7 + 3
    qu[:600] = 0.6 * db[src[:600]] + 0.4 * qu[:600]              # neighbours at every similarity level
    qu[600:700] = db[src[600:700]]                               # exact copies (cosine 1)
    qu[700:720] = 0.5 * (db[src[700:720]] + db[src[700:720] + 1])  # two near-equal neighbours
    db[9000:9010] = db[8000:8010]                                # duplicated rows: exact ties, the lower index first
    for lo, hi in ((0, 1000), (0, 61), (100, 356)):             # many-query panels, the few-query kernel, a mid-size call
        d, i = retrieval.search(db, qu[lo:hi], 20)
        swaps = _assert_identity(qu[lo:hi], db, d, i, 20)
        assert swaps <= (hi - lo) // 10
    d, i = retrieval.search(db, qu[640:688], 20)
    dr, ir = faiss_flat.flat_search(torch.nn.functional.normalize(qu[640:688].cpu()), torch.nn.functional.normalize(db.cpu()), 20)
    assert torch.equal(i[:, 0].cpu(), ir[:, 0])
    assert float((d.cpu() - dr).abs().max()) <= 3e-6
    both = (i.cpu() == ir)
    assert float(both.float().mean()) > 0.98                     # fp32 CPU search vs fp32-accurate GPU search: near-ties may swap


def test_topk_index_identity_on_a_config3_panel():
    """2 048 queries against one 8 192-row panel of 49 152 columns (the unit of work of the many-query path at configs[2]:
    two-term fp16 score panels on the 16x16x32 MFMA kernel, K-chunked accumulation): identical to the float64 search."""
    from anyloc_amd import retrieval
    db = vlad_like_rows(8192, 32, 1536, 3)
    qu = vlad_like_rows(2048, 32, 1536, 4)
    src = torch.arange(1024, device=DEV) * 5 + 1
    qu[:1024] = 0.7 * db[src] + 0.3 * qu[:1024]
    d, i = retrieval.search(db, qu, 20)
    assert torch.equal(i[:1024, 0], src)
    _assert_identity(qu, db, d, i, 20)


# ------------------------------------------------------------------------------------------- the prepared flat index
@pytest.mark.parametrize("ndb,dim,nq,k", [(9001, 1024, 70, 20), (8192, 512, 300, 5), (20000, 256, 129, 33), (300, 2048, 65, 400)])
def test_prepared_index_gives_the_lists_of_the_one_shot_search(ndb, dim, nq, k):
    """``anyloc_topk_search_index`` reads the panels ``anyloc_topk_index_build`` left instead of quantising the database per
    call: the same score kernels on the same operand images, so distances and indices are those of ``anyloc_topk`` on its fp16
    panels BIT FOR BIT -- both metrics, normalising or not, a ragged last panel, k beyond the database (-1 padding), an index
    base -- and identical to a float64 flat search."""
    from anyloc_amd import ops
    db, qu = spread_rows(ndb, dim, 1).to(DEV), spread_rows(nq, dim, 2).to(DEV)
    db[7] = db[ndb - 3]                                                # a tie across panels: lower index first
    index = ops.topk_index_build(db)
    assert index.numel() == ops.topk_index_bytes(ndb, dim) > 0
    for metric in ("ip", "l2"):
        for norm in (False, True):
            q = ops.l2norm_rows(qu) if norm else qu
            with ops.options(topk_h3=1):                               # the one-shot search on the same (fp16 panel) path
                d0, i0 = ops.topk(q, db, k, metric, index_base=11, normalize_db=norm)
            d1, i1 = ops.topk_indexed(q, index, ndb, k, metric, index_base=11, normalize_db=norm)
            assert torch.equal(i0, i1), (metric, norm)
            assert torch.equal(d0, d1), (metric, norm)
            # against float64
            dbn = torch.nn.functional.normalize(db.double(), dim=1) if norm else db.double()
            s = q.double() @ dbn.t()
            if metric == "l2":
                s = -((q.double() ** 2).sum(1, keepdim=True) + (dbn ** 2).sum(1)[None] - 2 * s)
            kk = min(k, ndb)
            ref = torch.sort(s, dim=1, descending=True, stable=True)
            got_i = (i1[:, :kk] - 11)
            same = got_i == ref.indices[:, :kk]
            # a differing index is a near-tie of the float64 scores
            alt = torch.gather(s, 1, got_i.clamp_min(0))
            assert bool((same | ((alt - ref.values[:, :kk]).abs() <= 3e-6 * ref.values[:, :kk].abs().clamp_min(1.0))).all()), (metric, norm)
            if k > ndb:
                assert bool((i1[:, ndb:] == -1).all())


def test_flat_index_object_serves_few_and_many_queries_and_drops_the_rows():
    """``retrieval.FlatIndex``: built once, searched several times -- few queries stream the fp32 rows (anyloc_topk's few-query
    path), many read the prepared planes; ``keep_fp32=False`` serves both from the planes.  All agree with ``retrieval.search``."""
    from anyloc_amd import retrieval
    dim = 4096
    db, qu = spread_rows(3000, dim, 3).to(DEV), spread_rows(300, dim, 4).to(DEV)
    for method in ("cosine", "l2"):
        ix = retrieval.FlatIndex(db, method, planes=True)
        assert ix.has_planes and ix.ntotal == 3000
        for n in (9, 200, 300):                                      # few-query stream / fp32-MFMA panels / fp16 panels (prepared)
            d0, i0 = retrieval.search(db, qu[:n], 10, method)
            d1, i1 = ix.search(qu[:n], 10)
            assert torch.equal(i0, i1) and torch.equal(d0, d1), (method, n)
            d2, i2 = retrieval.search(ix, qu[:n], 10, method)
            assert torch.equal(i1, i2) and torch.equal(d1, d2)
        lean = retrieval.FlatIndex(db, method, planes=True, keep_fp32=False)
        assert lean.db is None
        d3, i3 = lean.search(qu[:9], 10)                             # (no fp32 rows left: the panels serve nine queries too)
        d0, i0 = retrieval.search(db, qu[:9], 10, method)
        assert float((d3 - d0).abs().max()) <= 3e-6
        assert bool(((i3 == i0) | ((d3 - d0).abs() <= 3e-6)).all())
    with pytest.raises(ValueError):
        retrieval.search(retrieval.FlatIndex(db, "cosine", planes=False), qu, 5, "l2")
    plain = retrieval.FlatIndex(db, "cosine", planes=False)
    assert not plain.has_planes and torch.equal(plain.search(qu, 5)[1], retrieval.search(db, qu, 5)[1])
