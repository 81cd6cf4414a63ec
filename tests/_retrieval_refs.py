"""The float64 flat search, the list checker and the data recipes that the retrieval tests share (not a test module; the
checker is itself tested, on the CPU, by tests/test_refs_cpu.py).  Every function takes its device from its inputs or from a
``device=`` argument."""
import torch

BAR = {"ip": 3e-6, "l2": 1e-5}      # |returned distance - float64 score of the returned row|, and what counts as a float64 near-tie
GAP = {"ip": 3e-7, "l2": 1e-6}      # an adjacent gap of the float64 lists below this may cost two entries under cap="gaps"


def exact_scores64(qu, db, metric, normalize=True, block=None):
    """float64 score matrix of a flat search on the device of ``qu`` (larger = better): over F.normalize(db), or the raw rows;
    ``block``: that many database rows at a time (wide rows), None: the whole matrix at once."""
    q = qu.double()

    def scores(rows):
        d = torch.nn.functional.normalize(rows.double()) if normalize else rows.double()
        s = q @ d.t()
        if metric == "l2":
            s = -((q * q).sum(1, keepdim=True) + (d * d).sum(1)[None, :] - 2.0 * s)
        return s
    if block is None:
        return scores(db)
    out = torch.empty(qu.shape[0], db.shape[0], dtype=torch.float64, device=qu.device)
    for r0 in range(0, db.shape[0], block):
        out[:, r0:r0 + block] = scores(db[r0:r0 + block])
    return out


def check_lists(d, i, s, k, metric, tag, scale=1.0, cap=None):
    """Lists (d, i) against the float64 score matrix ``s`` (ties -> lower index): -1 padding beyond min(k, ndb), every other
    index inside [0, ndb), distances within BAR[metric] * scale of the float64 score of the returned row, a differing index
    only where the two float64 scores are closer than that bar.  How many entries may differ at all:
      cap=None      no limit;
      cap="gaps"    2 x (adjacent gaps below GAP[metric] * scale in the float64 top-(k + 1) lists): one swapped pair is two entries;
      cap=fraction  that share of the entries.
    -> the number of differing entries."""
    ndb = s.shape[1]
    kk = min(k, ndb)
    o = torch.sort(s, dim=1, descending=True, stable=True)
    assert bool((i[:, kk:] == -1).all()), tag
    assert bool(((i[:, :kk] >= 0) & (i[:, :kk] < ndb)).all()), tag
    got64 = torch.gather(s, 1, i[:, :kk])
    val = -d[:, :kk].double() if metric == "l2" else d[:, :kk].double()
    tol = BAR[metric] * scale
    err = float((val - got64).abs().max())
    mism = i[:, :kk] != o.indices[:, :kk]
    differing = int(mism.sum())
    if cap is None:
        limit = mism.numel()
    elif cap == "gaps":
        top = o.values[:, :min(k + 1, ndb)]
        limit = 2 * int((top[:, :-1] - top[:, 1:] < GAP[metric] * scale).sum())
    else:
        limit = cap * mism.numel()
    print(f"{tag}: max |distance - float64| {err:.2e} (bar {tol:.1e}); {differing} of {mism.numel()} entries differ, cap {cap}: {limit}")
    assert err <= tol, (tag, err)
    if differing:                                          # only float64 near-ties may swap
        off = (got64[mism] - o.values[:, :kk][mism]).abs()
        assert float(off.max()) <= tol, (tag, float(off.max()))
        if differing > limit:
            print(f"{tag}: float64 score differences of the differing entries: {sorted(off.tolist())[-20:]}")
    assert differing <= limit, (tag, differing, limit)
    return differing


def check_search(d, i, qu, db, k, metric, tag):
    """check_lists against the float64 search over F.normalize(db), no limit on the entries at float64 near-ties"""
    return check_lists(d, i, exact_scores64(qu, db, metric), k, metric, tag)


# ---- the other oracle: the flat-index restatement, with a tie proof per differing entry (not folded into check_lists)
def flat_oracle(qu, db, k, metric, norm):
    from oracle import faiss_flat
    q = torch.nn.functional.normalize(qu) if norm else qu
    d = torch.nn.functional.normalize(db) if norm else db
    return faiss_flat.flat_search(q, d, k, metric)


def check_topk(d_g, i_g, qu, db, k, metric, norm):
    """Indices identical to the flat-index restatement except at PROVEN near-ties (float64 scores of the two swapped
    rows closer than 2e-6), distances within 3e-6 of the float64 scores of the rows the kernel returned."""
    d_r, i_r = flat_oracle(qu, db, k, metric, norm)
    q64 = (torch.nn.functional.normalize(qu.double()) if norm else qu.double())
    d64 = (torch.nn.functional.normalize(db.double()) if norm else db.double())
    i_g, d_g = i_g.cpu(), d_g.cpu()
    for n in range(qu.shape[0]):
        rows = d64[i_g[n]]
        exact = rows @ q64[n] if metric == "ip" else ((rows - q64[n]) ** 2).sum(1)
        scale = max(1.0, float(exact.abs().max()))
        assert float((d_g[n].double() - exact).abs().max()) <= 3e-6 * scale, (n, float((d_g[n].double() - exact).abs().max()))
        bad = (i_g[n] != i_r[n]).nonzero().flatten()
        for j in bad.tolist():
            other = d64[i_r[n, j]]
            e_o = float(other @ q64[n]) if metric == "ip" else float(((other - q64[n]) ** 2).sum())
            assert abs(e_o - float(exact[j])) <= 2e-6 * scale, (n, j, e_o, float(exact[j]))


def planted_rows(nq, ndb, dim, seed, planted=True, device="cuda"):
    """-> (unit queries, rows of norm 0.3 ... 2.3), drawn with a generator of ``device``"""
    g = torch.Generator(device=device).manual_seed(seed)
    db = torch.randn(ndb, dim, generator=g, device=device) * (0.3 + 2.0 * torch.rand(ndb, 1, generator=g, device=device))
    qu = torch.nn.functional.normalize(torch.randn(nq, dim, generator=g, device=device))
    if planted and ndb >= 64:
        # every query has a handful of true neighbours at graded distances, some closer to each other than the screening bound
        for j in range(6):
            rows = torch.randint(0, ndb, (nq,), generator=g, device=device)
            noise = torch.nn.functional.normalize(torch.randn(nq, dim, generator=g, device=device))
            db[rows] = (qu + (0.02 + 0.0004 * j) * noise) * (0.5 + j)
    return qu, db


def spread_rows(n, dim, seed, spread=True):
    """CPU rows for the sharded searches: row norms over more than a decade"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, dim, generator=g)
    if spread:
        x = x * (0.25 + 4.0 * torch.rand(n, 1, generator=g))
    return x


def vlad_like_rows(n, k, d, seed, device="cuda"):
    """Rows shaped like VLADs: per-cluster unit blocks, globally normalised (bench.py's synthetic database recipe)."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    out = torch.empty(n, k * d, dtype=torch.float32, device=device)
    for s in range(0, n, 1000):
        e = min(n, s + 1000)
        blk = torch.nn.functional.normalize(torch.randn(e - s, k, d, generator=g, device=device), dim=-1) / (k ** 0.5)
        out[s:e] = blk.reshape(e - s, k * d)
    return out


def profiled(fn):
    """-> (fn(), the profile of the kernels it launched)"""
    from anyloc_amd import ops
    ops.profile_enable(True); ops.profile_reset()
    out = fn()
    torch.cuda.synchronize()
    prof = ops.profile_dump()
    ops.profile_enable(False)
    return out, prof


def _screened_without_fallback(prof):
    return "topk_screen_gemm" in prof and "topk_scores_gemm" not in prof


def _screened_then_fallback(prof):
    return "topk_screen_gemm" in prof and "topk_scores_gemm" in prof


def _rows_free(prof):
    """screened, re-scored from the planes, no fallback and no fp32 rows read"""
    return (_screened_without_fallback(prof) and "topk_screen_rescore_planes" in prof and "topk_screen_rescore" not in prof)
