"""The screened retrieval on an index that keeps no fp32 rows (ANYLOC_TOPK_RESCORE_PLANES, retrieval.FlatIndex(rescore="planes")).

    python tools/time_screen_rowsfree.py shard [nq] [ndb] [passes]     configs[2]'s shard on one GPU: 10 000 x 125 000 x 49 152, top-20, cosine
    python tools/time_screen_rowsfree.py whole [nq] [ndb]             the whole 1 M x 49 152 database as ONE resident index built from chunks

shard: ONE FlatIndex with rows and planes, three variants interleaved, HIP events, median of `passes` (>= 5) after a warm-up:
  (a) screened, candidates re-scored from the fp32 rows (the path of an index that keeps them),
  (b) screened, candidates re-scored from the planes (the flag on the same index),
  (c) unscreened three-product panels (what an index without its rows ran before the flag existed).
Per variant the profile's time of the re-scoring tag, the device memory the index object holds with and without its rows, and 32
queries checked against a float64 search over the whole shard.  THE BAR: (b) faster than (c) by more than the spread (max - min)
of the passes of either.  whole: the index is built panel by panel from generated rows (they never exist together), 10 000 queries
with a planted neighbour each; skipped with a printed reason where the device cannot hold index + workspace."""
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from anyloc_amd import _lib, ops, retrieval  # noqa: E402

dev = "cuda"
mode = sys.argv[1] if len(sys.argv) > 1 else "shard"
dim, k = 49152, 20


def box():
    """clock and power of the device as the driver reports them (read-only query; empty where the tool is missing)"""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        return " | ".join(l.strip() for l in out.splitlines() if "sclk" in l or "mclk" in l or "Power" in l)
    except Exception as e:                                  # noqa: BLE001
        return f"(no reading: {e})"


def prof_of(fn):
    ops.profile_enable(True)
    ops.profile_reset()
    fn()
    torch.cuda.synchronize()
    p = ops.profile_dump()
    ops.profile_enable(False)
    return {kk: round(v["ms"], 2) for kk, v in sorted(p.items(), key=lambda kv: -kv[1]["ms"])}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def f64_check(d, i, qu, db_rows, sel, tag):
    """the selected queries against a float64 search over all rows (row blocks: no float64 copy of the database)"""
    ndb = i.new_tensor(0).item() + sum(n for _, n in db_rows.blocks)
    qn = qu[sel].double()
    s64 = torch.empty(len(sel), ndb, dtype=torch.float64, device=dev)
    for r0, n in db_rows.blocks:
        s64[:, r0:r0 + n] = qn @ torch.nn.functional.normalize(db_rows(r0, n).double()).t()
    o = torch.sort(s64, dim=1, descending=True, stable=True)
    got = torch.gather(s64, 1, i[sel])
    mism = i[sel] != o.indices[:, :k]
    worst = float((got[mism] - o.values[:, :k][mism]).abs().max()) if bool(mism.any()) else 0.0
    err = float((d[sel].double() - got).abs().max())
    ok = worst <= 3e-6 and err <= 3e-6
    print(f"  float64 check {tag}: {len(sel)} queries, {int(mism.sum())} index mismatches (largest float64 score difference {worst:.2e}), "
          f"max |distance error| {err:.2e} -> {'ok' if ok else 'FAILED'}", flush=True)
    return ok


class Rows:
    """rows [r0, r0 + n) of the database: a resident tensor, or a generator of panels"""

    def __init__(self, get, ndb, step=8192):
        self.get, self.blocks = get, [(r0, min(step, ndb - r0)) for r0 in range(0, ndb, step)]

    def __call__(self, r0, n):
        return self.get(r0, n)


def shard():
    nq = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    ndb = int(sys.argv[3]) if len(sys.argv) > 3 else 125000
    passes = max(5, int(sys.argv[4])) if len(sys.argv) > 4 else 5
    g = torch.Generator(device=dev).manual_seed(0)
    db = torch.empty(ndb, dim, device=dev)
    for r0 in range(0, ndb, 8192):
        db[r0:r0 + 8192] = torch.randn(min(8192, ndb - r0), dim, generator=g, device=dev)
    qu = torch.nn.functional.normalize(torch.randn(nq, dim, generator=g, device=dev))
    rows = torch.randperm(ndb, generator=g, device=dev)[:nq] if nq <= ndb else torch.randint(0, ndb, (nq,), generator=g, device=dev)
    db[rows] = qu * 3.0 + 0.3 * torch.randn(nq, dim, generator=g, device=dev)      # a planted neighbour per query
    print(f"shard: {nq} queries x {ndb} rows x {dim}, top-{k}, cosine; {passes} passes per variant, interleaved; box: {box()}", flush=True)
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    index = retrieval.FlatIndex(db, "cosine", True, planes=True)
    mem_both = torch.cuda.memory_allocated() - m0 + db.numel() * 4
    mem_planes = index.planes.numel()
    print(f"index object: {mem_both / 1e9:.2f} GB with its rows (rows {db.numel() * 4 / 1e9:.2f} + planes {mem_planes / 1e9:.2f}), "
          f"{mem_planes / 1e9:.2f} GB without (keep_fp32=False, rescore=\"planes\": {mem_planes / db.numel():.3f} bytes per element)", flush=True)
    q = ops.l2norm_rows(qu)
    variants = {
        "a screened, re-scored from the rows": (1, lambda: ops.topk_indexed(q, index.planes, ndb, k, "ip", normalize_db=True, db=db)),
        "b screened, re-scored from the planes": (1, lambda: ops.topk_indexed(q, index.planes, ndb, k, "ip", normalize_db=True, rescore_planes=True)),
        "c unscreened three-product panels": (0, lambda: ops.topk_indexed(q, index.planes, ndb, k, "ip", normalize_db=True)),
    }
    times, outs = {n: [] for n in variants}, {}
    for p in range(passes + 1):                               # pass 0: warm-up
        for name, (screen, fn) in variants.items():
            with ops.options(topk_screen=screen):
                ms, out = event_ms(fn)
            if p:
                times[name].append(ms)
            outs[name] = out
    med = {}
    for name, (screen, fn) in variants.items():
        t = times[name]
        med[name] = statistics.median(t)
        with ops.options(topk_screen=screen):
            pr = prof_of(fn)
        resc = {kk: v for kk, v in pr.items() if "rescore" in kk}
        print(f"({name}): median {med[name]:8.2f} ms  min {min(t):8.2f}  max {max(t):8.2f}  spread {max(t) - min(t):6.2f}   "
              f"= {nq / med[name] * 1e3:8.0f} queries/s; re-scoring {resc}\n    kernels {pr}", flush=True)
    a, b, c = (n for n in variants)
    spread = max(max(times[b]) - min(times[b]), max(times[c]) - min(times[c]))
    print(f"THE BAR: (c) - (b) = {med[c] - med[b]:.2f} ms against a spread of {spread:.2f} ms -> {'MET' if med[c] - med[b] > spread else 'NOT MET'}; "
          f"(b) / (a) = {med[b] / med[a]:.4f}, (c) / (b) = {med[c] / med[b]:.3f}", flush=True)
    (da, ia), (db_, ib), (dc, ic) = outs[a], outs[b], outs[c]
    print(f"(b) vs (a): {int((ia != ib).sum())} of {ia.numel()} indices differ, max |distance difference| {float((da - db_).abs().max()):.3e}; "
          f"(b) vs (c): {int((ic != ib).sum())} differ, {float((dc - db_).abs().max()):.3e}; planted neighbour first: "
          f"(a) {float((ia[:, 0] == rows).float().mean()):.4f} (b) {float((ib[:, 0] == rows).float().mean()):.4f}", flush=True)
    sel = torch.arange(0, nq, max(1, nq // 32), device=dev)[:32]
    rows_of = Rows(lambda r0, n: db[r0:r0 + n], ndb)
    ok = all([f64_check(d, i, q, rows_of, sel, n[:1]) for n, (d, i) in outs.items()])
    # the object a user builds: rows dropped
    del index
    m0 = torch.cuda.memory_allocated()
    bare = retrieval.FlatIndex(db, "cosine", True, keep_fp32=False, rescore="planes")
    with ops.options(topk_screen=1):
        dd, ii = bare.search(qu, k)
    print(f"FlatIndex(keep_fp32=False, rescore=\"planes\"): holds {(torch.cuda.memory_allocated() - m0) / 1e9:.2f} GB + workspace; "
          f"lists equal (b): {bool(torch.equal(ii, ib) and torch.equal(dd, db_))}", flush=True)
    print(f"box after: {box()}", flush=True)
    return 0 if ok else 1


def whole():
    nq = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    ndb = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
    lib = _lib.load()
    need = ops.topk_index_bytes(ndb, dim) + lib.anyloc_topk_index_workspace_bytes(nq, ndb, dim, k) + 8192 * dim * 4 * 2 + nq * dim * 4 * 3 + (4 << 30)
    free, total = torch.cuda.mem_get_info()
    print(f"whole: {nq} queries x {ndb} rows x {dim} as one resident index: needs {need / 2**30:.0f} GiB (index "
          f"{ops.topk_index_bytes(ndb, dim) / 1e9:.1f} GB), free {free / 2**30:.0f} of {total / 2**30:.0f} GiB; box: {box()}", flush=True)
    if free < need:
        print("SKIPPED: the device cannot hold index + workspace", flush=True)
        return 0
    g = torch.Generator(device=dev).manual_seed(1)
    qu = torch.nn.functional.normalize(torch.randn(nq, dim, generator=g, device=dev))
    rows = (torch.arange(nq, device=dev) * 15013 + 5) % ndb         # the planted neighbour of query j (distinct rows: 15013 is prime)
    order = torch.argsort(rows)
    rows_sorted = rows[order]

    def panel(r0, n):
        """rows [r0, r0 + n): seeded by the panel, the planted neighbours of the queries that fall into it"""
        gp = torch.Generator(device=dev).manual_seed(1000 + r0)
        x = torch.randn(n, dim, generator=gp, device=dev)
        lo, hi = torch.searchsorted(rows_sorted, torch.tensor([r0, r0 + n], device=dev)).tolist()
        if hi > lo:
            qs = order[lo:hi]
            x[rows_sorted[lo:hi] - r0] = qu[qs] * 3.0 + 0.3 * torch.randn(hi - lo, dim, generator=gp, device=dev)
        return x
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index = retrieval.FlatIndex.from_chunks((panel(r0, min(5000, ndb - r0)) for r0 in range(0, ndb, 5000)), ndb, dim)   # ragged against the panels
    torch.cuda.synchronize()
    print(f"from_chunks: {time.perf_counter() - t0:.1f} s (generation included); index {index.planes.numel() / 1e9:.1f} GB, "
          f"device memory allocated {torch.cuda.memory_allocated() / 1e9:.1f} GB", flush=True)
    with ops.options(topk_screen=1):
        index.search(qu[:256], k)                                   # warm-up of kernels and workspace on a few queries
        ts = []
        for _ in range(3):
            ms, (d, i) = event_ms(lambda: index.search(qu, k))
            ts.append(ms)
        pr = prof_of(lambda: index.search(qu, k))
    print(f"one resident index: {statistics.median(ts) / 1e3:.3f} s per retrieval (passes {[round(t, 1) for t in ts]} ms) = "
          f"{nq / statistics.median(ts) * 1e3:.0f} queries/s\n    kernels {pr}", flush=True)
    found = float((i[:, 0] == rows).float().mean())
    print(f"planted neighbour first: {found:.4f}; screened without fallback: {'topk_screen_rescore_planes' in pr and 'topk_scores_gemm' not in pr}", flush=True)
    sel = torch.arange(0, nq, max(1, nq // 8), device=dev)[:8]
    ok = f64_check(d, i, ops.l2norm_rows(qu), Rows(lambda r0, n: torch.cat([panel(c, min(5000, ndb - c))[max(r0 - c, 0):r0 + n - c]
                                                                     for c in range(r0 // 5000 * 5000, r0 + n, 5000)]), ndb), sel, "whole")
    print(f"box after: {box()}", flush=True)
    return 0 if ok and found == 1.0 else 1


if __name__ == "__main__":
    sys.exit(shard() if mode == "shard" else whole())
