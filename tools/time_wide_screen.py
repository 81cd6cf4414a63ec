"""The screened search on rows wider than 49 152 columns, on one GPU (profiles/wide_screen_timing.md is made from this output).

Default: a one-shot ``ops.topk`` of 1 000 queries x 20 000 rows x 131 072 columns (10.5 GB of rows; ``normalize_db``, k = 20),
option topk_screen = 1 against = 0 -- HIP events around the call, median of 5 after 2 warm-ups; the kernel tags and times of one
profiled call of each leg (the topk_screen = 0 leg must show the three-product ``topk_scores_gemm`` and no ``topk_screen_*``: the
code path rows of this width had before); the re-scoring kernel's share of the screened call; candidates per query, counted for
32 queries by restating the screening in float64 (leading fp16 plane of every row, the margin of screen_margin_kernel); and the
float64 check of those queries' lists.
    python tools/time_wide_screen.py [nq] [ndb] [dim]

``--two-ranges``: 300 queries x 134 400 rows x 131 072 columns (70 GB of rows; 35 panels of 3 840 rows = a column range of 34
panels and a second one of one): one screened call, its kernel tags, and 32 queries' lists against a float64 search computed in
row blocks.  Skipped, saying so, when the device has less than 110 GB free."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from anyloc_amd import ops  # noqa: E402

dev = "cuda"
two_ranges = "--two-ranges" in sys.argv
args = [int(a) for a in sys.argv[1:] if not a.startswith("--")]
nq, ndb, dim = (args + [300, 134400, 131072][len(args):]) if two_ranges else (args + [1000, 20000, 131072][len(args):])
k, BLOCK = 20, 1920
if two_ranges and torch.cuda.mem_get_info()[0] < 110e9:
    print(f"two column ranges: skipped, {torch.cuda.mem_get_info()[0] / 1e9:.0f} GB free on this device (70 GB of rows + working memory needed)")
    sys.exit(0)

g = torch.Generator(device=dev).manual_seed(0)
db = torch.empty(ndb, dim, device=dev)
for r0 in range(0, ndb, BLOCK):
    n = min(BLOCK, ndb - r0)
    db[r0:r0 + n] = torch.randn(n, dim, generator=g, device=dev) * (0.3 + 2.0 * torch.rand(n, 1, generator=g, device=dev))
qu = torch.nn.functional.normalize(torch.randn(nq, dim, generator=g, device=dev))
for j in range(6):                                         # planted neighbours at graded distances (tests/test_gpu_screen.py)
    rows = torch.randint(0, ndb, (nq,), generator=g, device=dev)
    noise = torch.nn.functional.normalize(torch.randn(nq, dim, generator=g, device=dev))
    db[rows] = (qu + (0.02 + 0.0004 * j) * noise) * (0.5 + j)
print(f"{nq} queries x {ndb} rows x {dim} columns ({ndb * dim * 4 / 1e9:.1f} GB of rows), k = {k}, inner product over F.normalize(rows); "
      f"panel {ops.topk_index_panel(dim)} rows", flush=True)


def search():
    return ops.topk(qu, db, k, "ip", normalize_db=True)


def timed(warm=2, reps=5):
    for _ in range(warm):
        search()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = search()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), ms, out


def profiled():
    ops.profile_enable(True)
    ops.profile_reset()
    search()
    torch.cuda.synchronize()
    p = ops.profile_dump()
    ops.profile_enable(False)
    return {tag: round(v["ms"], 2) for tag, v in sorted(p.items())}


def float64_check(d, i, sel):
    """lists of the queries ``sel`` against a float64 flat search in row blocks; -> (float64 scores, leading-plane scores)"""
    q = qu[sel].double()
    s = torch.empty(len(sel), ndb, dtype=torch.float64, device=dev)
    s_hi = torch.empty_like(s)
    rho_d = 0.0
    # the leading plane of a row (csrc/gemm_h3.hip): scaled by a power of two so that its largest element lies in [2^14, 2^15), rounded to fp16
    def leading(x):
        e = torch.floor(torch.log2(x.abs().amax(dim=1, keepdim=True).clamp_min(1e-30)))
        scale = torch.exp2(14.0 - e)
        return (x * scale).half().double() / scale.double()
    q_hi = leading(qu[sel])
    rho_q = (q - q_hi).norm(dim=1) / q.norm(dim=1)
    for r0 in range(0, ndb, BLOCK):
        blk = db[r0:r0 + BLOCK]
        b64 = blk.double()
        nrm = b64.norm(dim=1).clamp_min(1e-12)
        hi = leading(blk)
        rho_d = max(rho_d, float(((b64 - hi).norm(dim=1) / nrm).max()))
        s[:, r0:r0 + BLOCK] = q @ (b64 / nrm[:, None]).t()
        s_hi[:, r0:r0 + BLOCK] = q_hi @ (hi / nrm[:, None]).t()
    o = torch.sort(s, dim=1, descending=True, stable=True)
    got = torch.gather(s, 1, i[sel])
    mism = i[sel] != o.indices[:, :k]
    worst = float((got[mism] - o.values[:, :k][mism]).abs().max()) if bool(mism.any()) else 0.0
    print(f"float64 check of {len(sel)} queries: max |distance - float64| {float((d[sel].double() - got).abs().max()):.2e}; "
          f"{int(mism.sum())} of {mism.numel()} entries differ (largest float64 score difference among them {worst:.1e})", flush=True)
    # candidates: rows whose leading-plane value is within the margin of the k-th best one (scores_screen.hip: screen_margin_kernel)
    k16 = dim // 16
    accum = (min(1536, k16) / 2.0 + 32.0 + 3.0 * -(-k16 // 1536)) / 8388608.0 * 1.01
    rq, rd = rho_q * 1.01 + 1e-9, rho_d * 1.01 + 1e-9
    bound = ((rq + rd + rq * rd) * (1.0 + 1.0 / 1024.0) + accum) * q.norm(dim=1)
    margin = 2.0 * bound * 1.0001 + 1e-6 * (1.0 + q.norm(dim=1))
    kth = torch.sort(s_hi, dim=1, descending=True).values[:, k - 1]
    cand = (s_hi >= (kth - margin)[:, None]).sum(1).float()
    print(f"candidates per query (restated in float64 for these queries; largest row residual {rho_d:.2e}, margin {float(margin.mean()):.2e}): "
          f"mean {float(cand.mean()):.1f}, min {int(cand.min())}, max {int(cand.max())} of at most 512", flush=True)


sel = torch.arange(0, nq, max(1, nq // 32), device=dev)[:32]
if two_ranges:
    with ops.options(topk_screen=1):
        d, i = search()
        torch.cuda.synchronize()
        prof = profiled()
    print(f"topk_screen=1 kernels (ms): {prof}", flush=True)
    print(f"screened without fallback: {'topk_screen_gemm' in prof and 'topk_scores_gemm' not in prof}", flush=True)
    float64_check(d, i, sel)
    sys.exit(0)

res, med = {}, {}
for screen in (0, 1):
    with ops.options(topk_screen=screen):
        med[screen], ms, res[screen] = timed()
        prof = profiled()
    print(f"topk_screen={screen}: median {med[screen]:8.1f} ms of {[round(m, 1) for m in ms]}", flush=True)
    print(f"    kernels (ms): {prof}", flush=True)
    if screen:
        rs = prof.get("topk_screen_rescore", 0.0)
        print(f"    screened without fallback: {'topk_screen_gemm' in prof and 'topk_scores_gemm' not in prof}; "
              f"re-scoring kernel {rs:.2f} ms = {100.0 * rs / sum(prof.values()):.1f} % of the kernel time, "
              f"{100.0 * rs / med[1]:.1f} % of the call", flush=True)
(d0, i0), (d1, i1) = res[0], res[1]
print(f"screened {med[1]:.1f} ms vs unscreened {med[0]:.1f} ms: x{med[0] / med[1]:.2f}; {int((i0 != i1).sum())} of {i0.numel()} indices differ, "
      f"max |distance difference| {float((d0 - d1).abs().max()):.2e}", flush=True)
float64_check(d1, i1, sel)
