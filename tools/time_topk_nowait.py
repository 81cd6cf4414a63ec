"""ANYLOC_TOPK_NO_WAIT: device time and host time-until-return of the screened search, waiting (default) against
``no_wait=True``, on
  a  600 x 20 000 x 4096         one-shot ``ops.topk``
  b  1 000 x 10 000 x 49 152     one-shot ``ops.topk``
  c  10 000 x 125 000 x 49 152   (the configs[2] shard) on a resident ``FlatIndex`` with its rows, and on a rows-free one
with four inputs each: no overflow; one zero query; 700 copies of one query's best row; 200 zero queries.
Method: one warm-up pass of both paths, then --reps interleaved passes (waiting, flagged, waiting, ...), each call between two HIP
events and two host clock reads; per path the median with min - max of the device times and the median host time.  Option
topk_screen = 1 throughout (shape b has fewer rows than the default rule asks for).  ``--scale`` shrinks the database rows and
the queries of a shape that does not fit (recorded in the output).  One JSON line per row of the table, then the table."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"a": (600, 20000, 4096), "b": (1000, 10000, 49152), "c": (10000, 125000, 49152)}
K = 20
DEV = "cuda"


def _data(nq, ndb, dim, seed):
    """the recipe of tests/test_gpu_screen.py: rows of norms 0.3 .. 2.3, unit queries, six planted neighbours per query"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    db = torch.randn(ndb, dim, generator=g, device=DEV)
    db.mul_(0.3 + 2.0 * torch.rand(ndb, 1, generator=g, device=DEV))
    qu = torch.nn.functional.normalize(torch.randn(nq, dim, generator=g, device=DEV))
    for j in range(6):
        rows = torch.randint(0, ndb, (nq,), generator=g, device=DEV)
        noise = torch.nn.functional.normalize(torch.randn(nq, dim, generator=g, device=DEV))
        db[rows] = (qu + (0.02 + 0.0004 * j) * noise) * (0.5 + j)
        del noise
    return qu, db


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    b.record()
    b.synchronize()
    return a.elapsed_time(b), host


def _measure(paths, reps):
    """paths: {name: callable}; interleaved -> {name: dict(dev_ms, dev_min, dev_max, host_ms)}"""
    for fn in paths.values():
        fn()
    torch.cuda.synchronize()
    got = {name: [] for name in paths}
    for _ in range(reps):
        for name, fn in paths.items():
            got[name].append(_timed(fn))
    out = {}
    for name, v in got.items():
        dev, host = [x[0] for x in v], [x[1] for x in v]
        out[name] = dict(dev_ms=round(float(np.median(dev)), 3), dev_min=round(min(dev), 3), dev_max=round(max(dev), 3),
                         host_ms=round(float(np.median(host)), 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink queries and database rows of shape c by this factor")
    ap.add_argument("--log", default=None, help="append the JSON lines and the table to this file")
    args = ap.parse_args()
    from anyloc_amd import ops, retrieval
    rows_out = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        rows_out.append(rec)
        if args.log:
            with open(args.log, "a") as f:
                f.write(json.dumps(rec) + "\n")

    with ops.options(topk_screen=1):
        for name in args.shapes.split(","):
            nq, ndb, dim = SHAPES[name]
            if name == "c" and args.scale != 1.0:
                nq, ndb = int(nq * args.scale), int(ndb * args.scale)
            qu, db = _data(nq, ndb, dim, nq + ndb + dim)
            one_zero, many_zero = qu.clone(), qu.clone()
            one_zero[3] = 0.0
            many_zero[torch.arange(0, nq, max(1, nq // 200), device=DEV)[:200]] = 0.0

            def searchers():
                if name != "c":
                    return {"one-shot": lambda q, nw: ops.topk(q, db, K, "ip", normalize_db=True, no_wait=nw)}
                index = retrieval.FlatIndex(db, "cosine", True, planes=True)
                free = copy.copy(index)                      # the same planes, no rows: what keep_fp32=False, rescore="planes" builds
                free.db, free.rescore = None, "planes"
                return {"FlatIndex, rows": lambda q, nw: index.search(q, K, no_wait=nw),
                        "FlatIndex, rows-free": lambda q, nw: free.search(q, K, no_wait=nw)}

            def run(case, q, how):
                for kind, search in how.items():
                    ops.profile_enable(True); ops.profile_reset()
                    search(q, False)
                    torch.cuda.synchronize()
                    fell_back = "topk_scores_gemm" in ops.profile_dump()
                    ops.profile_enable(False)
                    d0, i0 = search(q, False)
                    d1, i1 = search(q, True)
                    differ = int((i0 != i1).any(1).sum())
                    res = _measure({"waiting": lambda: search(q, False), "no_wait": lambda: search(q, True)}, args.reps)
                    emit(dict(shape=name, nq=nq, ndb=ndb, dim=dim, search=kind, case=case, waiting_fell_back=fell_back,
                              lists_that_differ=differ, **{f"{p}_{k}": v for p, r in res.items() for k, v in r.items()}))

            how = searchers()
            run("no overflow", qu, how)
            run("one zero query", one_zero, how)
            run("200 zero queries", many_zero, how)
            del how
            db[100] = 3.0 * qu[0]                            # 700 copies of one query's best row: the index is built again
            db[3000:3700] = db[100].clone().expand(700, -1)
            run("700 duplicates", qu, searchers())
            del qu, db, one_zero, many_zero
            torch.cuda.empty_cache()

    head = "| shape | search | case | waiting ms (min - max) | host ms | no_wait ms (min - max) | host ms |"
    lines = [head, "|---|---|---|---|---|---|---|"]
    for r in rows_out:
        lines.append(f"| {r['shape']} {r['nq']} x {r['ndb']} x {r['dim']} | {r['search']} | {r['case']} | "
                     f"{r['waiting_dev_ms']:.2f} ({r['waiting_dev_min']:.2f} - {r['waiting_dev_max']:.2f}) | {r['waiting_host_ms']:.2f} | "
                     f"{r['no_wait_dev_ms']:.2f} ({r['no_wait_dev_min']:.2f} - {r['no_wait_dev_max']:.2f}) | {r['no_wait_host_ms']:.2f} |")
    print("\n".join(lines))
    if args.log:
        with open(args.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
