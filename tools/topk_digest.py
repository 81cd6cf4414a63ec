"""Bitwise digest of the retrieval stage (csrc/topk.hip): for every case one JSON line with the SHA-256 of ``dist`` and ``idx``,
what ``anyloc_topk_workspace_bytes``, ``anyloc_topk_index_workspace_bytes``, ``anyloc_topk_index_bytes`` and ``anyloc_topk_path``
answer for its shape under its options and, from the library's profiler, every launch tag with its ``calls``, ``flops`` and
``bytes`` (computed by the launch wrappers from the arguments they were given; ``ms`` is left out).  The cases are the decisions
the host code takes, each at the smallest shape that reaches it: the three scoring paths with one and two panels, the few-query
arithmetics, k-chunks, the prepared index (built at once and by ranges, searched with and without its rows), the screened
search (column ranges, k-chunks, the k limit, the overflow fallback), the empty database, k beyond the database, a call without queries (k = 0 is outside the documented [1, 1024] and refused).
Two builds whose outputs of this tool are byte-identical launch the same tagged work and compute the same bits.

The ``rescore_rows`` and ``rescore_planes`` cases (70 queries x 300 rows) reach every instantiation of the re-scoring kernels of
csrc/scores_screen.hip (the names of tests/kernel_coverage.tsv) under the tags ``topk_screen_rescore`` and
``topk_screen_rescore_planes``; a ``+ 16`` row has two slices, the second one k-block long:

    dim (one slice)        rows: screen_rescore_kernel    planes: screen_rescore_planes_kernel
      2 048                  <1>                            --
      4 096                  <2>                            <1>
      8 192                  <4>                            <2>
     16 384                  <8>                            <4>
     32 768                  <16>                           <8>
     49 152                  <24>                           <12>
    topk_rescore_cols, dim   rows: screen_rescore_sliced_kernel    planes: screen_rescore_planes_sliced_kernel
      4 096,  4 112          <2>                            <1>
      8 192,  8 208          <4>                            <2>
     16 384, 16 400          <8>                            <4>
     32 768, 32 784          <16>                           <8>
     36 864, 36 880          <24>                           -- (the planes' slices end at 32 768 columns: <8> again)

(checked with ``rocprofv3 --kernel-trace`` around ``--only rescore_`` and ``tools/kernel_coverage.py launched``).

    python tools/topk_digest.py > digest.jsonl          # needs the GPU; ``--list`` prints the case names only

Inputs are torch.randn on the CPU from fixed seeds; the largest case (32 868 x 4096) holds half a gigabyte."""
import argparse
import functools
import hashlib
import itertools
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H3, SCREEN = {"topk_h3": 1, "topk_screen": 0}, {"topk_h3": 1, "topk_screen": 1}
VARIANTS = tuple(itertools.product(("ip", "l2"), (0, 1)))              # metric x normalize_db
RESCORE_DIMS = (2048, 4096, 8192, 16384, 32768, 49152)                 # the whole row in one slice: the top of every width class
RESCORE_COLS = (4096, 8192, 16384, 32768, 36864)                       # topk_rescore_cols, on rows 16 columns wider: two slices


def _cases():
    out = []

    def add(group, nq, ndb, dim, k=10, options=None, variants=VARIANTS, **kw):
        for metric, norm in variants:
            name = "/".join([group, f"q{nq}", f"n{ndb}", f"d{dim}", f"k{k}", metric, f"norm{norm}"] +
                            [f"{a}={b}" for a, b in kw.items()] + [f"opt:{a}={b}" for a, b in (options or {}).items()])
            out.append(dict(name=name, nq=nq, ndb=ndb, dim=dim, k=k, metric=metric, norm=norm, options=options or {}, kw=kw))
    one = (("ip", 0),)
    # fp32 panels: one, two
    add("f32", 9, 103, 64)
    add("f32", 9, 103, 64, variants=one, index_base=1000)
    add("f32", 70, 32868, 64)
    # few queries: every arithmetic, with and without the pre-split query image; two panels with different split-K factors
    for x6, qdma in itertools.product((0, 1, 2), (0, 1)):
        add("fewq", 5, 300, 4096, options={"topk_fewq_x6": x6, "topk_fewq_qdma": qdma})
    add("fewq", 5, 300, 4096, variants=one, index_base=1000)
    add("fewq", 5, 32868, 4096)
    # fp16 panels: one, two with a short last one, two k-chunks (the second one k-block long)
    add("h3", 70, 300, 256, options=H3)
    add("h3", 70, 300, 256, options=H3, variants=one, index_base=1000)
    add("h3", 70, 8492, 64, options=H3)
    add("h3", 70, 300, 8208, options=H3)
    # prepared index: without its rows (built at once and by ranges), with them, re-scoring from its planes
    for nq in (5, 70):
        add("index", nq, 8492, 64, index="whole")
        add("index", nq, 8492, 64, index="ranges")
        add("index_rows", nq, 8492, 64, options={"topk_screen": 1}, index="whole", rows=1)
        add("index_planes", nq, 8492, 64, options={"topk_screen": 1}, index="whole", rescore_planes=1)
    add("index", 70, 8492, 64, variants=one, index="whole", index_base=1000)
    # screened search on the rows: raw and normalised, two column ranges, two k-chunks, the largest k it serves and the next,
    # and a query with more near-duplicates inside its bound than the candidate list holds (the unscreened fallback)
    add("screen", 70, 8492, 256, options=SCREEN)
    add("screen", 70, 8492, 256, options=SCREEN, variants=one, index_base=1000)
    add("screen", 70, 131372, 64, options=SCREEN)
    add("screen", 70, 300, 24592, options=SCREEN)
    for k in (128, 129):
        add("screen", 70, 8492, 256, k=k, options=SCREEN)
    add("screen_overflow", 70, 1000, 256, options=SCREEN, duplicates=1)
    # every instantiation of the four re-scoring kernels (the table in the docstring), from the fp32 rows and from the planes
    for dim, cols in [(d, 0) for d in RESCORE_DIMS] + [(c + 16, c) for c in RESCORE_COLS]:
        sliced = {"topk_rescore_cols": cols} if cols else {}
        add("rescore_rows", 70, 300, dim, options=dict(SCREEN, **sliced))
        if dim >= 4096 and cols != RESCORE_COLS[-1]:
            add("rescore_planes", 70, 300, dim, options=dict({"topk_screen": 1}, **sliced), index="whole", rescore_planes=1)
    # edges: empty database (the padding list), k beyond the database, k = 1 and the largest k, calls that launch nothing
    add("edge", 9, 0, 64)
    add("edge", 9, 5, 64)
    for k in (1, 1024):
        add("edge", 9, 1100, 64, k=k)
    add("edge", 0, 103, 64, variants=one)
    assert len({c["name"] for c in out}) == len(out)
    return out


CASES = _cases()


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


@functools.lru_cache(maxsize=2)      # the variants of a case follow each other
def _randn(rows, dim, seed, dev):
    return torch.randn(rows, dim, generator=torch.Generator().manual_seed(seed)).to(dev)


def _run(c, dev):
    """-> (dist, idx)"""
    from anyloc_amd import ops
    nq, ndb, dim, k, kw = c["nq"], c["ndb"], c["dim"], c["k"], c["kw"]
    qu, db = _randn(nq, dim, 2, dev), _randn(ndb, dim, 1, dev)
    if kw.get("duplicates"):
        db = db.clone()
        db[200:900] = 3.0 * qu[0]
    common = dict(metric=c["metric"], index_base=kw.get("index_base", 0), normalize_db=bool(c["norm"]))
    if "index" not in kw:
        return ops.topk(qu, db, k, **common)
    if kw["index"] == "whole":
        index = ops.topk_index_build(db)
    else:           # the last panel first, then the others in one range
        panel = ops.topk_index_panel(dim)
        last = (ndb - 1) // panel * panel
        index = torch.empty(ops.topk_index_bytes(ndb, dim), dtype=torch.uint8, device=dev)
        ops.topk_index_build_range(index, db[last:], last, ndb)
        ops.topk_index_build_range(index, db[:last], 0, ndb)
    return ops.topk_indexed(qu, index, ndb, k, db=db if kw.get("rows") else None, rescore_planes=bool(kw.get("rescore_planes")), **common)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", action="store_true", help="print the case names and exit (no GPU needed)")
    ap.add_argument("--only", default="", help="run the cases whose name contains this")
    args = ap.parse_args()
    cases = [c for c in CASES if args.only in c["name"]]
    if args.list:
        print("\n".join(c["name"] for c in cases))
        return
    from anyloc_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    ops.profile_enable(True)
    for c in cases:
        with ops.options(**c["options"]):
            ops.profile_reset()
            dist, idx = _run(c, dev)
            torch.cuda.synchronize()
            launches = {tag: {k: v[k] for k in ("calls", "flops", "bytes")} for tag, v in sorted(ops.profile_dump().items())}
            shape = (c["nq"], c["ndb"], c["dim"])
            sizes = {"workspace_bytes": lib.anyloc_topk_workspace_bytes(*shape, c["k"]),
                     # (asked for at least one query: builds before the TopkPlan divided by the empty query chunk here)
                     "index_workspace_bytes": lib.anyloc_topk_index_workspace_bytes(*shape, c["k"]) if c["nq"] else 0,
                     "index_bytes": lib.anyloc_topk_index_bytes(c["ndb"], c["dim"]), "path": lib.anyloc_topk_path(*shape)}
        print(json.dumps({"case": c["name"], "sha256": {"dist": _sha(dist), "idx": _sha(idx)}, "sizes": sizes, "launches": launches}),
              flush=True)


if __name__ == "__main__":
    main()
