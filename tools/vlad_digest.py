"""Bitwise digest of the aggregation stage (csrc/vlad.hip, csrc/vlad_fused.hip): for every case one JSON line with the SHA-256
of every tensor the call returns, what the size functions of the ABI answer for its shape and, from the library's profiler,
every launch tag with its ``calls``, ``flops`` and ``bytes`` (computed by the launch wrappers from the arguments they were
given; ``ms`` is left out).  The cases are the decisions the host code takes: fused kernel or general path, metric, flags,
the caller's and the library's workgroups-per-image count, the kernel-version options, empty images and empty calls, the
soft and given-assignment variants, the k-means step with its chunk options.  Two builds whose outputs of this tool are
byte-identical launch the same kernels on the same arguments and compute the same bits.

    python tools/vlad_digest.py > digest.jsonl          # needs the GPU; ``--list`` prints the case names only

Inputs come from anyloc_amd.synth with fixed seeds; 1 to 5 images of 0 to 100 tokens keep the whole matrix to seconds."""
import argparse
import hashlib
import itertools
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# tokens per image
BATCHES = {"b1": [40], "b3": [40, 100, 67], "b5_one_empty": [50, 0, 100, 40, 77], "b2_no_tokens": [0, 0]}
FUSED_D = (384, 768, 1024, 1536)


def _cases():
    out = []

    def add(op, D, K, batch=None, options=None, **kw):
        name = "/".join([op, f"D{D}", f"K{K}"] + ([batch] if batch else []) + [f"{k}={v}" for k, v in kw.items()] +
                        [f"opt:{k}={v}" for k, v in (options or {}).items()])
        out.append(dict(name=name, op=op, D=D, K=K, batch=batch, options=options or {}, kw=kw))
    # hard VLAD on the fused shapes
    for D, K, metric, batch in itertools.product(FUSED_D, (8, 32), ("cosine", "euclidean"), ("b1", "b3", "b5_one_empty")):
        add("vlad", D, K, batch, dist_mode=metric)
    for D, batch, norm, intra, labels in itertools.product(FUSED_D, ("b3", "b5_one_empty"), (0, 1), (0, 1), (0, 1)):
        add("vlad", D, 8, batch, norm_descs=norm, intra_norm=intra, return_labels=labels)
    for D, K, batch, parts in itertools.product(FUSED_D, (8, 32), ("b1", "b5_one_empty"), (3, 64)):
        add("vlad", D, K, batch, parts=parts, return_labels=1)
    for D, batch, parts in itertools.product(FUSED_D, ("b1", "b5_one_empty"), (0, 3)):
        add("vlad", D, 32, batch, options={"vlad_parts": 4}, parts=parts)
    for D, K, ver, parts in itertools.product(FUSED_D, (8, 32), (1, 3, 4), (0, 3)):
        add("vlad", D, K, "b3", options={"vlad_fused_v": ver}, parts=parts, return_labels=1)
    for D, K, metric, parts in itertools.product(FUSED_D, (8, 32), ("cosine", "euclidean"), (0, 3)):
        add("vlad", D, K, "b5_one_empty", options={"vlad_two_pass": 1}, dist_mode=metric, parts=parts, return_labels=1)
    for D, opts in itertools.product(FUSED_D, ({}, {"vlad_two_pass": 1}, {"vlad_parts": 4})):
        add("vlad", D, 8, "b2_no_tokens", options=opts, return_labels=1)
    # hard VLAD, general path
    for (D, K), metric, batch in itertools.product(((64, 8), (260, 32), (64, 33), (384, 33), (384, 129), (384, 256)),
                                                    ("cosine", "euclidean"), ("b3", "b5_one_empty", "b2_no_tokens")):
        add("vlad", D, K, batch, dist_mode=metric, return_labels=1)
    add("vlad", 260, 8, "b3", norm_descs=0, intra_norm=0, parts=3)
    # soft assignment
    for (D, K), batch, norm, intra in itertools.product(((384, 8), (384, 64), (64, 8)), ("b3", "b5_one_empty", "b2_no_tokens"),
                                                         (0, 1), (0, 1)):
        add("vlad", D, K, batch, mode="soft", norm_descs=norm, intra_norm=intra, soft_temp=1.5)
    for D, K in ((384, 8), (384, 64), (64, 33)):
        add("vlad_soft_weights", D, K, "b3")
    for D, K, norm in itertools.product((384, 64), (8, 33), (0, 1)):
        add("vlad_residuals", D, K, "b1", norm_descs=norm)
    # VLAD from a given assignment
    for (D, K), norm, intra in itertools.product(((384, 8), (260, 33), (384, 129), (384, 256)), (0, 1), (0, 1)):
        add("vlad_assigned", D, K, "b3", given="labels", norm_descs=norm, intra_norm=intra)
    for (D, K), norm in itertools.product(((384, 8), (260, 33), (384, 64)), (0, 1)):
        add("vlad_assigned", D, K, "b3", given="soft", norm_descs=norm)
    for given in ("labels", "soft"):
        add("vlad_assigned", 384, 8, "b2_no_tokens", given=given)
    # k-means
    for (D, K), mode, labels, n in itertools.product(((384, 8), (1536, 32), (64, 33), (384, 129), (384, 256)),
                                                      ("cosine", "euclidean"), (0, 1), (100, 3000)):
        add("kmeans_step", D, K, n=n, mode=mode, want_labels=labels)
    for (D, K), chunks in itertools.product(((1536, 32), (64, 33)), (1, 3)):
        add("kmeans_step", D, K, options={"kmeans_max_chunks": chunks}, n=3000, want_labels=1)
    for (D, K), ver in itertools.product(((384, 8), (1536, 32)), (1, 3)):
        add("kmeans_step", D, K, options={"kmeans_fused_v": ver}, n=3000, want_labels=1)
    add("kmeans_step", 1536, 32, options={"vlad_two_pass": 1}, n=3000, want_labels=1)
    for D, K in ((1536, 32), (64, 33)):
        add("kmeans_update", D, K, n=3000)
    assert len({c["name"] for c in out}) == len(out)
    return out


CASES = _cases()


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _inputs(c, dev):
    from anyloc_amd import synth
    D, K = c["D"], c["K"]
    centers = (0.8 * synth.clustered_tokens(1, K, D, K, seed=11)[0]).to(dev)
    if c["batch"] is None:
        return centers, synth.clustered_tokens(1, c["kw"]["n"], D, 16, seed=13)[0].to(dev)
    counts = BATCHES[c["batch"]]
    rows = synth.clustered_tokens(1, max(1, sum(counts)), D, 16, seed=13)[0][:sum(counts)].to(dev)
    return centers, list(rows.split(counts))


def _run(c, dev):
    """-> (named output tensors, what the size functions answer)"""
    from anyloc_amd import _lib, ops
    lib = _lib.load()
    D, K, kw = c["D"], c["K"], dict(c["kw"])
    centers, x = _inputs(c, dev)
    if c["op"] in ("kmeans_step", "kmeans_update"):
        n = kw.pop("n")
        sizes = {"kmeans_workspace_bytes": lib.anyloc_kmeans_workspace_bytes(n, D, K)}
        sums, counts, labels = ops.kmeans_step(x, centers, **kw)
        if c["op"] == "kmeans_update":
            new, err = ops.kmeans_update(sums, counts, centers)
            return {"centers": new, "err": err}, sizes
        return {"sums": sums, "counts": counts, **({"labels": labels} if labels is not None else {})}, sizes
    n_img, total = len(x), sum(t.shape[0] for t in x)
    sizes = {"workspace_bytes": lib.anyloc_vlad_workspace_bytes(total, n_img, D, K),
             "workspace_bytes_parts": lib.anyloc_vlad_workspace_bytes_parts(total, n_img, D, K, kw.get("parts", 0)),
             "auto_parts": lib.anyloc_vlad_auto_parts(total, n_img, D, K)}
    if c["op"] == "vlad":
        kw = {k: bool(v) if k in ("norm_descs", "intra_norm", "return_labels") else v for k, v in kw.items()}
        if kw.get("return_labels"):
            out, labels = ops.vlad(x, centers, **kw)
            return {"descriptors": out, "labels": labels}, sizes
        return {"descriptors": ops.vlad(x, centers, **kw)}, sizes
    rows = torch.cat(x) if total else torch.empty(0, D, device=dev)
    if c["op"] == "vlad_soft_weights":
        return {"weights": ops.vlad_soft_weights(rows, centers, soft_temp=1.5)}, sizes
    if c["op"] == "vlad_residuals":
        return {"residuals": ops.vlad_residuals(rows, centers, norm_descs=bool(kw["norm_descs"]))}, sizes
    given = kw.pop("given")
    g = torch.Generator().manual_seed(19)
    if given == "labels":
        a = dict(labels=torch.randint(0, K, (total,), generator=g).to(dev))
    else:
        a = dict(soft=torch.softmax(torch.randn(total, K, generator=g), dim=1).to(dev))
    return {"descriptor": ops.vlad_assigned(rows, centers, **a, **{k: bool(v) for k, v in kw.items()})}, sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", action="store_true", help="print the case names and exit (no GPU needed)")
    ap.add_argument("--only", default="", help="run the cases whose name contains this")
    args = ap.parse_args()
    cases = [c for c in CASES if args.only in c["name"]]
    if args.list:
        print("\n".join(c["name"] for c in cases))
        return
    from anyloc_amd import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    ops.profile_enable(True)
    for c in cases:
        with ops.options(**c["options"]):
            ops.profile_reset()
            outputs, sizes = _run(c, dev)
            torch.cuda.synchronize()
            launches = {tag: {k: v[k] for k in ("calls", "flops", "bytes")} for tag, v in sorted(ops.profile_dump().items())}
        print(json.dumps({"case": c["name"], "sha256": {k: _sha(v) for k, v in outputs.items()}, "sizes": sizes,
                          "launches": launches}), flush=True)


if __name__ == "__main__":
    main()
