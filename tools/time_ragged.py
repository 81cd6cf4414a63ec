"""Mixed-size batches (DESIGN 4.x "Mixed-size batches"): ViT-G/14 layer-31 'value' tokens + K = 32 hard VLAD of a fixed,
seeded set of 61 images of five sizes (322x322, 224x224, 364x490, 308x420, 476x630 -- T = 530 / 257 / 911 / 661 / 1531),
synthetic weights, timed three ways in one process with HIP events:
  (a) one image per call (extractor + VLAD per image: the only option for mixed sizes before the ragged forward),
  (b) the images grouped by size, one batched call per size,
  (c) one ragged call (forward_taps_ragged -> VLAD of the packed tokens);
and, for reference, a uniform batch of 61 images at 322 x 322.  Every path is warmed up first; the figure is the median of
--reps timed passes.  Prints one JSON line.  ``--reps 1 --warmup 1`` under ``rocprofv3 --kernel-trace --stats`` gives the
kernel table of one pass of each path."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(322, 322), (224, 224), (364, 490), (308, 420), (476, 630)]
N_IMG = 61
MODEL, LAYER, FACET, K = "dinov2_vitg14", 31, "value", 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import utilities
    from anyloc_amd import synth, weights
    dev = torch.device("cuda", torch.cuda.current_device())
    sd = synth.synthetic_state_dict(MODEL, seed=0, device=str(dev))
    weights.register_state_dict(MODEL, sd)
    ext = utilities.DinoV2ExtractFeatures(MODEL, LAYER, FACET, device=str(dev))
    g = torch.Generator().manual_seed(61)
    pick = torch.randint(0, len(SIZES), (N_IMG,), generator=g).tolist()
    imgs = [torch.randn(3, *SIZES[p], generator=g).to(dev) for p in pick]
    uni = torch.randn(N_IMG, 3, 322, 322, generator=g).to(dev)
    vlad = utilities.VLAD(K, None, cache_dir=None)
    np.random.seed(42)
    vlad.fit(ext(uni[:8]).reshape(-1, 1536))
    groups = {}
    for i, p in enumerate(pick):
        groups.setdefault(p, []).append(i)
    stacks = {p: torch.stack([imgs[i] for i in idx]) for p, idx in groups.items()}
    out = torch.empty(N_IMG, K * 1536, device=dev)

    def one_per_call():
        for i, x in enumerate(imgs):
            out[i] = vlad.generate(ext(x[None])[0])

    def by_size():
        for p, idx in groups.items():
            out[torch.tensor(idx, device=dev)] = vlad.generate_multi(ext(stacks[p]))

    def ragged():
        out.copy_(vlad.generate_multi(ext.extract_ragged(imgs, packed=True)))

    def uniform():
        vlad.generate_multi(ext(uni))

    paths = {"one_per_call": one_per_call, "by_size": by_size, "ragged": ragged, "uniform_322": uniform}
    res = {}
    for name, fn in paths.items():
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        res[name] = float(np.median(times))
    # the three mixed-size paths compute the same VLADs
    ragged()
    v_r = out.clone()
    one_per_call()
    v_a = out.clone()
    by_size()
    v_b = out.clone()
    tokens = sum((h // 14) * (w // 14) + 1 for h, w in (SIZES[p] for p in pick))
    rep = {"workload": f"ViT-G/14 L{LAYER} {FACET} + K={K} hard VLAD, {N_IMG} mixed images (T = 257..1531), synthetic weights",
           "sizes": {f"{SIZES[p][0]}x{SIZES[p][1]}": len(idx) for p, idx in sorted(groups.items())},
           "tokens": tokens, "uniform_tokens": N_IMG * 530, "reps": args.reps}
    for name, ms in res.items():
        n_tok = N_IMG * 530 if name == "uniform_322" else tokens
        rep[name] = {"ms": round(ms, 2), "images_per_s": round(N_IMG / ms * 1e3, 1), "ktokens_per_s": round(n_tok / ms, 1)}
    rep["ragged_vs_one_per_call_max_abs"] = float((v_r - v_a).abs().max())
    rep["ragged_vs_by_size_max_abs"] = float((v_r - v_b).abs().max())
    # hard cluster ids of every token on the three paths, and the VLADs of the images whose ids all agree
    from anyloc_amd import ops
    c = vlad._centers_dev()
    tok_r = ext.extract_ragged(imgs)
    tok_a = [ext(x[None])[0] for x in imgs]
    tok_b = [None] * N_IMG
    for p, idx in groups.items():
        t = ext(stacks[p])
        for j, i in enumerate(idx):
            tok_b[i] = t[j]
    labels = {}
    for name, toks in (("ragged", [t[0] for t in tok_r]), ("one_per_call", tok_a), ("by_size", tok_b)):
        labels[name] = ops.vlad(toks, c, return_labels=True, dist_mode=vlad.mode)[1].cpu()
    n_tok = [t.shape[1] for t in tok_r]
    bounds = np.concatenate([[0], np.cumsum(n_tok)])
    for other, v_o in (("one_per_call", v_a), ("by_size", v_b)):
        flips = (labels["ragged"] != labels[other]).numpy()
        imgs_flip = [i for i in range(N_IMG) if flips[bounds[i]:bounds[i + 1]].any()]
        clean = [i for i in range(N_IMG) if i not in imgs_flip]
        rep[f"ragged_vs_{other}_label_flips"] = int(flips.sum())
        rep[f"ragged_vs_{other}_images_with_a_flip"] = imgs_flip
        rep[f"ragged_vs_{other}_max_abs_without_flips"] = float((v_r[clean] - v_o[clean]).abs().max()) if clean else None
        rep[f"ragged_vs_{other}_token_max_abs"] = max(float((a[0] - b).abs().max()) for a, b in
                                                      zip(tok_r, tok_a if other == "one_per_call" else tok_b))
    rep["options"] = os.environ.get("ANYLOC_OPTIONS", "")
    print(json.dumps(rep))
    weights.unregister_state_dict(MODEL)


if __name__ == "__main__":
    main()
