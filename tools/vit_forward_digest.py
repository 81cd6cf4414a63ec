"""Bitwise digest of the ViT forward: for every case one JSON line with the SHA-256 of the output bytes (ragged: of the
packed rows and of the offsets), ``ffn_exact_blocks`` after the call and the ``ffn_reruns`` it added and, from the
library's profiler, every launch tag with its ``calls``, ``flops`` and ``bytes`` (computed by the launch wrappers from the
shapes they were given: equal figures mean equal launch arguments; ``ms`` is left out).  Two builds whose outputs of this tool are
byte-identical launch the same kernels on the same arguments and compute the same bits; the order of the launches inside
one tag is not visible here, equal outputs cover it.  The last lines are ``ops.gemm_nt_h3`` on its own (``gemm_nt_h3/...``), one
shape per route of the two-term fp16 GEMM's planner; which kernel and grid a launch got is tools/kernel_trace_launches.py's part.

    python tools/vit_forward_digest.py > digest.jsonl          # needs the GPU; ``--list`` prints the case names only

Synthetic weights (anyloc_amd.synth, fixed seeds) cut to three blocks keep the whole matrix to a minute or two."""
import argparse
import hashlib
import itertools
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEPTH = 3
GEMMS = ("f32", "x6", "h3")
MODELS = ("dinov2_vits14", "dinov2_vitg14", "dinov2_vitg14_reg")          # GELU; SwiGLU; SwiGLU + registers
# name -> ("uniform", B, H, W) | ("ragged", [(H, W), ...])
SHAPES = {"b1_224": ("uniform", 1, 224, 224),                             # small-M plans
          "b3_322": ("uniform", 3, 322, 322),
          "ragged3": ("ragged", [(224, 308), (322, 322), (140, 224)]),
          "b4_322": ("uniform", 4, 322, 322),                             # 2 120 token rows: above x6_min_rows
          "ragged3_big": ("ragged", [(322, 322), (448, 448), (224, 308)]),    # 1 908 token rows: the same
          "b17_322": ("uniform", 17, 322, 322),                           # 71 tile rows of 128: the batched lead plan passes
          "b1_322": ("uniform", 1, 322, 322),                             # 530 rows: the 192 x 128 w12 plan, split-K 2 on fc2
          "b2_322": ("uniform", 2, 322, 322),                             # 1 060 rows: the two-image column of the plan table
          "b1_476x630": ("uniform", 1, 476, 630)}                         # 1 531 rows: the plans of up to 1 700 rows
TAPS = {"token_last": [(2, "token")],
        "value_last": [(2, "value")],                                     # the facet-only exit
        "key_token_last": [(2, "key"), (2, "token")],
        "q0_t1_v2_unordered": [(1, "token"), (2, "value"), (0, "query")]}
# option sets of the h3 forward beyond the defaults (h3_swiglu_t is read when the model is built); x6_fuse rides on x6
H3_OPTIONS = ({"h3_fuse": 0}, {"h3_patch": 0}, {"h3_swiglu_t": 0}, {"h3_min_rows": 1 << 20}, {"h3s_ln_lead": 1})
# what decides how a two-term fp16 GEMM is launched, at the shapes of the small-M plan table
H3_PLAN_OPTIONS = ({}, {"h3s_enable": 0}, {"h3s_w12_tall": 0}, {"h3_epi_lds": 0}, {"h3s_ln_lead": 1})
# ops.gemm_nt_h3 on its own, hashed the same way: (M, N, K, options)
GEMM_NT_H3 = ((4096, 4096, 4096, {}),                                     # 256 tiles of 256 x 256, K16 = 256: the 16 x 16 x 32 MFMA kernel
              (4096, 4096, 4096, {"h3_mfma16": 0}),
              (300, 700, 64, {}),                                         # small-M plan, no split-K buffers
              (3000, 40000, 128, {}))                                     # batched default tile
# weights: "synth" | "outlier" (synth.outlier_state_dict) | "loose" (one fc1 row of huge norm in block 1: the FFN bound of
# every image trips).  threshold: None = the stock FFN_LOOSENESS_MAX; "between" = the middle of the images' own figures,
# so that only some images are run again; "median" = the median of all (block, image) figures: several groups of blocks


def _cases():
    out = []

    def add(model, gemm, shape, taps, use_cls=False, norm_concat=False, options=None, ffn_check=True, weights="synth",
            threshold=None):
        out.append(dict(model=model, gemm=gemm, shape=shape, taps=taps, use_cls=use_cls, norm_concat=norm_concat,
                        options=options or {}, ffn_check=ffn_check, weights=weights, threshold=threshold))
    for model, gemm, shape, taps, cls in itertools.product(MODELS, GEMMS, ("b1_224", "b3_322", "ragged3"), TAPS, (False, True)):
        add(model, gemm, shape, taps, use_cls=cls)
    for model, gemm in itertools.product(MODELS, GEMMS):
        add(model, gemm, "b4_322", "token_last")
        add(model, gemm, "b4_322", "q0_t1_v2_unordered", use_cls=True, norm_concat=True)
        add(model, gemm, "ragged3_big", "q0_t1_v2_unordered", norm_concat=True)
    for model, shape, taps, cls in itertools.product(MODELS, ("b4_322", "ragged3_big"), TAPS, (False, True)):
        add(model, "x6", shape, taps, use_cls=cls, options={"x6_fuse": 1 - cls})
    for model, opts, shape, taps in itertools.product(MODELS, H3_OPTIONS, ("b1_224", "b3_322", "ragged3"),
                                                      ("token_last", "value_last", "q0_t1_v2_unordered")):
        add(model, "h3", shape, taps, options=opts)
    for model, check in itertools.product(MODELS, (True, False)):
        add(model, "h3", "b17_322", "token_last", options={"h3_ln_lead": 1}, ffn_check=check)
        if not check:                                                     # (with the check: among the cases above)
            add(model, "h3", "b1_224", "token_last", options={"h3s_ln_lead": 1}, ffn_check=False)
            add(model, "h3", "b3_322", "key_token_last", ffn_check=False)
    for shape in ("b3_322", "ragged3"):
        add("dinov2_vits14", "h3", shape, "token_last", weights="loose")                        # every image is run again
        add("dinov2_vits14", "h3", shape, "token_last", weights="loose", threshold="between")   # some images
        add("dinov2_vits14", "h3", shape, "token_last", threshold="median")
        add("dinov2_vitg14", "h3", shape, "token_last", threshold="median")
        for gemm in GEMMS:
            add("dinov2_vits14", gemm, shape, "token_last", weights="outlier")
    for model, opts, shape in itertools.product(MODELS, H3_PLAN_OPTIONS, ("b1_322", "b2_322", "b1_476x630")):
        add(model, "h3", shape, "token_last", options=opts)
    for opts in [{"h3_epi_lds": 0}] + [{"h3_cfg": c} for c in range(1, 6)]:
        add("dinov2_vits14", "h3", "b4_322", "token_last", options=opts)
    for c in out:
        c["name"] = "/".join([c["model"], c["gemm"], c["shape"], c["taps"]] + (["cls"] if c["use_cls"] else []) +
                             (["norm_concat"] if c["norm_concat"] else []) + [f"{k}={v}" for k, v in c["options"].items()] +
                             ([] if c["ffn_check"] else ["ffn_check=0"]) + ([] if c["weights"] == "synth" else [c["weights"]]) +
                             ([f"thr_{c['threshold']}"] if c["threshold"] else []))
    assert len({c["name"] for c in out}) == len(out)
    return out


CASES = _cases()


def _state_dict(model, kind, dev):
    from anyloc_amd import synth
    sd = synth.synthetic_state_dict(model, seed=5, depth=DEPTH, device=str(dev))
    if kind == "outlier":
        sd = synth.outlier_state_dict(sd, model, seed=3)
    if kind == "loose":
        # tests/test_gpu_vit.py, test_ffn_bound_telemetry_switches_a_loose_block_to_the_exact_quantiser: fc1 row 7 of block 1
        # along the one direction LayerNorm 2's output cannot move in -- a huge bound, unchanged activations
        w, b = sd["blocks.1.norm2.weight"].double(), sd["blocks.1.norm2.bias"].double()
        d = (1.0 / w) / (1.0 / w).norm()
        f1 = sd["blocks.1.mlp.fc1.weight"].double()
        c = 3000.0 * float(f1.norm(dim=1).max())
        f1[7] = c * d
        sd["blocks.1.mlp.fc1.weight"] = f1.float()
        sd["blocks.1.mlp.fc1.bias"][7] = float(-c * (d * b).sum())
    return sd


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", action="store_true", help="print the case names and exit (no GPU needed)")
    ap.add_argument("--only", default="", help="run the cases whose name contains this")
    args = ap.parse_args()
    cases = [c for c in CASES if args.only in c["name"]]
    gemms = [(f"gemm_nt_h3/{M}x{N}x{K}" + "".join(f"/{k}={v}" for k, v in o.items()), M, N, K, o) for M, N, K, o in GEMM_NT_H3]
    gemms = [g for g in gemms if args.only in g[0]]
    if args.list:
        print("\n".join([c["name"] for c in cases] + [g[0] for g in gemms]))
        return
    from anyloc_amd import extractor as ex, ops
    from anyloc_amd.extractor import HipDinoV2
    dev = torch.device("cuda", torch.cuda.current_device())
    stock = ex.FFN_LOOSENESS_MAX
    g = torch.Generator().manual_seed(17)
    inputs = {}
    for name, spec in SHAPES.items():
        sizes = [(spec[2], spec[3])] * spec[1] if spec[0] == "uniform" else spec[1]
        imgs = [torch.randn(3, h, w, generator=g).to(dev) for h, w in sizes]
        inputs[name] = torch.stack(imgs) if spec[0] == "uniform" else imgs
    models = {}
    ops.profile_enable(True)
    for c in cases:
        build_opts = {k: v for k, v in c["options"].items() if k == "h3_swiglu_t"}
        key = (c["model"], c["gemm"], c["weights"], tuple(build_opts.items()))
        if key not in models:
            with ops.options(**build_opts):
                models[key] = HipDinoV2(c["model"], _state_dict(c["model"], c["weights"], dev), dev, gemm=c["gemm"])
        m = models[key]
        m.ffn_check = c["ffn_check"]
        taps, x = TAPS[c["taps"]], inputs[c["shape"]]
        ragged = SHAPES[c["shape"]][0] == "ragged"
        run = (lambda: m.forward_taps_ragged(x, taps, use_cls=c["use_cls"], norm_concat=c["norm_concat"])) if ragged else \
            (lambda: (m.forward_taps(x, taps, use_cls=c["use_cls"], norm_concat=c["norm_concat"]), None))
        with ops.options(**c["options"]):
            if c["threshold"]:
                # a first call at the stock threshold leaves the per-image figures in m._telemetry [blocks, images]
                run()
                fig = m._telemetry[:DEPTH * len(x)].cpu().reshape(DEPTH, len(x))
                per_img = fig.max(dim=0).values.sort().values
                ex.FFN_LOOSENESS_MAX = float(0.5 * (per_img[0] + per_img[1])) if c["threshold"] == "between" \
                    else float(fig.flatten().sort().values[fig.numel() // 2 - 1:fig.numel() // 2 + 1].mean())
            runs0 = m.ffn_reruns
            ops.profile_reset()
            try:
                out, offsets = run()
                torch.cuda.synchronize()
                launches = {tag: {k: v[k] for k in ("calls", "flops", "bytes")} for tag, v in sorted(ops.profile_dump().items())}
            finally:
                ex.FFN_LOOSENESS_MAX = stock
        rec = {"case": c["name"], "sha256": _sha(out)}
        if ragged:
            rec["offsets_sha256"] = _sha(offsets)
        rec.update(ffn_exact_blocks=sorted(int(b) for b in m.ffn_exact_blocks), ffn_reruns=m.ffn_reruns - runs0, launches=launches)
        print(json.dumps(rec), flush=True)
        m.ffn_check = True
    for name, M, N, K, opts in gemms:
        a, w = (torch.randn(r, K, generator=torch.Generator().manual_seed(s)).to(dev) for r, s in ((M, 23), (N, 29)))
        with ops.options(**opts):
            a2, w2 = ops.split_h2(a), ops.split_h2(w)
            ops.profile_reset()
            out = ops.gemm_nt_h3(a2, w2, M, N, K)
            torch.cuda.synchronize()
            launches = {tag: {k: v[k] for k in ("calls", "flops", "bytes")} for tag, v in sorted(ops.profile_dump().items())}
        print(json.dumps({"case": name, "sha256": _sha(out), "launches": launches}), flush=True)


if __name__ == "__main__":
    main()
