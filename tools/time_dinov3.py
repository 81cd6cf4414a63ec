"""DINOv3: ms per ViT forward of ViT-L/16 in the h3 arithmetic, layer-23 'value' tokens, with the rotation
(the model as it is) and with ``anyloc_vit_set_rope(h, 0)`` on the same handle (the same launches minus the rotation, `pos` a table of
zeros; the rows then carry no position at all -- a timing twin, not a model):
  * a uniform 320 x 320 batch of B = 61 and of B = 1 (405 token rows per image: CLS, 4 registers, 400 patches);
  * a 61-image mixed-size ragged set (320x320, 224x224, 368x496, 304x416, 480x640).
Each figure is the median of --reps passes timed with HIP events after --warmup passes; the FFN-bound check of the product
path stays on.  ``--only uniform_320_b61 --rope 1|0`` runs one case alone in a loop (for a kernel trace).  Prints one JSON
line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(320, 320), (224, 224), (368, 496), (304, 416), (480, 640)]
N_IMG = 61
NAME, LAYER, FACET = "dinov3_vitl16", 23, "value"


def _ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, help="run this case alone")
    ap.add_argument("--rope", type=int, default=None, help="with --only: 1 = with the rotation, 0 = without")
    args = ap.parse_args()
    from anyloc_amd import _lib, synth
    from anyloc_amd.extractor import HipDinoV2
    dev = torch.device("cuda", torch.cuda.current_device())
    sd = synth.synthetic_state_dict(NAME, seed=0, depth=LAYER + 1, device=str(dev))
    model = HipDinoV2(NAME, sd, dev, max_layer=LAYER, gemm="h3")
    lib = _lib.load()

    rope_tables, zero_tables = model.pos_table, {}

    def zero_table(H, W):
        # without the rotation the forward reads `pos` as a positional table [1 + N, D] again: zeros of that shape
        if (H, W) not in zero_tables:
            zero_tables[(H, W)] = torch.zeros(1 + (H // 16) * (W // 16), model.dim, device=dev)
        return zero_tables[(H, W)]

    def set_rope(on):
        _lib.check(lib.anyloc_vit_set_rope(model._handle, int(on)), "anyloc_vit_set_rope")
        model.pos_table = rope_tables if on else zero_table
    g = torch.Generator().manual_seed(61)
    pick = torch.randint(0, len(SIZES), (N_IMG,), generator=g).tolist()
    mixed = [torch.randn(3, *SIZES[p], generator=g).to(dev) for p in pick]
    uni = torch.randn(N_IMG, 3, 320, 320, generator=g).to(dev)
    taps = [(LAYER, FACET)]
    runs = {"uniform_320_b61": lambda: model.forward_taps(uni, taps),
            "uniform_320_b1": lambda: model.forward_taps(uni[:1], taps),
            "ragged_61_mixed": lambda: model.forward_taps_ragged(mixed, taps)}
    rep = {"workload": f"ViT-L/16 h3, L{LAYER} '{FACET}' tokens, synthetic weights; no_rope = the same handle after "
                       "anyloc_vit_set_rope(h, 0)", "reps": args.reps}
    try:
        for name, fn in runs.items():
            if args.only and name != args.only:
                continue
            res = {}
            for on in ((1, 0) if args.rope is None else (args.rope,)):
                set_rope(on)
                res["rope_ms" if on else "no_rope_ms"] = round(_ms(fn, args.reps, args.warmup), 3)
            if len(res) == 2:
                res["rope_over_no_rope"] = round(res["rope_ms"] / res["no_rope_ms"], 4)
            rep[name] = res
    finally:
        set_rope(1)
    rep["token_rows_per_image_320"] = 405
    rep["options"] = os.environ.get("ANYLOC_OPTIONS", "")
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
