"""DINOv2 with registers: ms per ViT forward, plain model against its _reg twin (the same synthetic blocks plus
four register tokens), ViT-G/14 in the h3 arithmetic, layer-31 'value' tokens:
  * a uniform 322 x 322 batch of B = 61 and of B = 1;
  * the 61-image mixed-size ragged set of tools/time_ragged.py (322x322, 224x224, 364x490, 308x420, 476x630).
Each figure is the median of --reps passes timed with HIP events after --warmup passes; the FFN-bound check of the product
path stays on.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(322, 322), (224, 224), (364, 490), (308, 420), (476, 630)]
N_IMG = 61
BASE, LAYER, FACET = "dinov2_vitg14", 31, "value"


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
    args = ap.parse_args()
    from anyloc_amd import synth
    from anyloc_amd.extractor import HipDinoV2
    dev = torch.device("cuda", torch.cuda.current_device())
    sd = synth.synthetic_state_dict(BASE + "_reg", seed=0, depth=LAYER + 1, device=str(dev))
    plain = HipDinoV2(BASE, {k: v for k, v in sd.items() if k != "register_tokens"}, dev, max_layer=LAYER, gemm="h3")
    reg = HipDinoV2(BASE + "_reg", sd, dev, max_layer=LAYER, gemm="h3")
    g = torch.Generator().manual_seed(61)
    pick = torch.randint(0, len(SIZES), (N_IMG,), generator=g).tolist()
    mixed = [torch.randn(3, *SIZES[p], generator=g).to(dev) for p in pick]
    uni = torch.randn(N_IMG, 3, 322, 322, generator=g).to(dev)
    taps = [(LAYER, FACET)]
    runs = {"uniform_322_b61": lambda m: m.forward_taps(uni, taps),
            "uniform_322_b1": lambda m: m.forward_taps(uni[:1], taps),
            "ragged_61_mixed": lambda m: m.forward_taps_ragged(mixed, taps)}
    rep = {"workload": f"ViT-G/14 h3, L{LAYER} '{FACET}' tokens, synthetic weights; _reg = the same blocks + 4 registers",
           "reps": args.reps}
    for name, fn in runs.items():
        a = _ms(lambda: fn(plain), args.reps, args.warmup)
        b = _ms(lambda: fn(reg), args.reps, args.warmup)
        rep[name] = {"plain_ms": round(a, 2), "reg_ms": round(b, 2), "reg_over_plain": round(b / a, 4)}
    rep["tokens_per_image_322"] = {"plain": 530, "reg": 534}
    rep["options"] = os.environ.get("ANYLOC_OPTIONS", "")
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
