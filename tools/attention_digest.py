"""Bitwise digest of the attention kernels on their own (csrc/attention.hip through ``anyloc_attention``, ``anyloc_attention_h3``
and their ``_ragged`` twins): for every case one JSON line with the SHA-256 of the output bytes -- for the two-term fp16 kernel
the h2 image and ``out_inv`` -- and the ``calls``, ``flops`` and ``bytes`` of the profiler's ``attention`` tag.  The cases are the
decisions the host code takes: every workgroup shape of the two-term fp16 kernel forced and chosen by the 512-workgroup rule (the
shapes ``(85, 100, 2)`` and ``(86, 100, 2)`` are its two sides), the options that lose against another one (``attn_h3_qg`` against
the key split and in ragged calls, ``attn_cfg`` against ``attn_x6`` and in ragged calls), both ragged workgroup orders with a
padded and an unpadded grid (``heads * n_img`` a multiple of 8 or not).  Two builds whose outputs of this tool are byte-identical
take the same decisions and compute the same bits; the plane-image outputs and the default options inside a forward are
``vit_forward_digest.py``'s.

    python tools/attention_digest.py > digest.jsonl          # needs the GPU; ``--list`` prints the case names only

Inputs are the spiky generators of tests/test_gpu_kernels.py (uniform) and tests/test_gpu_ragged.py (packs), fixed seeds."""
import argparse
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(2, 257, 6), (1, 530, 24), (3, 33, 2), (1, 128, 1), (2, 1370, 2), (5, 530, 4), (1, 20, 3),      # test_attention_h3's
          (85, 100, 2), (86, 100, 2)]               # 3 * 2 * B = 510 / 516 key-split workgroups: the two sides of the rule
RAGGED_T = [530, 2, 2100, 197, 37, 1531]            # tests/test_gpu_ragged.py: 12 units at 2 heads, the dealt grid padded to 16
PACKS = {"ragged_t": RAGGED_T, "ragged_t4": RAGGED_T[:4],                                      # 8 units: no padding
         "n85": [100, 37] * 42 + [100], "n86": [100, 37] * 43}                                 # 170 / 172 units, 510 / 516
HEADS_RAGGED = 2
H3_SETS = [dict(attn_h3_ks=ks, attn_h3_qg=qg) for ks, qg in ((0, 1), (1, 1), (2, 1), (0, 2), (1, 2), (2, 2))]
F32_SETS = [dict(attn_x6=x6, attn_cfg=cfg) for x6, cfg in itertools.product((0, 1), (0, 1, 2, 3))]
H3_RAGGED_SETS = [dict(attn_h3_ks=ks, attn_h3_ragged_xcd=xcd) for ks, xcd in itertools.product((0, 1, 2), (0, 1))] + \
    [dict(attn_h3_ks=1, attn_h3_qg=2)]
F32_RAGGED_SETS = [dict(attn_x6=0), dict(attn_x6=1), dict(attn_x6=0, attn_cfg=1)]


def _cases():
    out = []
    for kernel, sets in (("h3", H3_SETS), ("f32", F32_SETS)):
        for (B, T, heads), opts in itertools.product(SHAPES, sets):
            out.append(dict(kernel=kernel, shape=(B, T, heads), pack=None, options=opts))
    for kernel, sets in (("h3", H3_RAGGED_SETS), ("f32", F32_RAGGED_SETS)):
        for pack, opts in itertools.product(PACKS, sets):
            out.append(dict(kernel=kernel, shape=None, pack=pack, options=opts))
    for c in out:
        what = c["pack"] or "b{}_t{}_h{}".format(*c["shape"])
        c["name"] = "/".join([c["kernel"], what] + [f"{a}={b}" for a, b in c["options"].items()])
    assert len({c["name"] for c in out}) == len(out)
    return out


CASES = _cases()


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _uniform_qkv(B, T, heads):
    D = heads * 64
    qkv = torch.randn(B, T, 3 * D, generator=torch.Generator().manual_seed(B * T + heads)) * 1.5
    qkv[0, 3, :D] *= 6.0
    qkv[0, T - 2, D:2 * D] *= 6.0
    qkv[:, ::7] *= 0.05
    qkv[:, 5, 2 * D:] *= 40.0
    if T > 64:
        qkv[0, 32:64, 2 * D:] = 0.0
    return qkv


def _image_qkv(T, heads, seed):
    D = heads * 64
    qkv = torch.randn(T, 3 * D, generator=torch.Generator().manual_seed(seed)) * 1.5
    qkv[min(3, T - 1), :D] *= 6.0
    qkv[max(T - 2, 0), D:2 * D] *= 6.0
    qkv[::7] *= 0.05
    qkv[min(5, T - 1), 2 * D:] *= 40.0
    return qkv


def _run(c, dev):
    """-> {name: tensor} of the call's outputs"""
    from anyloc_amd import _lib, ops
    lib = _lib.load()
    if c["pack"] is None:
        B, T, heads = c["shape"]
        qkv = _uniform_qkv(B, T, heads).to(dev)
        if c["kernel"] == "f32":
            return {"out": ops.attention(qkv, heads)}
        D, rows = heads * 64, B * T                 # (zeroed buffers: the image's size is rounded up past what the kernel writes)
        img = torch.zeros(lib.anyloc_h2_bytes(rows, D), dtype=torch.uint8, device=dev)
        inv = torch.zeros(rows, dtype=torch.float32, device=dev)
        ws = _lib.workspace(lib.anyloc_attention_h3_workspace_bytes(B, T, heads), dev, "attn_h3")
        _lib.check(lib.anyloc_attention_h3(_lib.ptr(qkv), _lib.ptr(img), _lib.ptr(inv), B, T, D, heads, _lib.ptr(ws), ws.numel(),
                                           _lib.stream_ptr()), "anyloc_attention_h3")
        return {"out": img, "out_inv": inv}
    tokens, heads = PACKS[c["pack"]], HEADS_RAGGED
    D, rows = heads * 64, sum(tokens)
    x = torch.cat([_image_qkv(t, heads, 100 + i) for i, t in enumerate(tokens)]).to(dev).contiguous()
    off = torch.zeros(len(tokens) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(tokens), 0)
    off_d = off.to(dev)
    tok = (C.c_int32 * len(tokens))(*tokens)
    if c["kernel"] == "h3":
        img = torch.zeros(lib.anyloc_h2_bytes(rows, D), dtype=torch.uint8, device=dev)
        inv = torch.zeros(rows, dtype=torch.float32, device=dev)
        ws = _lib.workspace(lib.anyloc_attention_h3_workspace_bytes(1, rows, heads), dev, "attn_h3")
        _lib.check(lib.anyloc_attention_h3_ragged(_lib.ptr(x), _lib.ptr(img), _lib.ptr(inv), len(tokens), tok, _lib.ptr(off_d), D,
                                                  heads, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "anyloc_attention_h3_ragged")
        return {"out": img, "out_inv": inv}
    y = torch.zeros(rows, D, dtype=torch.float32, device=dev)
    _lib.check(lib.anyloc_attention_ragged(_lib.ptr(x), _lib.ptr(y), len(tokens), tok, _lib.ptr(off_d), D, heads, _lib.stream_ptr()),
               "anyloc_attention_ragged")
    return {"out": y}


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
            outs = _run(c, dev)
            torch.cuda.synchronize()
            prof = ops.profile_dump().get("attention", {})
        print(json.dumps({"case": c["name"], "sha256": {k: _sha(v) for k, v in outs.items()},
                          "attention": {k: prof.get(k) for k in ("calls", "flops", "bytes")}}), flush=True)


if __name__ == "__main__":
    main()
