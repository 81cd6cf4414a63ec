"""Restatement of the DINOv3 ViT (``dinov3_vit*16``) in plain torch, in any dtype, from a state dict in the project's
key layout (``anyloc_amd.synth.synthetic_state_dict`` / ``anyloc_amd.weights.from_hf_dinov3``).  It is the oracle of the GPU
tests (``transformers`` may be absent there); ``tests/test_dinov3_cpu.py`` holds it against ``transformers``'
``DINOv3ViTModel`` in float64.

The model: token rows [CLS, reg_0 .. reg_{R-1}, patches] with no positional term; per block LN (eps 1e-5), q | k | v,
rotation of q and k of the PATCH rows by the 2-D rotary table, softmax((q k^T) / 8) v, proj, LayerScale, LN, mlp (exact GELU,
or silu(gate) * up), LayerScale.  The table is computed in float32 whatever the model's dtype (as the original does) and
cast.  Hooks: the q | k | v projections' outputs -- BEFORE the rotation -- and the block outputs."""
import math

import torch
from torch.nn import functional as F

PATCH = 16
EPS = 1e-5
THETA = 100.0
HEAD = 64


def rope_cos_sin(gh, gw, dtype):
    """cos, sin [gh * gw, 64] of the patch grid: centres ((i + .5) / gh, (j + .5) / gw) mapped to [-1, 1] in (y, x) order,
    16 frequencies theta^-(k / 16) each, angles = 2 pi coord freq, the 32 angles tiled twice over the head."""
    freq = 1.0 / THETA ** (torch.arange(0, HEAD // 4, dtype=torch.float32) * (4.0 / HEAD))
    ys = (torch.arange(gh, dtype=torch.float32) + 0.5) / gh
    xs = (torch.arange(gw, dtype=torch.float32) + 0.5) / gw
    yy, xx = torch.meshgrid(ys, xs, indexing="ij")
    coords = 2.0 * torch.stack([yy.reshape(-1), xx.reshape(-1)], dim=1) - 1.0          # [N, (y, x)]
    ang = (2 * math.pi * coords[:, :, None] * freq[None, None, :]).reshape(gh * gw, HEAD // 2)
    ang = torch.cat([ang, ang], dim=1)
    return torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)


def _rotate(x, cos, sin, prefix):
    """x [B, heads, T, 64]: rows >= prefix rotated, x' = x cos + rotate_half(x) sin."""
    pre, pat = x[:, :, :prefix], x[:, :, prefix:]
    half = torch.cat([-pat[..., HEAD // 2:], pat[..., :HEAD // 2]], dim=-1)
    return torch.cat([pre, pat * cos + half * sin], dim=2)


class Model:
    def __init__(self, sd, depth=None, dtype=torch.float32):
        have = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
        self.depth = have if depth is None else min(depth, have)
        self.dtype = dtype
        self.sd = {k: v.detach().to("cpu", dtype) for k, v in sd.items()}
        self.dim = self.sd["cls_token"].shape[-1]
        self.heads = self.dim // HEAD
        self.R = self.sd["register_tokens"].shape[1]
        self.gated = "blocks.0.mlp.w12.weight" in self.sd

    @torch.no_grad()
    def hooked(self, img, layers):
        """img [B, 3, H, W] -> {(layer, "qkv"): [B, T, 3D] (pre-rotation), (layer, "token"): [B, T, D]}, every token row."""
        sd, D, nh, R = self.sd, self.dim, self.heads, self.R
        img = img.to(self.dtype)
        B, _, H, W = img.shape
        gh, gw = H // PATCH, W // PATCH
        x = F.conv2d(img, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=PATCH).flatten(2).transpose(1, 2)
        x = torch.cat([sd["cls_token"].reshape(1, 1, D).expand(B, -1, -1), sd["register_tokens"].reshape(1, R, D).expand(B, -1, -1),
                       x], dim=1)
        cos, sin = rope_cos_sin(gh, gw, self.dtype)
        T = x.shape[1]
        grabbed = {}
        for l in range(min(self.depth, max(layers) + 1)):
            p = f"blocks.{l}."
            y = F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], EPS)
            qkv = F.linear(y, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"])
            if l in layers:
                grabbed[(l, "qkv")] = qkv
            q, k, v = (t.reshape(B, T, nh, HEAD).transpose(1, 2) for t in qkv.split(D, dim=-1))
            q, k = _rotate(q, cos, sin, 1 + R), _rotate(k, cos, sin, 1 + R)
            a = torch.softmax((q @ k.transpose(-1, -2)) * HEAD ** -0.5, dim=-1) @ v
            a = a.transpose(1, 2).reshape(B, T, D)
            x = x + sd[p + "ls1.gamma"] * F.linear(a, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
            y = F.layer_norm(x, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], EPS)
            if self.gated:
                g, u = F.linear(y, sd[p + "mlp.w12.weight"], sd[p + "mlp.w12.bias"]).chunk(2, dim=-1)
                m = F.linear(F.silu(g) * u, sd[p + "mlp.w3.weight"], sd[p + "mlp.w3.bias"])
            else:
                m = F.linear(F.gelu(F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])),
                             sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
            x = x + sd[p + "ls2.gamma"] * m
            if l in layers:
                grabbed[(l, "token")] = x
        return grabbed


def tap(raw, layer, facet, n_reg, use_cls=False, norm=True):
    """The extractor's tap on the output of ``Model.hooked``: the patch rows (CLS first with ``use_cls``), never a register
    row: [B, N(+1), D]."""
    res = raw[(layer, "token" if facet == "token" else "qkv")]
    res = torch.cat([res[:, :1], res[:, 1 + n_reg:]], dim=1) if use_cls else res[:, 1 + n_reg:]
    if facet != "token":
        d = res.shape[2] // 3
        j = ("query", "key", "value").index(facet)
        res = res[:, :, j * d:(j + 1) * d]
    return F.normalize(res, dim=-1) if norm else res
