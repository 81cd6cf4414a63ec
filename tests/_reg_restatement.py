"""Restatement of DINOv2 with registers (hub ``dinov2_vit*14_reg``: ``num_register_tokens=4``,
``interpolate_antialias=True``, ``interpolate_offset=0.0``) on top of the plain restated model of
``oracle/dinov2_ref.py``, for the register tests.  ``oracle/`` stays as it is: the model is built for the base
architecture, loaded without ``register_tokens``, and given a local ``prepare_tokens`` -- patch embedding, CLS, the
antialiased size-driven positional table, then the registers inserted after CLS (no positional term), as
``prepare_tokens_with_masks`` does.  The tap is the one of ``extract_facet`` minus the register rows."""
import math

import torch
from torch.nn import functional as F

from anyloc_amd import synth
from oracle import dinov2_ref


def pos_table_reg(pos_embed, h_img, w_img):
    """[1, 1+M*M, D] -> [1, 1+(h/14)*(w/14), D]: bicubic, antialias, output size (h/14, w/14), no offset; skipped for
    the native square grid.  Computed in the table's own dtype."""
    n_tab = pos_embed.shape[1] - 1
    gh, gw = h_img // 14, w_img // 14
    if gh * gw == n_tab and h_img == w_img:
        return pos_embed
    m = int(math.sqrt(n_tab))
    dim = pos_embed.shape[-1]
    grid = pos_embed[:, 1:].reshape(1, m, m, dim).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, size=(gh, gw), mode="bicubic", align_corners=False, antialias=True)
    grid = grid.permute(0, 2, 3, 1).reshape(1, gh * gw, dim)
    return torch.cat([pos_embed[:, :1], grid], dim=1)


def build(name, sd, depth, dtype=torch.float32):
    """The restated ``name`` (a ``_reg`` model) with ``depth`` blocks in ``dtype``."""
    model = dinov2_ref.DinoVisionTransformer(synth.base_model(name))
    model.blocks = model.blocks[:depth]
    model.load_state_dict({k: v for k, v in sd.items() if k != "register_tokens"}, strict=True)
    model.register_tokens = torch.nn.Parameter(sd["register_tokens"].detach().clone().cpu())
    model = model.eval().to(dtype)

    def prepare_tokens(img):
        B, _, H, W = img.shape
        x = model.patch_embed(img)
        x = torch.cat([model.cls_token.expand(B, -1, -1), x], dim=1)
        x = x + pos_table_reg(model.pos_embed, H, W)
        return torch.cat([x[:, :1], model.register_tokens.expand(B, -1, -1), x[:, 1:]], dim=1)

    model.prepare_tokens = prepare_tokens
    return model


@torch.no_grad()
def hooked(model, img, layers):
    """One forward of ``img`` [B,3,H,W] -> {(layer, "qkv" | "token"): the hooked tensor, every token row}."""
    grabbed, handles = {}, []
    for l in set(layers):
        handles.append(model.blocks[l].attn.qkv.register_forward_hook(
            lambda m, i, o, l=l: grabbed.__setitem__((l, "qkv"), o)))
        handles.append(model.blocks[l].register_forward_hook(lambda m, i, o, l=l: grabbed.__setitem__((l, "token"), o)))
    try:
        model(img)
    finally:
        for h in handles:
            h.remove()
    return grabbed


def tap(raw, layer, facet, n_reg, use_cls=False, norm=True):
    """The tap of ``extract_facet`` on the output of :func:`hooked`, minus the register rows: [B, N(+1), D]."""
    res = raw[(layer, "token" if facet == "token" else "qkv")]
    res = torch.cat([res[:, :1], res[:, 1 + n_reg:]], dim=1) if use_cls else res[:, 1 + n_reg:]
    if facet != "token":
        d = res.shape[2] // 3
        j = ("query", "key", "value").index(facet)
        res = res[:, :, j * d:(j + 1) * d]
    return F.normalize(res, dim=-1) if norm else res
