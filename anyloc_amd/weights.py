"""Where DINOv2 weights come from.

The reference calls ``torch.hub.load('facebookresearch/dinov2', name)``
(``utilities.py:239-240``), which downloads code and a checkpoint.  This
implementation needs only the *state dict* (hub key names).  Resolution order:

1. a state dict registered in-process with :func:`register_state_dict`
   (tests / benchmarks inject seeded synthetic weights this way);
2. ``$ANYLOC_DINOV2_WEIGHTS`` -- a ``.pth`` file, or a directory holding
   ``<name>_pretrain.pth`` (the file names facebookresearch publishes;
   ``<base>_reg4_pretrain.pth`` for a ``<base>_reg`` model with registers);
3. the torch hub checkpoint cache (``torch.hub.get_dir()/checkpoints``), where
   a previous ``torch.hub.load`` of the real model would have left it;
4. ``$ANYLOC_SYNTHETIC_WEIGHTS=<seed>`` -- seeded random weights (explicit opt-in);
5. download with ``torch.hub.load_state_dict_from_url`` (needs network).
"""
import os

import torch

from .synth import ARCH, UNSERVED, base_model, is_rope, n_registers, synthetic_state_dict

_REGISTERED = {}
_URL = "https://dl.fbaipublicfiles.com/dinov2/{short}/{fname}"
# DINOv3 checkpoints are handed out per request (no public URL to fetch from): a file placed by hand is used.  Neither
# these file names nor the upstream hub's own state-dict key names could be checked offline -- UNVERIFIED; the two layouts
# read are this project's (synth.synthetic_state_dict) and the transformers one (from_hf_dinov3).
_V3_FILE = "{name}_pretrain.pth"


def checkpoint_name(name):
    """The published checkpoint file of a hub model: ``dinov2_vits14_pretrain.pth``, ``dinov2_vits14_reg4_pretrain.pth``."""
    if is_rope(name):
        return _V3_FILE.format(name=name)
    r = n_registers(name)
    return f"{base_model(name)}_reg{r}_pretrain.pth" if r else f"{name}_pretrain.pth"


def register_state_dict(name, state_dict):
    _REGISTERED[name] = state_dict


def unregister_state_dict(name=None):
    if name is None:
        _REGISTERED.clear()
    else:
        _REGISTERED.pop(name, None)


def from_hf_dinov3(state_dict):
    """The state dict of a transformers ``DINOv3ViTModel`` (``embeddings.{cls_token, register_tokens, patch_embeddings.*}``,
    ``model.layer.N.{norm1, attention.{q,k,v,o}_proj, layer_scale{1,2}.lambda1, norm2, mlp.{up,down,gate}_proj}``; an outer
    ``model.`` / ``backbone.`` prefix of a wrapping module is dropped) in this project's layout: q / k / v stacked into
    ``attn.qkv`` with a zero bias for a projection that has none (k), gate / up stacked into ``mlp.w12`` ([gates; values]),
    up / down as ``mlp.fc1`` / ``mlp.fc2`` without a gate."""
    sd = dict(state_dict)
    for prefix in ("backbone.", "model.", "dinov3."):
        if not any(k.startswith("embeddings.") for k in sd) and any(k.startswith(prefix + "embeddings.") for k in sd):
            sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    layer = "model.layer." if any(k.startswith("model.layer.") for k in sd) else "layer."
    out = {"cls_token": sd["embeddings.cls_token"], "register_tokens": sd["embeddings.register_tokens"],
           "patch_embed.proj.weight": sd["embeddings.patch_embeddings.weight"],
           "patch_embed.proj.bias": sd["embeddings.patch_embeddings.bias"]}
    if "embeddings.mask_token" in sd:
        out["mask_token"] = sd["embeddings.mask_token"].reshape(1, -1)
    for k in ("norm.weight", "norm.bias"):
        if k in sd:
            out[k] = sd[k]
    depth = 1 + max(int(k[len(layer):].split(".")[0]) for k in sd if k.startswith(layer))
    for i in range(depth):
        s, p = f"{layer}{i}.", f"blocks.{i}."
        ws = [sd[s + f"attention.{n}_proj.weight"] for n in "qkv"]
        bs = [sd.get(s + f"attention.{n}_proj.bias", torch.zeros_like(w[:, 0])) for n, w in zip("qkv", ws)]
        out[p + "attn.qkv.weight"], out[p + "attn.qkv.bias"] = torch.cat(ws), torch.cat(bs)
        out[p + "attn.proj.weight"], out[p + "attn.proj.bias"] = sd[s + "attention.o_proj.weight"], sd[s + "attention.o_proj.bias"]
        for n in ("norm1", "norm2"):
            out[p + n + ".weight"], out[p + n + ".bias"] = sd[s + n + ".weight"], sd[s + n + ".bias"]
        out[p + "ls1.gamma"], out[p + "ls2.gamma"] = sd[s + "layer_scale1.lambda1"], sd[s + "layer_scale2.lambda1"]
        lin = lambda n: (sd[s + f"mlp.{n}_proj.weight"],
                         sd.get(s + f"mlp.{n}_proj.bias", torch.zeros_like(sd[s + f"mlp.{n}_proj.weight"][:, 0])))
        (up_w, up_b), (down_w, down_b) = lin("up"), lin("down")
        if s + "mlp.gate_proj.weight" in sd:
            gate_w, gate_b = lin("gate")
            out[p + "mlp.w12.weight"], out[p + "mlp.w12.bias"] = torch.cat([gate_w, up_w]), torch.cat([gate_b, up_b])
            out[p + "mlp.w3.weight"], out[p + "mlp.w3.bias"] = down_w, down_b
        else:
            out[p + "mlp.fc1.weight"], out[p + "mlp.fc1.bias"] = up_w, up_b
            out[p + "mlp.fc2.weight"], out[p + "mlp.fc2.bias"] = down_w, down_b
    return out


def _project_layout(name, sd):
    """A loaded checkpoint in this project's key layout (a DINOv3 checkpoint may come in the transformers layout)."""
    if is_rope(name) and not any(k.startswith("blocks.") for k in sd) and any("embeddings.patch_embeddings" in k for k in sd):
        return from_hf_dinov3(sd)
    return sd


def resolve_state_dict(name):
    if name in UNSERVED:
        raise NotImplementedError(f"{name} is not served: {UNSERVED[name]}")
    if name not in ARCH:
        raise ValueError(f"unknown DINOv2 model {name!r}; expected one of {sorted(ARCH)}")
    if name in _REGISTERED:
        return _project_layout(name, _REGISTERED[name])
    fname = checkpoint_name(name)
    cands = []
    env = os.environ.get("ANYLOC_DINOV2_WEIGHTS")
    if env:
        cands.append(env if os.path.isfile(env) else os.path.join(env, fname))
    cands.append(os.path.join(torch.hub.get_dir(), "checkpoints", fname))
    for c in cands:
        if os.path.isfile(c):
            return _project_layout(name, torch.load(c, map_location="cpu"))
    seed = os.environ.get("ANYLOC_SYNTHETIC_WEIGHTS")
    if seed is not None:
        print(f"[anyloc_amd] using SYNTHETIC {name} weights (seed {seed})")
        return synthetic_state_dict(name, int(seed))
    try:
        if is_rope(name):
            raise RuntimeError("DINOv3 checkpoints have no public download URL")
        return torch.hub.load_state_dict_from_url(_URL.format(short=base_model(name), fname=fname), map_location="cpu")
    except Exception as exc:   # no network
        raise FileNotFoundError(
            f"no weights for {name}: set ANYLOC_DINOV2_WEIGHTS to a checkpoint / directory, place "
            f"{fname} in {os.path.join(torch.hub.get_dir(), 'checkpoints')}, or opt in to random "
            f"weights with ANYLOC_SYNTHETIC_WEIGHTS=<seed> (download failed: {exc})") from exc
