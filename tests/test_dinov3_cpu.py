"""DINOv3 (``dinov3_vit*16``) on a GPU-less host: the restatement the GPU tests compare against agrees with
``transformers``' ``DINOv3ViTModel`` in float64; the product's rotation table is HF's, bit for bit; ``from_hf_dinov3`` gives
the project's key layout; the names, the row layout for patch 16 with four registers, the size checks and the new C entry
points are as documented; the synthetic dicts of the earlier names are what they were."""
import ctypes as C
import hashlib
import os
import re
import sys

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from anyloc_amd import synth, weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dinov3_restatement as v3ref  # noqa: E402

V3_NAMES = ("dinov3_vits16", "dinov3_vits16plus", "dinov3_vitb16", "dinov3_vitl16", "dinov3_vith16plus")


# ---------------------------------------------------------------- the restatement against transformers ----

def _hf_model(gated, seed, depth=3):
    """A 3-block DINOv3ViTModel at D = 384 / 6 heads / 4 registers with every parameter drawn at random."""
    transformers = pytest.importorskip("transformers")
    cfg = transformers.DINOv3ViTConfig(hidden_size=384, num_attention_heads=6, num_hidden_layers=depth, intermediate_size=1536,
                                       num_register_tokens=4, use_gated_mlp=gated, hidden_act="silu" if gated else "gelu",
                                       attn_implementation="eager")
    assert cfg.patch_size == 16 and cfg.layer_norm_eps == 1e-5 and cfg.rope_theta == 100.0
    assert cfg.key_bias is False and cfg.query_bias and cfg.value_bias and cfg.proj_bias and cfg.mlp_bias
    hf = transformers.DINOv3ViTModel(cfg).eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in hf.named_parameters():
            if "norm" in k and k.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif "lambda1" in k:
                p.copy_(0.3 + 0.2 * torch.rand(p.shape, generator=g))
            elif p.ndim >= 2 and "token" not in k:
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 / p[0].numel() ** 0.5))
            else:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    return hf


def _hf_hooked(hf, img, layer):
    grabbed = {}
    att = hf.model.layer[layer].attention if hasattr(hf, "model") else hf.layer[layer].attention
    blk = hf.model.layer[layer] if hasattr(hf, "model") else hf.layer[layer]
    hs = [att.q_proj.register_forward_hook(lambda m, i, o: grabbed.__setitem__("query", o)),
          att.k_proj.register_forward_hook(lambda m, i, o: grabbed.__setitem__("key", o)),
          att.v_proj.register_forward_hook(lambda m, i, o: grabbed.__setitem__("value", o)),
          blk.register_forward_hook(lambda m, i, o: grabbed.__setitem__("token", o[0] if isinstance(o, tuple) else o))]
    try:
        with torch.no_grad():
            hf(pixel_values=img)
    finally:
        for h in hs:
            h.remove()
    return grabbed


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("hw", [(48, 80), (80, 48)])
def test_restatement_matches_hf(gated, hw):
    """q / k / v (outputs of the projections, before the rotation) and the block output of layer 2, patch rows as unit
    rows, float64 on both sides, at two non-square sizes -- a swapped (y, x) order would pass a square one."""
    hf = _hf_model(gated, 7 + gated).double()
    # the model computes its angles in float32 whatever its dtype ("Force float32" in DINOv3ViTRopePositionEmbedding.forward);
    # .double() also casts the inv_freq BUFFER, which would silently move that product to float64: keep the buffer float32
    hf.rope_embeddings.inv_freq = hf.rope_embeddings.inv_freq.float()
    sd = weights.from_hf_dinov3(hf.state_dict())
    ours = v3ref.Model(sd, 3, torch.float64)
    assert ours.R == 4 and ours.gated == gated
    img = torch.randn(2, 3, *hw, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    want = _hf_hooked(hf, img, 2)
    raw = ours.hooked(img, [2])
    n = (hw[0] // 16) * (hw[1] // 16)
    for facet in ("query", "key", "value", "token"):
        got = v3ref.tap(raw, 2, facet, 4)
        ref = F.normalize(want[facet][:, 5:], dim=-1)
        assert got.shape == ref.shape == (2, n, 384)
        err = float((got - ref).abs().max())
        print(f"gated={gated} {hw} {facet}: max-abs {err:.2e}")
        assert err <= 1e-10, (facet, err)
    # the rotation matters at this size: without it the layer-2 tokens are far away
    cls_got = v3ref.tap(raw, 2, "token", 4, use_cls=True)[:, 0]
    assert float((cls_got - F.normalize(want["token"][:, 0], dim=-1)).abs().max()) <= 1e-10


@pytest.mark.parametrize("hw", [(16, 16), (48, 80), (80, 48), (224, 224)])
def test_rope_table_is_hfs(hw):
    from anyloc_amd.extractor import rope_table
    hf = _hf_model(False, 3, depth=1)
    with torch.no_grad():
        cos, sin = hf.rope_embeddings(torch.zeros(1, 3, *hw))
    got = rope_table(*hw)
    n = (hw[0] // 16) * (hw[1] // 16)
    assert got.shape == (n, 64) and got.dtype == torch.float32 and cos.shape == (n, 64)
    assert torch.equal(got[:, :32], cos[:, :32]) and torch.equal(got[:, :32], cos[:, 32:])
    assert torch.equal(got[:, 32:], sin[:, :32]) and torch.equal(got[:, 32:], sin[:, 32:])
    # the restatement's own table is the same numbers
    c2, s2 = v3ref.rope_cos_sin(hw[0] // 16, hw[1] // 16, torch.float32)
    assert torch.equal(c2, cos) and torch.equal(s2, sin)


@pytest.mark.parametrize("gated", [False, True])
def test_from_hf_dinov3_layout(gated):
    hf = _hf_model(gated, 5)
    hsd = hf.state_dict()
    sd = weights.from_hf_dinov3(hsd)
    name = "dinov3_vits16plus" if gated else "dinov3_vits16"
    want = synth.synthetic_state_dict(name, 0, depth=3)
    for k, v in want.items():
        if k == "mask_token":
            continue
        assert k in sd, k
        assert tuple(sd[k].shape) == tuple(v.shape), (k, sd[k].shape, v.shape)
    assert not [k for k in sd if k not in want]
    assert "pos_embed" not in sd
    for i in range(3):
        b = sd[f"blocks.{i}.attn.qkv.bias"]
        assert torch.count_nonzero(b[384:768]) == 0 and torch.count_nonzero(b[:384]) > 0 and torch.count_nonzero(b[768:]) > 0
        layer = f"model.layer.{i}." if f"model.layer.{i}.norm1.weight" in hsd else f"layer.{i}."
        assert torch.equal(sd[f"blocks.{i}.attn.qkv.weight"][384:768], hsd[layer + "attention.k_proj.weight"])
        if gated:
            # [gates; values]: the order the SwiGLU loader of the extractor splits at `hidden`
            w12 = sd[f"blocks.{i}.mlp.w12.weight"]
            assert torch.equal(w12[:1536], hsd[layer + "mlp.gate_proj.weight"]) and torch.equal(w12[1536:], hsd[layer + "mlp.up_proj.weight"])
            assert torch.equal(sd[f"blocks.{i}.mlp.w3.weight"], hsd[layer + "mlp.down_proj.weight"])
    # both layouts resolve for a registered name
    weights.register_state_dict(name, hsd)
    try:
        got = weights.resolve_state_dict(name)
        assert "blocks.0.attn.qkv.weight" in got
    finally:
        weights.unregister_state_dict(name)


# ---------------------------------------------------------------- names and host logic ----

def test_names_resolve_and_7b_is_refused():
    import utilities
    from anyloc_amd import extractor
    for name in V3_NAMES:
        assert name in extractor._DINO_V3_MODELS and name in extractor._DINO_MODELS and name in utilities._DINO_MODELS
        dim, depth, heads, ffn, hidden = synth.ARCH[name]
        assert dim == heads * 64 and synth.n_registers(name) == 4 and synth.patch_size(name) == 16
        assert synth.is_rope(name) and synth.ln_eps(name) == 1e-5 and synth.base_model(name) == name
        assert weights.checkpoint_name(name).startswith(name)
    assert synth.ARCH["dinov3_vith16plus"] == (1280, 32, 20, "swiglu", 5120)
    assert synth.ARCH["dinov3_vits16plus"][3] == "swiglu" and synth.ARCH["dinov3_vitl16"] == (1024, 24, 16, "mlp", 4096)
    for name in ("dinov2_vits14", "dinov2_vitg14_reg"):
        assert not synth.is_rope(name) and synth.patch_size(name) == 14 and synth.ln_eps(name) == 1e-6
    with pytest.raises(NotImplementedError):
        utilities.DinoV2ExtractFeatures("dinov3_vit7b16", 2, "value")
    with pytest.raises(NotImplementedError):
        extractor.hub_load("facebookresearch/dinov3", "dinov3_vit7b16")
    with pytest.raises(NotImplementedError):
        weights.resolve_state_dict("dinov3_vit7b16")
    with pytest.raises(RuntimeError):
        extractor.hub_load("facebookresearch/dinov2", "dinov3_vits16")      # the wrong repository for the name


def test_synthetic_v3_layout():
    for name in ("dinov3_vits16", "dinov3_vits16plus"):
        sd = synth.synthetic_state_dict(name, 3, depth=2)
        assert "pos_embed" not in sd and sd["register_tokens"].shape == (1, 4, 384)
        assert sd["patch_embed.proj.weight"].shape == (384, 3, 16, 16)
        b = sd["blocks.1.attn.qkv.bias"]
        assert torch.count_nonzero(b[384:768]) == 0 and torch.count_nonzero(b[:384]) > 300
        assert ("blocks.0.mlp.w12.weight" in sd) == (name == "dinov3_vits16plus")
        again = synth.synthetic_state_dict(name, 3, depth=2)
        assert all(torch.equal(sd[k], again[k]) for k in sd)


def test_earlier_names_keep_their_synthetic_dicts():
    """Hashes taken before DINOv3 was added: the earlier names draw the same numbers for the same seed."""
    def digest(name, seed, keys):
        sd = synth.synthetic_state_dict(name, seed, depth=1)
        h = hashlib.sha256()
        for k in keys:
            h.update(sd[k].numpy().tobytes())
        return h.hexdigest()[:16]
    keys = ("cls_token", "pos_embed", "blocks.0.attn.qkv.weight", "blocks.0.ls2.gamma", "norm.bias")
    assert digest("dinov2_vits14", 0, keys) == EARLIER["dinov2_vits14"]
    assert digest("dinov2_vitg14", 4, keys + ("blocks.0.mlp.w12.bias",)) == EARLIER["dinov2_vitg14"]
    assert digest("dinov2_vitb14_reg", 2, keys + ("register_tokens",)) == EARLIER["dinov2_vitb14_reg"]


EARLIER = {"dinov2_vits14": "001ae13271c8e641", "dinov2_vitg14": "b8944f0999e31d08", "dinov2_vitb14_reg": "e5eea8b00ff5f574"}


def test_ragged_layout_patch_16_four_registers():
    from anyloc_amd.extractor import ragged_chunks, ragged_offsets
    sizes = [(48, 80), (80, 48), (112, 160), (16, 16), (48, 80)]
    N = np.array([15, 15, 70, 1, 15])
    tok, out, pix = ragged_offsets(sizes, use_cls=False, patch=16, registers=4)
    i = np.arange(len(sizes) + 1)
    assert tok.tolist() == [0] + np.cumsum(N + 5).tolist()
    assert out.tolist() == [0] + np.cumsum(N).tolist() == (tok - 5 * i).tolist()
    assert pix.tolist() == [0] + np.cumsum([3 * h * w for h, w in sizes]).tolist()
    tok_c, out_c, _ = ragged_offsets(sizes, use_cls=True, patch=16, registers=4)
    assert tok_c.tolist() == tok.tolist() and out_c.tolist() == (tok - 4 * i).tolist()
    assert ragged_chunks(sizes, 40, patch=16, registers=4) == [(0, 2), (2, 3), (3, 5)]
    assert ragged_chunks(sizes, 10 ** 6, patch=16, registers=4) == [(0, 5)]


# ---------------------------------------------------------------- the C entry points ----

@pytest.fixture(scope="module")
def lib():
    from anyloc_amd import _lib, build
    build.build_library(verbose=False)
    return _lib.load()


@pytest.fixture()
def handle(lib):
    """A ViT-S/16 geometry handle with placeholder (never dereferenced) pointers: nothing here touches a device."""
    from anyloc_amd import _lib
    cfg = _lib.VitConfig(384, 2, 6, 0, 1536, 16, 768)
    blocks = (_lib.VitBlockWeights * 2)()
    for i in range(2):
        for f in _lib.BLOCK_FIELDS:
            setattr(blocks[i], f, 4096)
    h = C.c_void_p()
    assert lib.anyloc_vit_create(C.byref(h), C.byref(cfg), 4096, 4096, 4096, blocks) == 0
    assert lib.anyloc_vit_set_registers(h, 4096, 4) == 0
    yield h
    lib.anyloc_vit_destroy(h)


def test_new_entries_declared_bound_exported(lib):
    from anyloc_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "anyloc_hip.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("anyloc_vit_set_rope", "anyloc_vit_set_ln_eps", "anyloc_rope_rows"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES and hasattr(raw, name), name
    assert lib.anyloc_version() == _lib.ABI_VERSION            # additive: the number stays


def test_setters_validate(lib, handle):
    assert lib.anyloc_vit_set_rope(None, 1) == -1 and b"null handle" in lib.anyloc_last_error()
    assert lib.anyloc_vit_set_ln_eps(None, 1e-5) == -1
    for bad in (0.0, -1e-5, 1.0, float("nan")):
        assert lib.anyloc_vit_set_ln_eps(handle, bad) == -1 and b"eps" in lib.anyloc_last_error()
    assert lib.anyloc_vit_set_ln_eps(handle, 1e-5) == 0 and lib.anyloc_vit_set_rope(handle, 1) == 0
    assert lib.anyloc_vit_set_rope(handle, 0) == 0
    assert lib.anyloc_rope_rows(None, 60, 6, 4096, 20, 5, None, 0, None) == -1
    assert lib.anyloc_rope_rows(4096, 61, 6, 4096, 20, 5, None, 0, None) == -1        # rows % tokens
    assert lib.anyloc_rope_rows(4096, 60, 6, 4096, 5, 5, None, 0, None) == -1         # no patch rows
    assert lib.anyloc_rope_rows(4096, 60, 6, 4096, 0, 5, 4096, 0, None) == -1         # ragged without images


def test_sizes_must_be_multiples_of_16(lib, handle):
    """The C entry points refuse a size that is no multiple of the model's patch before any device work; the workspace for
    patch 16 counts (H / 16)(W / 16) + 5 rows per image."""
    taps = (C.c_int32 * 1)(1)
    facets = (C.c_int32 * 1)(3)
    assert lib.anyloc_vit_set_rope(handle, 1) == 0
    for hw in ((224, 230), (14, 28), (230, 224), (8, 16)):
        assert lib.anyloc_vit_forward(handle, 4096, 1, hw[0], hw[1], 4096, 1, taps, facets, 0, 4096, 4096, 1 << 30, None) == -1
        assert b"multiple of the patch size 16" in lib.anyloc_last_error()
        sizes = (C.c_int32 * 4)(48, 80, *hw)
        assert lib.anyloc_vit_forward_ragged(handle, 4096, 2, sizes, 4096, 4096, 1, taps, facets, 0, 4096, 4096, 1 << 30, None) == -1
        assert b"patch size 16" in lib.anyloc_last_error()
    uni = lib.anyloc_vit_workspace_bytes(handle, 2, 48, 80)
    rag = lib.anyloc_vit_workspace_bytes_ragged(handle, 2, (C.c_int32 * 4)(48, 80, 48, 80))
    assert uni == rag > 2 * 20 * 4 * (384 + 384 + 1536)
    # the Python host refuses them too
    from anyloc_amd.extractor import ragged_offsets
    tok, _, _ = ragged_offsets([(48, 80)], False, patch=16, registers=4)
    assert tok.tolist() == [0, 20]
