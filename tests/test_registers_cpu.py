"""DINOv2 with registers (``dinov2_vit*14_reg``) on a GPU-less host: the float64 restatement the GPU tests compare
against agrees with ``transformers``' ``Dinov2WithRegistersModel``; the product's positional table is HF's; the new C entry
point is declared, bound, exported and validates its arguments before any device work; the ragged row layout, the weight
files and the synthetic state dicts of the plain models are as documented."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

from anyloc_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _reg_restatement as regref  # noqa: E402

REG_NAMES = ("dinov2_vits14_reg", "dinov2_vitb14_reg", "dinov2_vitl14_reg", "dinov2_vitg14_reg")


# ---------------------------------------------------------------- the restatement against transformers ----

def _to_hf(sd, depth, swiglu):
    """facebookresearch -> HF key remap (as in test_oracle_dinov2_hf.py) plus the register tokens."""
    out = {"embeddings.cls_token": sd["cls_token"], "embeddings.mask_token": sd["mask_token"],
           "embeddings.register_tokens": sd["register_tokens"],
           "embeddings.position_embeddings": sd["pos_embed"],
           "embeddings.patch_embeddings.projection.weight": sd["patch_embed.proj.weight"],
           "embeddings.patch_embeddings.projection.bias": sd["patch_embed.proj.bias"],
           "layernorm.weight": sd["norm.weight"], "layernorm.bias": sd["norm.bias"]}
    for i in range(depth):
        p, q = f"blocks.{i}.", f"encoder.layer.{i}."
        D = sd[p + "attn.proj.weight"].shape[0]
        for j, name in enumerate(("query", "key", "value")):
            out[q + f"attention.attention.{name}.weight"] = sd[p + "attn.qkv.weight"][j * D:(j + 1) * D]
            out[q + f"attention.attention.{name}.bias"] = sd[p + "attn.qkv.bias"][j * D:(j + 1) * D]
        out[q + "attention.output.dense.weight"] = sd[p + "attn.proj.weight"]
        out[q + "attention.output.dense.bias"] = sd[p + "attn.proj.bias"]
        for n in ("norm1", "norm2"):
            out[q + n + ".weight"], out[q + n + ".bias"] = sd[p + n + ".weight"], sd[p + n + ".bias"]
        out[q + "layer_scale1.lambda1"], out[q + "layer_scale2.lambda1"] = sd[p + "ls1.gamma"], sd[p + "ls2.gamma"]
        if swiglu:
            out[q + "mlp.weights_in.weight"], out[q + "mlp.weights_in.bias"] = sd[p + "mlp.w12.weight"], sd[p + "mlp.w12.bias"]
            out[q + "mlp.weights_out.weight"], out[q + "mlp.weights_out.bias"] = sd[p + "mlp.w3.weight"], sd[p + "mlp.w3.bias"]
        else:
            for f in ("fc1", "fc2"):
                out[q + f"mlp.{f}.weight"], out[q + f"mlp.{f}.bias"] = sd[p + f"mlp.{f}.weight"], sd[p + f"mlp.{f}.bias"]
    return out


def _hf_model(name, sd, depth):
    transformers = pytest.importorskip("transformers")
    dim, _, heads, ffn, _ = synth.ARCH[name]
    cfg = transformers.Dinov2WithRegistersConfig(
        hidden_size=dim, num_hidden_layers=depth, num_attention_heads=heads, mlp_ratio=4, image_size=518, patch_size=14,
        layerscale_value=1.0, use_swiglu_ffn=(ffn == "swiglu"), layer_norm_eps=1e-6, qkv_bias=True, hidden_act="gelu",
        num_register_tokens=synth.n_registers(name), attn_implementation="eager")
    hf = transformers.Dinov2WithRegistersModel(cfg).eval()
    missing, unexpected = hf.load_state_dict(_to_hf(sd, depth, ffn == "swiglu"), strict=False)
    assert not unexpected and all("mask" in m or "pooler" in m for m in missing), (missing, unexpected)
    return hf


@pytest.mark.parametrize("name,depth", [("dinov2_vits14_reg", 2), ("dinov2_vitg14_reg", 1)])
@pytest.mark.parametrize("hw", [(518, 518), (224, 224), (210, 238)])
def test_restatement_matches_hf_with_registers(name, depth, hw):
    """Every hidden state, the final norm and the patch rows of the tap, float64 on both sides: at 518² (no
    interpolation), 224² (downsampling, where the antialias filter matters) and 210x238 (non-square)."""
    sd = synth.synthetic_state_dict(name, 3, depth=depth)
    ours = regref.build(name, sd, depth, torch.float64)
    hf = _hf_model(name, sd, depth).double()
    R = synth.n_registers(name)
    img = torch.randn(2, 3, *hw, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    with torch.no_grad():
        x = ours.prepare_tokens(img)
        hid = [x]
        for blk in ours.blocks:
            x = blk(x)
            hid.append(x)
        y = ours.norm(x)
        ref = hf(pixel_values=img, output_hidden_states=True)
    assert hid[0].shape[1] == 1 + R + (hw[0] // 14) * (hw[1] // 14)
    # (HF interpolates the positional table in float32: its rounding, ~1e-9 here, is the only float32 step)
    for a, b in zip(hid, ref.hidden_states):
        assert a.shape == b.shape
        assert float((a - b).abs().max()) < 1e-6 * max(1.0, float(b.abs().max()))
    assert float((y - ref.last_hidden_state).abs().max()) < 1e-6
    raw = regref.hooked(ours, img, [depth - 1])
    tok = regref.tap(raw, depth - 1, "token", R, norm=False)
    assert torch.allclose(tok, hid[-1][:, 1 + R:], rtol=0, atol=0)
    # HF's patch tokens: sequence_output[:, 1 + R:] (before its final norm: the block output)
    assert float((tok - ref.hidden_states[-1][:, 1 + R:]).abs().max()) < 1e-6 * max(1.0, float(tok.abs().max()))


@pytest.mark.parametrize("hw", [(518, 518), (224, 224), (210, 238), (476, 630), (322, 322)])
def test_product_positional_table_is_hfs(hw):
    """The host table the extractor hands the forward for a _reg model == HF's interpolate_pos_encoding (float32); the plain
    models keep their own (+0.1 offset, no antialias) table, which differs from it whenever it interpolates."""
    from anyloc_amd.extractor import interpolate_pos_embed, interpolate_pos_embed_reg
    name = "dinov2_vits14_reg"
    sd = synth.synthetic_state_dict(name, 5, depth=1)
    hf = _hf_model(name, sd, 1)
    n = (hw[0] // 14) * (hw[1] // 14)
    with torch.no_grad():
        want = hf.embeddings.interpolate_pos_encoding(torch.zeros(1, 1 + n, 384), *hw)[0]
    got = interpolate_pos_embed_reg(sd["pos_embed"], *hw)
    assert got.shape == (1 + n, 384) and got.dtype == torch.float32
    assert torch.equal(got, want)
    plain = interpolate_pos_embed(sd["pos_embed"], *hw)
    assert torch.equal(plain, got) == (hw == (518, 518))


# ---------------------------------------------------------------- the C entry point ----

@pytest.fixture(scope="module")
def lib():
    from anyloc_amd import _lib, build
    build.build_library(verbose=False)
    return _lib.load()


def test_set_registers_declared_bound_exported(lib):
    import re
    from anyloc_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "anyloc_hip.h")).read()
    assert int(re.search(r"#define ANYLOC_ABI_VERSION (\d+)", header).group(1)) == 10
    assert re.search(r"\banyloc_vit_set_registers\s*\(", header)
    assert "anyloc_vit_set_registers" in _lib.SIGNATURES
    assert hasattr(C.CDLL(_lib.LIB_PATH), "anyloc_vit_set_registers")


@pytest.fixture()
def handle(lib):
    """A ViT-S geometry handle with placeholder (never dereferenced) pointers: nothing here touches a device."""
    from anyloc_amd import _lib
    cfg = _lib.VitConfig(384, 2, 6, 0, 1536, 14, 588)
    blocks = (_lib.VitBlockWeights * 2)()
    for i in range(2):
        for f in _lib.BLOCK_FIELDS:
            setattr(blocks[i], f, 4096)
    h = C.c_void_p()
    assert lib.anyloc_vit_create(C.byref(h), C.byref(cfg), 4096, 4096, 4096, blocks) == 0
    yield h
    lib.anyloc_vit_destroy(h)


def _hw(*sizes):
    flat = [v for s in sizes for v in s]
    return (C.c_int32 * len(flat))(*flat)


def test_set_registers_validation(lib, handle):
    plain = lib.anyloc_vit_workspace_bytes(handle, 2, 224, 224)
    assert lib.anyloc_vit_set_registers(None, 4096, 4) == -1
    assert b"null handle" in lib.anyloc_last_error()
    assert lib.anyloc_vit_set_registers(handle, 4096, -1) == -1
    assert b"[0, 16]" in lib.anyloc_last_error()
    assert lib.anyloc_vit_set_registers(handle, 4096, 17) == -1
    assert lib.anyloc_vit_set_registers(handle, None, 4) == -1
    assert b"null register tokens" in lib.anyloc_last_error()
    # a refused call leaves the handle as it was
    assert lib.anyloc_vit_workspace_bytes(handle, 2, 224, 224) == plain
    assert lib.anyloc_vit_set_registers(handle, 4096, 16) == 0
    assert lib.anyloc_vit_set_registers(handle, 4096, 0) == 0
    assert lib.anyloc_vit_workspace_bytes(handle, 2, 224, 224) == plain
    assert lib.anyloc_vit_set_registers(handle, None, 0) == 0
    assert lib.anyloc_vit_workspace_bytes(handle, 2, 224, 224) == plain


def test_workspace_counts_the_register_rows(lib, handle):
    """The workspace grows by the register rows: with R = 4 a 224 x 224 batch needs more than without, and the ragged query
    for equal sizes is the uniform one; R = 0 gives the plain figures back."""
    plain_u = lib.anyloc_vit_workspace_bytes(handle, 3, 224, 224)
    plain_r = lib.anyloc_vit_workspace_bytes_ragged(handle, 2, _hw((224, 224), (210, 238)))
    assert lib.anyloc_vit_set_registers(handle, 4096, 4) == 0
    reg_u = lib.anyloc_vit_workspace_bytes(handle, 3, 224, 224)
    reg_r = lib.anyloc_vit_workspace_bytes_ragged(handle, 2, _hw((224, 224), (210, 238)))
    assert reg_u > plain_u and reg_r > plain_r
    assert lib.anyloc_vit_workspace_bytes_ragged(handle, 3, _hw((224, 224), (224, 224), (224, 224))) == reg_u
    # 12 more token rows of a 3-image batch: at least their fp32 residual stream, LN output and FFN activation
    assert reg_u - plain_u >= 12 * 4 * (384 + 384 + 1536)
    assert lib.anyloc_vit_set_registers(handle, 4096, 0) == 0
    assert lib.anyloc_vit_workspace_bytes(handle, 3, 224, 224) == plain_u
    assert lib.anyloc_vit_workspace_bytes_ragged(handle, 2, _hw((224, 224), (210, 238))) == plain_r


# ---------------------------------------------------------------- host-side layout ----

def test_ragged_offsets_and_chunks_with_registers():
    from anyloc_amd.extractor import ragged_chunks, ragged_offsets
    sizes = [(224, 224), (476, 630), (14, 14), (210, 238)]
    N = np.array([256, 1530, 1, 255])
    R = 4
    tok, out, pix = ragged_offsets(sizes, use_cls=False, registers=R)
    i = np.arange(len(sizes) + 1)
    assert tok.tolist() == [0] + np.cumsum(N + 1 + R).tolist()
    assert out.tolist() == [0] + np.cumsum(N).tolist() == (tok - i * (1 + R)).tolist()
    assert pix.tolist() == ragged_offsets(sizes, use_cls=False)[2].tolist()
    tok_c, out_c, _ = ragged_offsets(sizes, use_cls=True, registers=R)
    assert tok_c.tolist() == tok.tolist()
    assert out_c.tolist() == [0] + np.cumsum(N + 1).tolist() == (tok - i * R).tolist()
    # registers = 0 is the plain layout
    for use_cls in (False, True):
        assert all((a == b).all() for a, b in zip(ragged_offsets(sizes, use_cls, registers=0), ragged_offsets(sizes, use_cls)))
    # the packing budget counts 1 + R rows per image
    two = [(224, 224), (224, 224)]
    assert ragged_chunks(two, 514) == [(0, 2)]
    assert ragged_chunks(two, 514, registers=R) == [(0, 1), (1, 2)]
    assert ragged_chunks(two, 522, registers=R) == [(0, 2)]
    for budget in (300, 600, 1600, 2000, 10 ** 6):
        for a, b in ragged_chunks(sizes, budget, registers=R):
            assert b - a == 1 or int((N[a:b] + 1 + R).sum()) <= budget


def test_register_models_are_served():
    import utilities
    from anyloc_amd import extractor
    for name in REG_NAMES:
        assert name in extractor._DINO_V2_MODELS and name in utilities._DINO_V2_MODELS
        base = synth.base_model(name)
        assert synth.ARCH[name] == synth.ARCH[base] and synth.n_registers(name) == 4 and synth.n_registers(base) == 0


# ---------------------------------------------------------------- weights ----

@pytest.fixture()
def no_download(monkeypatch, tmp_path):
    from anyloc_amd import weights

    def refuse(*a, **k):
        raise RuntimeError("no download in tests")
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", refuse)
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    monkeypatch.delenv("ANYLOC_SYNTHETIC_WEIGHTS", raising=False)
    monkeypatch.delenv("ANYLOC_DINOV2_WEIGHTS", raising=False)
    weights.unregister_state_dict()
    yield weights
    weights.unregister_state_dict()


def test_reg_checkpoint_file_in_weights_directory(no_download, monkeypatch, tmp_path):
    weights = no_download
    d = tmp_path / "w"
    d.mkdir()
    sd = {"register_tokens": torch.full((1, 4, 384), 0.25)}
    torch.save(sd, d / "dinov2_vits14_reg4_pretrain.pth")
    monkeypatch.setenv("ANYLOC_DINOV2_WEIGHTS", str(d))
    got = weights.resolve_state_dict("dinov2_vits14_reg")
    assert torch.equal(got["register_tokens"], sd["register_tokens"])
    with pytest.raises(FileNotFoundError, match="dinov2_vits14_pretrain.pth"):
        weights.resolve_state_dict("dinov2_vits14")
    assert weights.checkpoint_name("dinov2_vitg14_reg") == "dinov2_vitg14_reg4_pretrain.pth"
    assert weights.checkpoint_name("dinov2_vitg14") == "dinov2_vitg14_pretrain.pth"


def test_reg_checkpoint_file_in_hub_cache(no_download, tmp_path):
    weights = no_download
    ck = tmp_path / "hub" / "checkpoints"
    ck.mkdir(parents=True)
    torch.save({"x": torch.ones(2)}, ck / "dinov2_vitb14_reg4_pretrain.pth")
    assert torch.equal(weights.resolve_state_dict("dinov2_vitb14_reg")["x"], torch.ones(2))
    with pytest.raises(FileNotFoundError):
        weights.resolve_state_dict("dinov2_vitb14")


def test_reg_download_url(no_download, monkeypatch):
    weights = no_download
    seen = []

    def fake(url, **k):
        seen.append(url)
        raise RuntimeError("no network")
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", fake)
    with pytest.raises(FileNotFoundError):
        weights.resolve_state_dict("dinov2_vitl14_reg")
    assert seen == ["https://dl.fbaipublicfiles.com/dinov2/dinov2_vitl14/dinov2_vitl14_reg4_pretrain.pth"]


# ---------------------------------------------------------------- synthetic weights ----

# recorded on the tree before the register models were added (seed 0, depth 2)
PLAIN_SHA256 = {
    "dinov2_vits14": "600ab6e75cc46a70ccd7713ea668bb81c02f3864ea9e68eceedf04b644404d19",
    "dinov2_vitb14": "4d1cf0b6e91d26c258ff4166f17e52e85e0231f28495f88416f1a32946a75a1f",
    "dinov2_vitl14": "75a06eaaa160747f53556d63b3cc1c26be843abc67ce07ddd2ed3b65c4d71235",
    "dinov2_vitg14": "67816dedf9720cc944b496f0c61c812db68b2d977fa9e37a1e64c54f3bd933fb",
}


def _digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        t = sd[k].detach().cpu().contiguous()
        h.update(k.encode())
        h.update(str(tuple(t.shape)).encode())
        h.update(t.numpy().tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("name", sorted(PLAIN_SHA256))
def test_plain_synthetic_state_dicts_unchanged(name):
    assert _digest(synth.synthetic_state_dict(name, 0, depth=2)) == PLAIN_SHA256[name]


@pytest.mark.parametrize("name", REG_NAMES)
def test_reg_synthetic_state_dict(name):
    base = synth.base_model(name)
    sd, plain = synth.synthetic_state_dict(name, 7, depth=1), synth.synthetic_state_dict(base, 7, depth=1)
    assert set(sd) == set(plain) | {"register_tokens"}
    assert all(torch.equal(sd[k], plain[k]) for k in plain)
    reg = sd["register_tokens"]
    assert reg.shape == (1, 4, synth.ARCH[name][0]) and float(reg.std()) > 0.01
    assert not torch.equal(reg, synth.synthetic_state_dict(name, 8, depth=1)["register_tokens"])
    out = synth.outlier_state_dict(sd, name, 1)
    assert torch.equal(out["register_tokens"], reg) and not torch.equal(out["cls_token"], sd["cls_token"])
