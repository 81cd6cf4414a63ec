"""Kernel instantiations of the two-term fp16 forward that the kernel-trace audit of the suite (profiles/kernel_coverage.md,
tools/kernel_coverage.py) found no test launching, each reached at the smallest shape that selects it and held to the bar of
the existing test of its family (``pytest -m gpu``).  Before a launch the library's own plan (anyloc_h3_plan_describe) must name
the intended route and tile.

  * the fp32 FFN epilogues of the unfused data flow (h3_fuse = 0) on the tiles tests/test_gpu_tile_configs.py leaves out: GELU on
    the fixed 128 x 128 tile and on the batched 128 x 256 tile, SwiGLU (interleaved layout) on the fixed 64 x 64 tile;
  * the LayerNorm lead role in front of the LDS-transposing SWIGLU_H2 epilogue (a ViT-g built under h3_swiglu_t = 0), one image
    and batched;
  * layernorm_h2_kernel with 2 and 4 rows per wave, 4 and 8 waves, at the widths of ViT-S / B / L (the scheduling test of
    tests/test_gpu_round3.py runs ViT-g only), and -- on two models of the test's own, 256 and 2 048 columns wide, which
    anyloc_vit_create accepts like any width that is a multiple of 64 up to 2 048 -- the one- and eight-float4-per-lane
    instantiations of layernorm_h2_kernel, layernorm_h2_direct_kernel and layernorm_x3_kernel;
  * the batched 128 x 256 tile of the split-bf16 GEMM under the fp32 GELU / SwiGLU epilogues (x6_fuse = 0);
  * the fp32-MFMA attention kernel writing the split-bf16 plane image (attn_x6 = 0 under the fused x6 forward), uniform and ragged;
  * the patch epilogue of the fp32-MFMA GEMM without a K tail (a model whose patch-embedding rows are zero-padded from 588 to 608
    columns, as anyloc_vit_config.patch_k_pad allows) under every gemm_f32_cfg."""
import pytest
import torch

import _plan_edges as pe
from anyloc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOKEN_ATOL = 2e-5            # tests/test_gpu_vit.py, tests/test_gpu_tile_configs.py: unit-norm token rows against the oracle
ROUTE_FIXED, ROUTE_BATCHED = 1, 2
TILE_TINY, TILE_128 = 6, 7   # csrc/gemm_h3_kernel.hpp: kH3Tile ids of the two fixed shapes


@pytest.fixture(scope="module")
def lib():
    from anyloc_amd import _lib
    return _lib.load()


def _oracle_values(name, sd, imgs, layer):
    from oracle import dinov2_ref
    with torch.device("meta"):                                                 # (no random init of the full-depth model)
        full = dinov2_ref.DinoVisionTransformer(name)
    full.blocks = full.blocks[:layer + 1]
    full.load_state_dict(sd, strict=True, assign=True)
    full.eval()
    return dinov2_ref.extract_facet(full, imgs, layer, "value")


# (model, images of 224 x 224 = 257 rows each, options at model build, fc1 epilogue, route, tile)
UNFUSED = [("dinov2_vits14", 11, {}, "gelu", ROUTE_FIXED, TILE_128),                 # 2 827 rows: 23 x 12 tiles of 128 x 128, no longer "tiny"
           ("dinov2_vitl14", 16, {}, "gelu", ROUTE_BATCHED, 0),                      # 4 112 rows: 33 x 16 = 528 tiles of 128 x 256
           ("dinov2_vitg14", 1, {"h3_swiglu_t": 0}, "swiglu", ROUTE_FIXED, TILE_TINY)]  # 257 rows: 3 x 64 tiles of 128 x 128 < h3_tiny_max


@pytest.mark.parametrize("name,batch,build,epilogue,route,tile", UNFUSED, ids=[f"{u[0]}-{u[1]}-{u[3]}" for u in UNFUSED])
def test_unfused_ffn_epilogues_on_the_other_tiles(lib, name, batch, build, epilogue, route, tile):
    """h3_fuse = 0: fc1 writes the fp32 activation through the GELU / SwiGLU epilogue, which has no small-M plans -- two fixed
    shapes below 512 tiles of 128 x 256, the batched tile above.  2 blocks, layer-1 values against the CPU oracle under
    TOKEN_ATOL (tests/test_gpu_tile_configs.py::test_forward_epilogues_every_configuration, which reaches GELU on the 64 x 64 and
    SwiGLU on the 128 x 128 fixed tile only)."""
    from anyloc_amd import extractor, ops
    sd = synth.synthetic_state_dict(name, 40, depth=2)
    imgs = synth.synthetic_places(batch, 1, 224, 224, seed=9)[0]
    assert imgs.shape[0] == batch
    with ops.options(**build):
        m = extractor.HipDinoV2(name, sd, torch.device(DEV), gemm="h3")
    m.ffn_check = False
    dim, _, _, ffn, hidden = synth.ARCH[name]
    assert m.fc1_layout == 0
    with ops.options(h3_fuse=0):
        d = pe.describe(lib, 257 * batch, 2 * hidden if ffn == "swiglu" else hidden, dim, epilogue, pe.KIND_FC1, pe.WS)
        assert (d["route"], d["tile"], d["lead"]) == (route, tile, 0), d
        got = m.forward_taps(imgs.to(DEV), [(1, "value")]).clone()
        assert torch.equal(got, m.forward_taps(imgs.to(DEV), [(1, "value")]))
    fused = m.forward_taps(imgs.to(DEV), [(1, "value")])
    assert not torch.equal(got, fused), "h3_fuse = 0 changed no bit: the option was not read"
    want = _oracle_values(name, sd, imgs, 1)
    err = float((got.cpu() - want).abs().max())
    print(f"{name} x {batch}, fc1 {epilogue} on route {route} tile {tile}: err {err:.2e} (bound {TOKEN_ATOL})")
    assert torch.isfinite(got).all() and err < TOKEN_ATOL


@pytest.mark.parametrize("batch", [1, 17])
def test_layernorm_lead_role_in_front_of_the_interleaved_swiglu(lib, batch):
    """A 3-block ViT-g built under h3_swiglu_t = 0 (w12 on the SWIGLU_H2 epilogue): LayerNorm 2 as the lead role of the w12 launch,
    one 322 x 322 image (h3s_ln_lead, the 192 x 128 plan) and 17 (h3_ln_lead, the batched role).  The plan must name the role; the
    tokens must be the bits of the separate launches on every repeat -- the bar of tests/test_gpu_round6.py::
    test_layernorm_lead_role_gives_the_bits_of_the_separate_launch and ::test_batched_layernorm_lead_role_gives_the_bits_of_the_separate_launch."""
    from anyloc_amd import extractor, ops
    name = "dinov2_vitg14"
    sd = synth.synthetic_state_dict(name, 41, device=DEV, depth=3)
    with ops.options(h3_swiglu_t=0):
        m = extractor.HipDinoV2(name, sd, torch.device(DEV), gemm="h3")
    assert m.fc1_layout == 0
    m.ffn_check = False
    img = torch.randn(batch, 3, 322, 322, generator=torch.Generator().manual_seed(batch)).to(DEV)
    lead, role = ("h3s_ln_lead", 1) if batch == 1 else ("h3_ln_lead", 2)
    N, K, _, kind, flags = pe.block_gemms(name)["fc1"]
    with ops.options(**{lead: 0}):
        assert pe.describe(lib, 530 * batch, N, K, "swiglu_h2", kind, flags)["lead"] == 0
        want = m.forward_taps(img, [(2, "token")]).clone()
    assert torch.isfinite(want).all()
    with ops.options(**{lead: 1}):
        d = pe.describe(lib, 530 * batch, N, K, "swiglu_h2", kind, flags)
        assert d["lead"] == role and (batch > 1 or (d["tile"], d["stages"]) == (7, 6)), d
        for rep in range(12):
            assert torch.equal(m.forward_taps(img, [(2, "token")]), want), (batch, rep, "the lead-role forward differs from the separate launches")


@pytest.mark.parametrize("name", ["dinov2_vits14", "dinov2_vitb14", "dinov2_vitl14"])
def test_layernorm_scheduling_variants_at_every_width(name):
    """layernorm_h2 with 1 / 2 / 4 rows per wave on 4 or 8 waves reorders instructions, not arithmetic: at 384, 768 and 1 024
    columns (2, 3 and 4 float4 per lane) the tokens are the bits of the default launch -- the bar of
    tests/test_gpu_round3.py::test_scheduling_variants_are_bitwise_equal, which runs 1 536 columns only -- and the default
    meets the oracle."""
    from anyloc_amd import extractor, ops
    sd = synth.synthetic_state_dict(name, 42, depth=2)
    m = extractor.HipDinoV2(name, sd, torch.device(DEV), gemm="h3")
    imgs = synth.synthetic_places(2, 1, 224, 224, seed=10)[0]
    base = m.forward_taps(imgs.to(DEV), [(1, "token")], use_cls=True, norm_taps=False).clone()
    assert torch.isfinite(base).all()
    for opts in (dict(ln_rows_per_wave=1), dict(ln_rows_per_wave=2), dict(ln_rows_per_wave=4), dict(ln_rows_per_wave=2, ln_waves=4)):
        with ops.options(**opts):
            ops.profile_enable(True); ops.profile_reset()
            got = m.forward_taps(imgs.to(DEV), [(1, "token")], use_cls=True, norm_taps=False)
            torch.cuda.synchronize()
            prof = ops.profile_dump()
            ops.profile_enable(False)
        assert "layernorm_h2" in prof, sorted(prof)                            # a launch of its own, not a lead role
        assert torch.equal(got, base), (name, opts)
    val = m.forward_taps(imgs.to(DEV), [(1, "value")])
    err = float((val.cpu() - _oracle_values(name, sd, imgs, 1)).abs().max())
    assert err < TOKEN_ATOL, err


# ------------------------------------------------------------------------------------------- widths no published model has ----
NARROW, WIDE = "dinov2_test_d256", "dinov2_test_d2048"
TEST_ARCH = {NARROW: (256, 2, 4, "mlp", 1024), WIDE: (2048, 2, 32, "mlp", 2048)}


@pytest.fixture
def test_archs(monkeypatch):
    """two 2-block models of 256 and 2 048 columns (head_dim 64), known to the synthetic weights, the extractor and the oracle
    for the length of a test"""
    from oracle import dinov2_ref
    for name, arch in TEST_ARCH.items():
        monkeypatch.setitem(synth.ARCH, name, arch)
        monkeypatch.setitem(dinov2_ref.ARCH, name, arch)


@pytest.mark.parametrize("name", [NARROW, WIDE])
def test_layernorm_at_the_narrowest_and_widest_rows(test_archs, name):
    """One and eight float4 per lane (256 and 2 048 columns): the direct kernel (514 rows), the tiled kernel with 1 / 2 / 4 rows per
    wave on 4 or 8 waves -- the same bits (tests/test_gpu_round3.py::test_scheduling_variants_are_bitwise_equal) -- and
    layernorm_x3_kernel under the split-bf16 forward; both forwards against the CPU oracle under TOKEN_ATOL."""
    from anyloc_amd import extractor, ops
    sd = synth.synthetic_state_dict(name, 43, depth=2)
    imgs = synth.synthetic_places(2, 1, 224, 224, seed=11)[0]
    want = _oracle_values(name, sd, imgs, 1)
    assert want.shape == (2, 256, TEST_ARCH[name][0])
    m = extractor.HipDinoV2(name, sd, torch.device(DEV), gemm="h3")
    assert ops.get_option("ln_direct_rows") > 514
    base = m.forward_taps(imgs.to(DEV), [(1, "token")], use_cls=True, norm_taps=False).clone()
    for opts in (dict(ln_rows_per_wave=1), dict(ln_rows_per_wave=2), dict(ln_rows_per_wave=4), dict(ln_rows_per_wave=2, ln_waves=4)):
        with ops.options(**opts):
            assert torch.equal(m.forward_taps(imgs.to(DEV), [(1, "token")], use_cls=True, norm_taps=False), base), (name, opts)
    err = float((m.forward_taps(imgs.to(DEV), [(1, "value")]).cpu() - want).abs().max())
    x6 = extractor.HipDinoV2(name, sd, torch.device(DEV), gemm="x6")
    with ops.options(x6_min_rows=0):
        ops.profile_enable(True); ops.profile_reset()
        got = x6.forward_taps(imgs.to(DEV), [(1, "value")]).clone()
        torch.cuda.synchronize()
        prof = ops.profile_dump()
        ops.profile_enable(False)
    assert "layernorm_x3" in prof, sorted(prof)
    err_x6 = float((got.cpu() - want).abs().max())
    print(f"{name}: h3 err {err:.2e}, x6 err {err_x6:.2e} (bound {TOKEN_ATOL})")
    assert err < TOKEN_ATOL and err_x6 < TOKEN_ATOL


# ------------------------------------------------------------------------------------------------- split-bf16 forward ----
@pytest.mark.parametrize("name,batch", [("dinov2_vitl14", 16), ("dinov2_vitg14", 8)])
def test_x6_unfused_ffn_epilogues_on_the_batched_tile(name, batch):
    """x6_fuse = 0 with 512 or more tiles of 128 x 256 in the FFN input GEMM (ViT-L: 33 x 16, ViT-g: 17 x 32): the fp32 GELU /
    SwiGLU epilogue on the default tile, where tests/test_gpu_tile_configs.py (514 rows) meets the 128 x 128 tile of few-tile
    calls; layer-1 values against the CPU oracle under TOKEN_ATOL, other bits than the fused flow."""
    from anyloc_amd import extractor, ops
    dim, _, _, ffn, hidden = synth.ARCH[name]
    assert -(-257 * batch // 128) * -(-(2 * hidden if ffn == "swiglu" else hidden) // 256) >= 512       # csrc/gemm_x6.hip: x6_plan
    sd = synth.synthetic_state_dict(name, 44, depth=2)
    imgs = synth.synthetic_places(batch, 1, 224, 224, seed=12)[0]
    m = extractor.HipDinoV2(name, sd, torch.device(DEV), gemm="x6")
    m.ffn_check = False
    with ops.options(x6_min_rows=0):
        fused = m.forward_taps(imgs.to(DEV), [(1, "value")]).clone()
        with ops.options(x6_fuse=0):
            got = m.forward_taps(imgs.to(DEV), [(1, "value")]).clone()
    assert not torch.equal(got, fused), "x6_fuse = 0 changed no bit: the option was not read"
    err = float((got.cpu() - _oracle_values(name, sd, imgs, 1)).abs().max())
    print(f"{name} x {batch}, x6 unfused: err {err:.2e} (bound {TOKEN_ATOL})")
    assert torch.isfinite(got).all() and err < TOKEN_ATOL


def test_fp32_attention_writes_the_plane_image():
    """attn_x6 = 0 under the fused split-bf16 forward: the fp32-MFMA attention kernel writes proj's operand as the plane image
    (its OUT3 instantiations, uniform and ragged), where the default runs attention_x6_kernel.  A 2-block ViT-S on two images of
    one size and, through the ragged forward, of two sizes; values against the CPU oracle under TOKEN_ATOL, other bits than the
    default."""
    from anyloc_amd import extractor, ops
    name = "dinov2_vits14"
    sd = synth.synthetic_state_dict(name, 45, depth=2)
    m = extractor.HipDinoV2(name, sd, torch.device(DEV), gemm="x6")
    m.ffn_check = False
    a = synth.synthetic_places(2, 1, 224, 224, seed=13)[0]
    b = synth.synthetic_places(1, 1, 224, 308, seed=14)[0]
    with ops.options(x6_min_rows=0):
        default = m.forward_taps(a.to(DEV), [(1, "token")]).clone()
        with ops.options(attn_x6=0):
            got = m.forward_taps(a.to(DEV), [(1, "token")]).clone()
            packed, off = m.forward_taps_ragged([a[0].to(DEV), b[0].to(DEV)], [(1, "token")])
    assert not torch.equal(got, default), "attn_x6 = 0 changed no bit: the option was not read"
    from oracle import dinov2_ref
    with torch.device("meta"):
        full = dinov2_ref.DinoVisionTransformer(name)
    full.blocks = full.blocks[:2]
    full.load_state_dict(sd, strict=True, assign=True)
    full.eval()
    err = float((got.cpu() - dinov2_ref.extract_facet(full, a, 1, "token")).abs().max())
    off = off.tolist()
    assert off == [0, 256, 256 + 352]
    err_r = max(float((packed[off[i]:off[i + 1]].cpu() - dinov2_ref.extract_facet(full, im, 1, "token")[0]).abs().max())
                for i, im in enumerate((a[:1], b)))
    print(f"fp32 attention -> plane image: uniform err {err:.2e}, ragged err {err_r:.2e} (bound {TOKEN_ATOL})")
    assert err < TOKEN_ATOL and err_r < TOKEN_ATOL


# ------------------------------------------------------------------------------------ patch embedding without a K tail ----
# option gemm_f32_cfg -> (tile id in kF32Tile, ABL) of a wide call (tests/test_gemm_plan_cpu.py: CFG_TILE)
PATCH_CFGS = {0: (0, 0), 1: (1, 0), 2: (2, 0), 3: (3, 0), 4: (4, 0), 10: (0, 8), 11: (4, 8), 20: (0, 64)}


def test_patch_epilogue_without_a_k_tail(lib):
    """The patch embedding of a plain model contracts over 3 x 14 x 14 = 588 columns, never a multiple of 32, so the KFULL
    instantiations of the patch epilogue are reached only by a model whose rows are padded: patch_k_pad = 608 (zeros).  A 2-block
    ViT-S on the fp32 kernels under every gemm_f32_cfg that computes right results; the library's plan for the patch GEMM
    (anyloc_gemm_plan_describe) must name the option's tile without a K-tail predicate; layer-1 values against the CPU oracle under
    TOKEN_ATOL (tests/test_gpu_tile_configs.py::test_forward_epilogues_every_configuration, family f32) and within 2e-6 of the
    unpadded model's, that test's bar between two configurations (zero columns add nothing; the slabs are cut elsewhere)."""
    import ctypes as C
    from anyloc_amd import _lib, extractor, ops
    name = "dinov2_vits14"
    sd = synth.synthetic_state_dict(name, 46, depth=2)
    imgs = synth.synthetic_places(2, 1, 224, 308, seed=15)[0]                  # 2 x 352 patches: a partial tile of every shape
    want = _oracle_values(name, sd, imgs, 1)
    plain = extractor.HipDinoV2(name, sd, torch.device(DEV), gemm="f32")
    padded = extractor.HipDinoV2(name, sd, torch.device(DEV), gemm="f32", patch_k_pad=608)
    assert plain.patch_k_pad == 588 and padded.patch_k_pad == 608
    base = plain.forward_taps(imgs.to(DEV), [(1, "value")]).clone()
    for cfg, (tile, abl) in PATCH_CFGS.items():
        with ops.options(gemm_f32_cfg=cfg):
            d = _lib.GemmPlanDesc()
            assert lib.anyloc_gemm_plan_describe(2 * 352, 384, 608, b"patch", 0, C.byref(d)) == 0
            assert (d.parts, d.part[0].tile, d.part[0].kfull, d.part[0].abl, d.part[0].rowsq) == (1, tile, 1, abl, 0), cfg
            assert lib.anyloc_gemm_plan_describe(2 * 352, 384, 588, b"patch", 0, C.byref(d)) == 0 and d.part[0].kfull == 0
            got = padded.forward_taps(imgs.to(DEV), [(1, "value")]).clone()
        err, e_base = float((got.cpu() - want).abs().max()), float((got - base).abs().max())
        print(f"patch epilogue, K = 608, gemm_f32_cfg {cfg}: err {err:.2e} (bound {TOKEN_ATOL}), against the unpadded model {e_base:.2e}")
        assert torch.isfinite(got).all() and err < TOKEN_ATOL and e_base <= 2e-6, (cfg, err, e_base)
