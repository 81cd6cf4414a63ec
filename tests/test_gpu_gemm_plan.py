"""The fp32 MFMA GEMM on either side of its plan's decisions (csrc/gemm_f32.hip: gemm_f32_plan): all rows on 64-row tiles, the
unsplit 128-row grid with one live row in its last tile, the two-launch row split with one and with 65 rows in the 64-row part,
K % 32 != 0 (never split) and the chunked summation of a long contraction -- ``anyloc_gemm_nt`` inside the guard arena, against
float64.  The fused epilogues are reached by the forward only: one block of ViT-g/14 on the fp32 kernels at the two batch sizes
where the SwiGLU GEMM and where the LayerScale-residual GEMMs (in place) are cut, against the same forward without a cut.
Every case first asks ``anyloc_gemm_plan_describe`` whether it sits where it claims to.  GPU box only."""
import ctypes as C

import pytest
import torch

from _guard_arena import ALIGN, GUARD, Arena
from anyloc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODE_RTOL = 2e-6             # tests/test_gpu_tile_configs.py: un-normalised tokens of two kernel variants, relative to their scale
HALF = 5                     # csrc/gemm_f32.hip, kF32Tile: the 64 x 128 tile


@pytest.fixture(scope="module")
def lib():
    from anyloc_amd import _lib
    return _lib.load()


def plan(lib, M, N, K, epilogue="store"):
    """-> [(row0, rows, tile_rows, kfull, abl)] of the library's plan under the options in force"""
    from anyloc_amd import _lib
    d = _lib.GemmPlanDesc()
    _lib.check(lib.anyloc_gemm_plan_describe(M, N, K, epilogue.encode(), 0, C.byref(d)), "anyloc_gemm_plan_describe")
    return [(p.row0, p.rows, p.tile_rows, p.kfull, p.abl) for p in d.part[:d.parts]]


# (M, N, K) -> the plan the case is there for
DIRECT = {
    (768, 8192, 32): [(0, 768, 64, 1, 0)],                              # all rows on 64-row tiles
    (769, 8192, 32): [(0, 769, 128, 1, 0)],                             # unsplit, one live row in the last tile
    (1025, 8192, 32): [(0, 1024, 128, 1, 0), (1024, 1, 64, 1, 0)],      # one live row in the 64-row part
    (1089, 8192, 64): [(0, 1024, 128, 1, 0), (1024, 65, 64, 1, 0)],     # a full 64-row tile and one live row behind it
    (1793, 4608, 32): [(0, 1792, 128, 1, 0), (1792, 1, 64, 1, 0)],
    (1025, 8192, 36): [(0, 1025, 128, 0, 0)],                           # K % 32 != 0: the K-tail kernel, never cut
    (130, 40, 8192): [(0, 130, 128, 1, 32)],                            # chunked summation
}


@pytest.mark.parametrize("M,N,K", list(DIRECT))
def test_gemm_nt_where_the_plan_decides(lib, M, N, K):
    """With and without bias, ldc in {N, N + 4}, every buffer a view of exactly its size between guard bytes: nothing outside C
    changes, every element of C is written, and |out - ref| <= 1.5e-6 |a| |w|^T + 1e-6 against float64 (the bound of
    tests/test_gpu_kernels.py::test_gemm_nt)."""
    from anyloc_amd import _lib
    assert plan(lib, M, N, K) == DIRECT[(M, N, K)]
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    a, w, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    ref = (a.double() @ w.double().T).to(DEV)
    bound = (1.5e-6 * (a.abs().double() @ w.abs().double().T) + 1e-6).to(DEV)
    for with_bias in (True, False):
        want = ref + bias.double().to(DEV) if with_bias else ref
        for ldc in (N, N + 4):
            guard = max(GUARD, (256 * ldc * 4 + ALIGN) // ALIGN * ALIGN)       # more than one 256-row tile row of C
            ar = Arena(DEV, 4 * (M * K + N * K + N + M * ldc) + 6 * (guard + ALIGN), guard=guard)
            ain, win = ar.input("A", a), ar.input("W", w)
            bin_ = ar.input("bias", bias) if with_bias else None
            out = ar.output("C", torch.float32, (M, N), (ldc, 1))
            st = lib.anyloc_gemm_nt(_lib.ptr(ain), K, _lib.ptr(win), K, _lib.ptr(bin_), _lib.ptr(out), ldc, M, N, K, _lib.stream_ptr())
            torch.cuda.synchronize()
            what = (M, N, K, with_bias, ldc)
            assert st == 0, (what, lib.anyloc_last_error())
            assert ar.check({"C": None}) == [], what
            err = (out.double() - want).abs()
            print(f"[gemm_nt {what}] max err {float(err.max()):.2e}, largest err / bound {float((err / bound).max()):.3f}")
            assert bool((err <= bound).all()), what


_FWD = {}


def _vitg_block():
    """one block of ViT-g/14 on the fp32 kernels, once"""
    if "model" not in _FWD:
        from anyloc_amd import extractor
        sd = synth.synthetic_state_dict("dinov2_vitg14", 0, depth=1)
        m = extractor.HipDinoV2("dinov2_vitg14", sd, torch.device(DEV), gemm="f32")
        assert m.gemm == "f32"
        _FWD["model"] = m
    return _FWD["model"]


@pytest.fixture(scope="module", autouse=True)
def _drop_the_model():
    yield
    _FWD.clear()


def _tokens(model, imgs):
    """un-normalised block-0 tokens with CLS (what tests/test_gpu_tile_configs.py::_forward compares between kernel variants)"""
    return model.forward_taps(imgs, [(0, "token")], use_cls=True, norm_taps=False).clone()


# images -> the parts (rows, tile rows) of the block's four GEMMs: qkv (plain store), proj and fc2 (LayerScale-residual, in
# place), w12 (SwiGLU)
FORWARD = {
    4: {"qkv": [(1028, 64)], "proj": [(1028, 64)], "fc2": [(1028, 64)], "w12": [(1024, 128), (4, 64)]},
    22: {"qkv": [(5376, 128), (278, 64)], "proj": [(5376, 128), (278, 64)], "fc2": [(5376, 128), (278, 64)], "w12": [(5654, 128)]},
}
BLOCK_GEMMS = {"qkv": (4608, 1536, "store"), "proj": (1536, 1536, "ls_resid"), "fc2": (1536, 4096, "ls_resid"), "w12": (8192, 1536, "swiglu")}


@pytest.mark.parametrize("images", list(FORWARD))
def test_row_split_under_the_fused_epilogues(lib, images):
    """257 token rows per 224 x 224 image.  Default options against gemm_f32_cfg = 10 -- the default tile with no row split,
    itself held to float64 and the oracle by tests/test_gpu_tile_configs.py: un-normalised tokens within 2e-6 of their scale."""
    from anyloc_amd import ops
    M = 257 * images
    for label, (N, K, epi) in BLOCK_GEMMS.items():
        assert [(rows, tr) for _, rows, tr, _, _ in plan(lib, M, N, K, epi)] == FORWARD[images][label], (images, label)
    model = _vitg_block()
    imgs = torch.randn(images, 3, 224, 224, generator=torch.Generator().manual_seed(images)).to(DEV)
    got = _tokens(model, imgs)
    with ops.options(gemm_f32_cfg=10):
        for N, K, epi in BLOCK_GEMMS.values():
            assert [(rows, tr, abl) for _, rows, tr, _, abl in plan(lib, M, N, K, epi)] == [(M, 128, 8)]
        base = _tokens(model, imgs)
    assert got.shape == base.shape and got.numel() == M * 1536 and bool(torch.isfinite(got).all()) and bool(torch.isfinite(base).all())
    scale = float(base.abs().max())
    err = float((got - base).abs().max()) / scale
    print(f"[ViT-g/14 block, {images} images = {M} rows] default against gemm_f32_cfg=10: {err:.3e} of scale {scale:.3e} "
          f"(bound {MODE_RTOL}); bits of cfg 10: {torch.equal(got, base)}")
    assert err < MODE_RTOL, (images, err)
