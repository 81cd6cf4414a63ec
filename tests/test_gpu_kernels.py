"""Unit parity of the HIP building blocks against fp64 / torch references (GPU box only).
Called through the C ABI (anyloc_amd.ops -> ctypes -> libanyloc_hip.so)."""
import math

import pytest
import torch

from _attention_refs import attention_f64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from anyloc_amd import _lib
    _lib.load()
    return torch.device("cuda")


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


# the bars of this module by name (tests/test_gpu_addressing.py holds the same kernels to them at sizes past 2 GiB)
L2NORM_REL = 5e-7          # _rel of anyloc_l2norm_rows against F.normalize in float64
LAYERNORM_ATOL = 5e-6      # largest absolute error of anyloc_layernorm
ATTN_ATOL, ATTN_REL = 2e-5, 5e-6      # anyloc_attention: largest absolute error, and _rel
RESIZE_ATOL = 1e-5         # anyloc_resize_bicubic alone against F.interpolate(mode="bicubic", align_corners=False)


def gemm_nt_bound(abs_products):
    """anyloc_gemm_nt against float64, per output: k-ordered fp32 fma chain, random-walk rounding error ~ sqrt(K) * 6e-8 *
    |partial sums|; ~15 sigma of that at K = 1536 over millions of outputs (a layout bug is O(1)).  abs_products = |A| |W|^T"""
    return 1.5e-6 * abs_products + 1e-6


@pytest.mark.parametrize("M,N,K", [(300, 256, 64), (129, 384, 588), (1000, 32, 96), (64, 17, 40),
                                   (257, 130, 36), (1, 128, 4), (4240, 1536, 1536), (530, 8192, 1536)])
def test_gemm_nt(dev, M, N, K):
    from anyloc_amd import ops
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g)          # asymmetric operands: a transposed C would fail
    bias = torch.randn(N, generator=g)
    ref = a.double() @ w.double().T + bias.double()
    out = ops.gemm_nt(a.to(dev), w.to(dev), bias.to(dev)).cpu()
    assert out.shape == (M, N)
    bound = gemm_nt_bound(a.abs().double() @ w.abs().double().T)
    assert bool(((out.double() - ref).abs() <= bound).all()), _rel(out, ref)
    out2 = ops.gemm_nt(a.to(dev), w.to(dev)).cpu()
    assert bool(((out2.double() - (ref - bias.double())).abs() <= bound).all())


def test_gemm_identity_is_exact(dev):
    """A = I picks rows of W exactly (catches operand/accumulator layout swaps)."""
    from anyloc_amd import ops
    g = torch.Generator().manual_seed(1)
    w = torch.randn(160, 192, generator=g)
    eye = torch.eye(192)
    out = ops.gemm_nt(eye.to(dev), w.to(dev)).cpu()     # [192,160] = W^T
    assert torch.equal(out, w.T.contiguous())


@pytest.mark.parametrize("rows,dim", [(7, 384), (529, 1536), (3, 49152), (5, 10), (2, 6)])
def test_l2norm_rows(dev, rows, dim):
    from anyloc_amd import ops
    g = torch.Generator().manual_seed(rows + dim)
    x = torch.randn(rows, dim, generator=g) * 3
    x[0] = 0                                            # zero row stays zero (eps clamp)
    out = ops.l2norm_rows(x.to(dev)).cpu()
    ref = torch.nn.functional.normalize(x.double(), dim=-1)
    assert _rel(out, ref) < L2NORM_REL
    assert torch.equal(out[0], torch.zeros(dim))


@pytest.mark.parametrize("rows,dim", [(11, 384), (530, 1536), (9, 1024)])
def test_layernorm(dev, rows, dim):
    from anyloc_amd import ops
    g = torch.Generator().manual_seed(rows * dim)
    x = torch.randn(rows, dim, generator=g) * 2 + 0.5
    w, b = torch.randn(dim, generator=g), torch.randn(dim, generator=g)
    out = ops.layernorm(x.to(dev), w.to(dev), b.to(dev), 1e-6).cpu()
    ref = torch.nn.functional.layer_norm(x.double(), (dim,), w.double(), b.double(), 1e-6)
    assert float((out.double() - ref).abs().max()) < LAYERNORM_ATOL


# option attn_cfg shapes the fp32-MFMA kernel alone (csrc/attention.hip, attn_f32_plan): 1 = exact expf and no operand preload,
# 2 = no preload, 3 = exact expf -- three more instantiations of attention_kernel; the split-bf16 kernel does not read it
ATTN_KERNELS = {"fp32-mfma": (0, 0), "split-bf16": (1, 0), "fp32-mfma-cfg1": (0, 1), "fp32-mfma-cfg2": (0, 2), "fp32-mfma-cfg3": (0, 3)}


@pytest.mark.parametrize("kernel", list(ATTN_KERNELS))
@pytest.mark.parametrize("B,T,heads", [(2, 257, 6), (1, 530, 24), (3, 33, 2), (1, 128, 1), (2, 1370, 2), (1, 129, 1)])
def test_attention(dev, B, T, heads, kernel, monkeypatch):
    """Both attention kernels behind anyloc_attention against float64: the exact-fp32 MFMA one -- under every value of option
    attn_cfg -- and the six-product split-bf16 one the x6 forward uses (option attn_x6 selects it for anyloc_attention).
    (1, 129, 1): one query in the second 128-query block."""
    from anyloc_amd import ops
    attn_x6, attn_cfg = ATTN_KERNELS[kernel]
    ops.set_option("attn_x6", attn_x6)
    ops.set_option("attn_cfg", attn_cfg)
    assert ops.get_option("attn_x6") == attn_x6 and ops.get_option("attn_cfg") == attn_cfg
    D = heads * 64
    g = torch.Generator().manual_seed(B * T + heads)
    qkv = torch.randn(B, T, 3 * D, generator=g) * 1.5
    qkv[0, 3, :D] *= 6.0      # a spiky query/key pair: forces the running-max rescale path
    qkv[0, T - 2, D:2 * D] *= 6.0
    out = ops.attention(qkv.to(dev), heads).cpu()
    check_attention(out, qkv, heads)


def check_attention(out, qkv, heads):
    """anyloc_attention's output (CPU) against float64; -> the largest absolute error"""
    ref = attention_f64(qkv, heads)
    worst = float((out.double() - ref).abs().max())
    assert worst < ATTN_ATOL, worst
    assert _rel(out, ref) < ATTN_REL
    return worst


@pytest.mark.parametrize("qg,ks", [(1, 1), (2, 1), (1, 2)], ids=["4x32q", "2x64q", "2x32q-x-2keys"])
@pytest.mark.parametrize("B,T,heads", [(2, 257, 6), (1, 530, 24), (3, 33, 2), (1, 128, 1), (2, 1370, 2), (5, 530, 4), (1, 20, 3)])
def test_attention_h3(dev, B, T, heads, qg, ks):
    """The attention kernel of the two-term fp16 forward (anyloc_attention_h3: per-(head, 32-row group) scaled fp16
    tiles, three matrix-core products per contraction, output written as the h2 image of the projection GEMM)
    against float64.  Tokens of very different magnitude share 32-row groups and images share groups (T % 32 != 0)."""
    from anyloc_amd import ops
    ops.set_option("attn_h3_qg", qg)                      # 2 = the two-waves-of-64-queries workgroup shape (A/B variant)
    ops.set_option("attn_h3_ks", ks)                      # 2 = two query waves x two key waves (the shape of few-image calls)
    D = heads * 64
    g = torch.Generator().manual_seed(B * T + heads)
    qkv = torch.randn(B, T, 3 * D, generator=g) * 1.5
    qkv[0, 3, :D] *= 6.0
    qkv[0, T - 2, D:2 * D] *= 6.0
    qkv[:, ::7] *= 0.05                                   # small-magnitude tokens next to ordinary ones
    qkv[:, 5, 2 * D:] *= 40.0                             # one value row far above the others (sets the image scale)
    if T > 64:
        qkv[0, 32:64, 2 * D:] = 0.0                       # an all-zero V tile (global rows 32..63): must not set the scale
    img, inv = ops.attention_h3(qkv.to(dev), heads)
    check_attention_h3(img, inv, qkv, heads)


def check_attention_h3(img, inv, qkv, heads):
    """anyloc_attention_h3's output image and row scales (device) against float64; -> the largest absolute error"""
    from anyloc_amd import ops
    B, T, D = qkv.shape[0], qkv.shape[1], qkv.shape[2] // 3
    out = ops.h2_image_to_f32(img, inv, B * T, D).reshape(B, T, D).cpu()
    return check_attention_h3_decoded(out, inv, qkv, heads)


def check_attention_h3_decoded(out, inv, qkv, heads):
    """the same from the decoded output [B, T, D] (float64, CPU) and the row scales of those images"""
    B, T, D = qkv.shape[0], qkv.shape[1], qkv.shape[2] // 3
    ref = attention_f64(qkv, heads)
    # every row of an image carries 22 bits relative to the image's largest |v|: error <= 2^-22 of that bound
    vmax = qkv[:, :, 2 * D:].abs().amax(dim=(1, 2)).double()
    err = (out - ref).abs().amax(dim=(1, 2))
    assert bool((err <= 3e-6 * vmax + 2e-6).all()), (err, vmax)
    assert _rel(out, ref) < 5e-6
    assert bool(torch.isfinite(out).all())
    inv_c = inv.cpu().reshape(B, T)
    assert bool((inv_c == inv_c[:, :1]).all())            # one power-of-two scale per image
    assert bool((torch.log2(inv_c) == torch.log2(inv_c).round()).all())
    return float(err.max())


def _attention_h3_raw(qkv, heads, tokens=None):
    """anyloc_attention_h3 on qkv [B, T, 3D], or (tokens = the images' lengths) anyloc_attention_h3_ragged on the packed
    qkv [sum(tokens), 3D]  ->  (h2 image, out_inv) as the kernel left them, in zeroed buffers."""
    import ctypes as C
    from anyloc_amd import _lib
    lib = _lib.load()
    D = heads * 64
    rows = qkv.numel() // (3 * D)
    img = torch.zeros(lib.anyloc_h2_bytes(rows, D), dtype=torch.uint8, device=qkv.device)
    inv = torch.zeros(rows, dtype=torch.float32, device=qkv.device)
    ws = _lib.workspace(lib.anyloc_attention_h3_workspace_bytes(1, rows, heads), qkv.device, "attn_h3")
    if tokens is None:
        B, T = qkv.shape[:2]
        _lib.check(lib.anyloc_attention_h3(_lib.ptr(qkv), _lib.ptr(img), _lib.ptr(inv), B, T, D, heads, _lib.ptr(ws), ws.numel(),
                                           _lib.stream_ptr()), "anyloc_attention_h3")
    else:
        off = torch.zeros(len(tokens) + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(torch.tensor(tokens), 0)
        off_d = off.to(qkv.device)
        _lib.check(lib.anyloc_attention_h3_ragged(_lib.ptr(qkv), _lib.ptr(img), _lib.ptr(inv), len(tokens),
                                                  (C.c_int32 * len(tokens))(*tokens), _lib.ptr(off_d), D, heads, _lib.ptr(ws),
                                                  ws.numel(), _lib.stream_ptr()), "anyloc_attention_h3_ragged")
    torch.cuda.synchronize()
    return img, inv


@pytest.mark.parametrize("ragged_xcd", [None, 0, 1], ids=["uniform", "ragged-xcd-ranges", "ragged-xcd-dealt"])
@pytest.mark.parametrize("n_img,ks_rule", [(85, 2), (86, 1)])
def test_attention_h3_automatic_key_split_at_its_boundary(dev, n_img, ks_rule, ragged_xcd):
    """attn_h3_ks = 0 takes the two-key-wave workgroups (KS = 2) while QB2 * heads * images <= 512, QB2 the workgroups of
    two 32-query groups that cover the (longest) image.  At T = 100 an image intersects at most (100 + 31) // 32 + 1 = 5
    groups, QB2 = (5 + 1) // 2 = 3, and with 2 heads the count is 3 * 2 * n_img: 510 for 85 images (KS = 2), 516 for 86
    (KS = 1).  The automatic choice must give the bits of the forced value the rule names -- and the two forced values
    differ in bits (the key waves' partial sums meet in another order), so that tells which kernel ran.  Uniform batches and
    ragged packs (lengths alternating 100 and 37: the longest image sets the grid), both ragged workgroup orders."""
    from anyloc_amd import ops
    heads, T = 2, 100
    D = heads * 64
    g = torch.Generator().manual_seed(n_img)
    if ragged_xcd is None:
        tokens = None
        qkv = torch.randn(n_img, T, 3 * D, generator=g) * 1.5
        qkv[:, ::7] *= 0.05                               # the spiky generator of test_attention_h3
        qkv[0, 3, :D] *= 6.0
        qkv[0, T - 2, D:2 * D] *= 6.0
        qkv[:, 5, 2 * D:] *= 40.0
    else:
        tokens = [T if i % 2 == 0 else 37 for i in range(n_img)]
        qkv = torch.randn(sum(tokens), 3 * D, generator=g) * 1.5
        qkv[::7] *= 0.05
        qkv[3, :D] *= 6.0
        qkv[T - 2, D:2 * D] *= 6.0
        qkv[5::137, 2 * D:] *= 40.0
    assert 3 * heads * 85 <= 512 < 3 * heads * 86
    names = ("attn_h3_ks", "attn_h3_qg", "attn_h3_ragged_xcd")
    before = {k: ops.get_option(k) for k in names}
    try:
        ops.set_option("attn_h3_qg", 1)
        if ragged_xcd is not None:
            ops.set_option("attn_h3_ragged_xcd", ragged_xcd)
        got = {}
        for ks in (0, 1, 2):
            ops.set_option("attn_h3_ks", ks)
            got[ks] = _attention_h3_raw(qkv.to(dev), heads, tokens)
    finally:
        for k, v in before.items():
            ops.set_option(k, v)
    assert not torch.equal(got[1][0], got[2][0])          # the two shapes are told apart by their bits
    assert torch.equal(got[0][0], got[ks_rule][0]) and torch.equal(got[0][1], got[ks_rule][1])


@pytest.mark.parametrize("H,W", [(224, 224), (333, 481), (126, 155)])
def test_preprocess_u8_matches_totensor_normalize_centercrop(dev, H, W):
    """uint8 HWC -> float CHW ingest == ToTensor + Normalize + CenterCrop(h//14*14, w//14*14), bit-exact."""
    from anyloc_amd import preprocess, synth
    g = torch.Generator().manual_seed(H + W)
    u8 = torch.randint(0, 256, (3, H, W, 3), generator=g, dtype=torch.uint8)
    out = preprocess.images_to_input(u8).cpu()
    ref = totensor_normalize_centercrop(u8)
    assert out.shape == ref.shape
    assert torch.equal(out, ref)


def totensor_normalize_centercrop(u8):
    """uint8 [B, H, W, 3] (CPU) -> ToTensor + Normalize + CenterCrop(H // 14 * 14, W // 14 * 14) in torch on the CPU"""
    from anyloc_amd import synth
    H, W = u8.shape[1:3]
    x = u8.permute(0, 3, 1, 2).float().div(255)
    mean = torch.tensor(synth.IMAGENET_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(synth.IMAGENET_STD).view(1, 3, 1, 1)
    x = (x - mean) / std
    th, tw = H // 14 * 14, W // 14 * 14
    t, l = int(round((H - th) / 2.0)), int(round((W - tw) / 2.0))
    return x[..., t:t + th, l:l + tw]


@pytest.mark.parametrize("H,W,max_size", [(480, 640, 322), (700, 500, 448), (333, 1024, 1024), (2000, 1500, 1024)])
def test_ingest_with_bicubic_downscale(dev, H, W, max_size):
    """uint8 ingest with the demo's downscale rule (demo/anyloc_vlad_generate.py:163-181): ToTensor + Normalize, bicubic
    resize so the longer side is max_img_size (aspect kept), CenterCrop to multiples of 14 -- vs the same steps in torch."""
    from anyloc_amd import preprocess, synth
    g = torch.Generator().manual_seed(H * 3 + W)
    u8 = (torch.rand(2, H // 8, W // 8, 3, generator=g) * 255).to(torch.uint8)
    u8 = torch.nn.functional.interpolate(u8.permute(0, 3, 1, 2).float(), size=(H, W), mode="bilinear").permute(0, 2, 3, 1)
    u8 = (u8 + 8 * torch.rand(2, H, W, 3, generator=g)).clamp(0, 255).to(torch.uint8)
    out = preprocess.images_to_input(u8, max_img_size=max_size).cpu()
    x = u8.permute(0, 3, 1, 2).float().div(255)
    x = (x - torch.tensor(synth.IMAGENET_MEAN).view(1, 3, 1, 1)) / torch.tensor(synth.IMAGENET_STD).view(1, 3, 1, 1)
    if max(H, W) > max_size:
        if H == max(H, W):
            w2, h2 = int(W * max_size / H), max_size
        else:
            h2, w2 = int(H * max_size / W), max_size
        x = torch.nn.functional.interpolate(x, size=(h2, w2), mode="bicubic", align_corners=False)
    h, w = x.shape[-2:]
    th, tw = h // 14 * 14, w // 14 * 14
    t, l = int(round((h - th) / 2.0)), int(round((w - tw) / 2.0))
    ref = x[..., t:t + th, l:l + tw]
    assert out.shape == ref.shape and out.shape[-1] % 14 == 0 and out.shape[-2] % 14 == 0
    assert float((out - ref).abs().max()) < 2e-5
    # the resize alone, an upscale too
    y = torch.randn(1, 3, 37, 53, generator=g)
    up = preprocess.resize_bicubic(y.to(dev), (90, 61)).cpu()
    assert float((up - torch.nn.functional.interpolate(y, size=(90, 61), mode="bicubic", align_corners=False)).abs().max()) < RESIZE_ATOL
