"""Ragged batches: images of different sizes in one ViT forward (``anyloc_vit_forward_ragged``,
``HipDinoV2.forward_taps_ragged``, ``describe_images``), against float64 attention and the CPU oracle
(``oracle/dinov2_ref.py``) per image.  GPU box only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _attention_refs import attention_f64, spiky_qkv_image
from anyloc_amd import synth, weights
from oracle import dinov2_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOKEN_ATOL = 2e-5
# a mixed batch: the script default 476 x 630 (T = 1531), one patch (T = 2), square / non-square, ViT-g bench size
SIZES = [(224, 224), (476, 630), (14, 14), (322, 322), (98, 154)]


# ---------------------------------------------------------------- attention kernels alone ----

# token counts: T = 2 (a 14 x 14 image), T > 1984 (more than 64 key groups: per-tile scales from memory), ordinary ones;
# none a multiple of 32, so every image after the first starts inside a 32-row group it shares with its neighbour
RAGGED_T = [530, 2, 2100, 197, 37, 1531]


def _run_ragged_attention(kernel, qkv, tokens, heads):
    from anyloc_amd import _lib, ops
    import ctypes as C
    lib = _lib.load()
    D = heads * 64
    rows = sum(tokens)
    x = qkv.to(DEV).contiguous()
    off = torch.zeros(len(tokens) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(tokens), 0)
    off_d = off.to(DEV)
    tok = (C.c_int32 * len(tokens))(*tokens)
    if kernel == "h3":
        img = torch.empty(lib.anyloc_h2_bytes(rows, D), dtype=torch.uint8, device=DEV)
        inv = torch.empty(rows, dtype=torch.float32, device=DEV)
        ws = _lib.workspace(lib.anyloc_attention_h3_workspace_bytes(1, rows, heads), DEV, "attn_h3")
        _lib.check(lib.anyloc_attention_h3_ragged(_lib.ptr(x), _lib.ptr(img), _lib.ptr(inv), len(tokens), tok, _lib.ptr(off_d),
                                                  D, heads, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   "anyloc_attention_h3_ragged")
        out = ops.h2_image_to_f32(img, inv, rows, D).cpu()
    else:
        ops.set_option("attn_x6", 1 if kernel == "split-bf16" else 0)
        y = torch.empty(rows, D, dtype=torch.float32, device=DEV)
        _lib.check(lib.anyloc_attention_ragged(_lib.ptr(x), _lib.ptr(y), len(tokens), tok, _lib.ptr(off_d), D, heads,
                                               _lib.stream_ptr()), "anyloc_attention_ragged")
        out = y.cpu()
    torch.cuda.synchronize()
    return out.double(), off.tolist()


@pytest.mark.parametrize("kernel,ks,xcd", [("h3", 1, 1), ("h3", 2, 1), ("h3", 1, 0), ("h3", 2, 0), ("fp32-mfma", 0, 1),
                                            ("split-bf16", 0, 1)],
                         ids=["h3-keys-unsplit", "h3-keys-split-2", "h3-keys-unsplit-xcd-ranges", "h3-keys-split-2-xcd-ranges",
                              "fp32-mfma", "split-bf16"])
def test_ragged_attention_vs_float64(kernel, ks, xcd):
    """Every image of one packed batch against its own float64 attention, and no leakage: flipping the signs of one image's
    q / k / v (same magnitudes, so the same tile scales in the two-term fp16 kernel) changes that image and leaves every
    other image's rows bit for bit as they were."""
    from anyloc_amd import ops
    ops.set_option("attn_h3_ks", ks)
    ops.set_option("attn_h3_ragged_xcd", xcd)          # both workgroup orders of the two-term fp16 kernel
    heads = 2
    D = heads * 64
    parts = [spiky_qkv_image(t, heads, 100 + i) for i, t in enumerate(RAGGED_T)]
    qkv = torch.cat(parts)
    try:
        out, off = _run_ragged_attention(kernel, qkv, RAGGED_T, heads)
        assert bool(torch.isfinite(out).all())
        for i, p in enumerate(parts):
            ref = attention_f64(p, heads, per_head=True)
            got = out[off[i]:off[i + 1]]
            vmax = float(p[:, 2 * D:].abs().max())
            err = float((got - ref).abs().max())
            # the bars of tests/test_gpu_long_sequences.py at these lengths: 22 bits relative to the image's largest |v|
            # (two-term fp16), 2e-5 + the fp32 logit rounding of the spiky query / key rows (fp32 / split-bf16)
            bar = 3e-6 * vmax + 2e-6 if kernel == "h3" else 2e-5 + 2.0 ** -22 * 250.0 * vmax
            print(f"[{kernel} ks={ks}] image {i} T={RAGGED_T[i]}: err {err:.2e} (bar {bar:.2e})")
            assert err <= bar, (i, RAGGED_T[i], err, bar)
        # no cross-image leakage
        j = 2                                                       # the T = 2100 image, neighbour of T = 2 and T = 197
        g = torch.Generator().manual_seed(7)
        flip = torch.where(torch.rand(parts[j].shape, generator=g) < 0.5, -1.0, 1.0)
        qkv2 = torch.cat([p * flip if i == j else p for i, p in enumerate(parts)])
        out2, _ = _run_ragged_attention(kernel, qkv2, RAGGED_T, heads)
        for i in range(len(parts)):
            a, b = out[off[i]:off[i + 1]], out2[off[i]:off[i + 1]]
            if i == j:
                assert float((a - b).abs().max()) > 1e-2
            else:
                assert torch.equal(a, b), i
    finally:
        ops.set_option("attn_h3_ks", 0)
        ops.set_option("attn_h3_ragged_xcd", 1)
        ops.set_option("attn_x6", -1)


# ---------------------------------------------------------------- the ViT forward ----

class _Case:
    """ViT-S/14 with 2 synthetic blocks: the HIP model per arithmetic and the restated hub model."""

    def __init__(self):
        self.name = "dinov2_vits14"
        self.sd = synth.synthetic_state_dict(self.name, 31, depth=2)
        m = dinov2_ref.DinoVisionTransformer(self.name)
        m.blocks = m.blocks[:2]
        m.load_state_dict(self.sd, strict=True)
        self.ref = m.eval()
        self._models = {}
        g = torch.Generator().manual_seed(5)
        self.imgs = []
        for h, w in SIZES:
            x = torch.randn(1, 3, max(1, h // 14), max(1, w // 14), generator=g)
            x = F.interpolate(x, size=(h, w), mode="bilinear", align_corners=False) + 0.3 * torch.randn(1, 3, h, w, generator=g)
            self.imgs.append(x[0])

    def model(self, mode):
        from anyloc_amd.extractor import HipDinoV2
        if mode not in self._models:
            self._models[mode] = HipDinoV2(self.name, {k: v.to(DEV) for k, v in self.sd.items()}, torch.device(DEV), gemm=mode)
        return self._models[mode]

    def oracle(self, img, layer, facet, use_cls=False):
        with torch.no_grad():
            return dinov2_ref.extract_facet(self.ref, img[None], layer, facet, use_cls=use_cls)[0]


@pytest.fixture(scope="module")
def case():
    return _Case()


def _check_rows(packed, offsets, refs, bar=TOKEN_ATOL):
    off = offsets.cpu().tolist()
    assert len(off) == len(refs) + 1 and off[0] == 0 and off[-1] == packed.shape[0]
    got = packed.cpu()
    errs = []
    for i, ref in enumerate(refs):
        g = got[off[i]:off[i + 1]]
        assert g.shape == ref.shape, (i, g.shape, ref.shape)
        errs.append(float((g - ref).abs().max()))
    print("per-image max-abs err", ["%.1e" % e for e in errs])
    assert max(errs) <= bar, errs
    assert bool(torch.isfinite(got).all())


@pytest.mark.parametrize("mode", ["h3", "x6", "f32"])
def test_ragged_forward_vs_oracle(case, mode):
    """Every image of a mixed batch (476 x 630 and a one-patch image included) within 2e-5 of its own oracle forward."""
    m = case.model(mode)
    packed, offsets = m.forward_taps_ragged(case.imgs, [(1, "value")])
    _check_rows(packed, offsets, [case.oracle(x, 1, "value") for x in case.imgs])


@pytest.mark.parametrize("facet,use_cls", [("token", False), ("query", False), ("value", True)])
def test_ragged_facets_and_cls(case, facet, use_cls):
    m = case.model("h3")
    packed, offsets = m.forward_taps_ragged(case.imgs, [(1, facet)], use_cls=use_cls)
    _check_rows(packed, offsets, [case.oracle(x, 1, facet, use_cls) for x in case.imgs])


def test_ragged_two_taps_out_of_order_norm_concat(case):
    """Two taps given out of layer order with norm_concat: blocks in the caller's order, the concatenation normalised."""
    m = case.model("h3")
    packed, offsets = m.forward_taps_ragged(case.imgs, [(1, "value"), (0, "key")], norm_concat=True)
    refs = [F.normalize(torch.cat([case.oracle(x, 1, "value"), case.oracle(x, 0, "key")], dim=-1), dim=-1) for x in case.imgs]
    _check_rows(packed, offsets, refs)


def test_ragged_batch_larger_than_max_rows_is_chunked(case):
    from anyloc_amd.extractor import ragged_chunks
    m = case.model("h3")
    keep = m.max_rows
    m.max_rows = 1600                                   # the 476 x 630 image (1531 rows) nearly fills a call on its own
    try:
        sizes = [tuple(x.shape[1:]) for x in case.imgs]
        assert len(ragged_chunks(sizes, m.max_rows)) >= 3
        packed, offsets = m.forward_taps_ragged(case.imgs, [(1, "value")])
    finally:
        m.max_rows = keep
    _check_rows(packed, offsets, [case.oracle(x, 1, "value") for x in case.imgs])


@pytest.mark.parametrize("mode", ["h3", "x6", "f32"])
def test_ragged_equal_sizes_match_the_uniform_forward(case, mode):
    """B images of one size through the ragged entry point and through forward_taps: the same bits (the block GEMMs,
    LayerNorms and quantisers see the same row count; the patch GEMM runs the same tile configuration with a plain bias
    epilogue, and embed_ragged forms the same fp32 sums as EPI_PATCH + cls_rows)."""
    m = case.model(mode)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4, 3, 224, 308, generator=g).to(DEV)
    uni = m.forward_taps(x, [(1, "value")]).reshape(-1, m.dim).cpu()
    rag, off = m.forward_taps_ragged(list(x), [(1, "value")])
    rag = rag.cpu()
    err = float((uni - rag).abs().max())
    print(f"[{mode}] ragged vs uniform: max-abs {err:.2e}")
    assert off.cpu().tolist() == [i * 16 * 22 for i in range(5)]
    assert torch.equal(uni, rag), err


def test_ragged_ffn_bound_rerun_is_per_image(case, monkeypatch):
    """The FFN-bound check inside a ragged call: with the threshold set between the images' own figures, only the image
    above it is run again with exact blocks and ffn_exact_blocks names them.  Its rows are bit for bit those of a ragged call
    with exactly those blocks forced exact; every other image's rows are bit for bit those of the call where nothing
    tripped; every image meets the oracle bar."""
    from anyloc_amd import extractor as ex
    m = case.model("h3")
    n = len(case.imgs)
    taps = [(1, "token")]
    base, offsets = m.forward_taps_ragged(case.imgs, taps)
    base = base.clone()
    assert m.ffn_exact_blocks == set()
    per_img = m._telemetry[:2 * n].cpu().reshape(2, n)
    fig = per_img.max(dim=0).values
    order = torch.argsort(fig)
    if not fig[order[-2]] < fig[order[-1]]:
        pytest.skip("the two loosest images' figures coincide")
    thr = float(0.5 * (fig[order[-2]] + fig[order[-1]]))
    top = int(order[-1])
    want_blocks = {int(l) for l in torch.nonzero(per_img[:, top] > thr).flatten()}
    # the re-run's own conditions: no telemetry, exactly those blocks exact
    m.ffn_check = False
    try:
        exact = []
        m._with_exact(sorted(want_blocks), lambda: exact.append(m.forward_taps_ragged(case.imgs, taps)[0].clone()))
    finally:
        m.ffn_check = True
    exact = exact[0]
    monkeypatch.setattr(ex, "FFN_LOOSENESS_MAX", thr)
    runs0 = m.ffn_reruns
    packed, offsets = m.forward_taps_ragged(case.imgs, taps)
    assert m.ffn_reruns - runs0 == 1
    assert m.ffn_exact_blocks == want_blocks and want_blocks
    off = offsets.cpu().tolist()
    for i in range(n):
        got = packed[off[i]:off[i + 1]]
        want = exact[off[i]:off[i + 1]] if i == top else base[off[i]:off[i + 1]]
        assert torch.equal(got, want), i
    print("tripped image: exact-block rows differ from the bound-quantised ones:",
          not torch.equal(exact[off[top]:off[top + 1]], base[off[top]:off[top + 1]]))
    _check_rows(packed, offsets, [case.oracle(x, 1, "token") for x in case.imgs])


# ---------------------------------------------------------------- end to end ----

def test_describe_images_matches_the_demo_loop():
    """describe_images on mixed uint8 images (two above max_img_size) = the demo's per-image loop on the same library
    (images_to_input -> extractor(img) -> vlad.generate): the same hard cluster ids, VLADs within 1e-5; the top-20 lists
    of a retrieval over the descriptors equal a float64 search."""
    import utilities
    from anyloc_amd import ops, preprocess
    from anyloc_amd.describe import describe_images
    name = "dinov2_vits14"
    sd = synth.synthetic_state_dict(name, 41, depth=3)
    weights.register_state_dict(name, {k: v.to(DEV) for k, v in sd.items()})
    try:
        ext = utilities.DinoV2ExtractFeatures(name, 2, "value", device=DEV)
        rng = np.random.default_rng(3)
        shapes = [(240, 320), (300, 200), (500, 380), (224, 224), (610, 470), (150, 290)] * 5
        images = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in shapes]
        max_img = 448
        per = [ext(preprocess.images_to_input(im, max_img_size=max_img))[0] for im in images]
        vlad = utilities.VLAD(8, None, cache_dir=None)
        utilities.seed_everything(42)
        vlad.fit(torch.cat(per[:6]).cpu())
        loop = torch.stack([vlad.generate(t) for t in per]).cpu()
        got = describe_images(ext, vlad, images, max_img_size=max_img).cpu()
        assert got.shape == loop.shape
        # hard cluster ids of every token: the ragged tokens against the per-image ones
        flat, sizes = preprocess.images_to_input_ragged(images, max_img)
        packed, offsets = ext.extract_ragged((flat, sizes), packed=True)
        c = vlad._centers_dev()
        _, lab_r = ops.vlad((packed, offsets), c, return_labels=True, dist_mode=vlad.mode)
        _, lab_l = ops.vlad(per, c, return_labels=True, dist_mode=vlad.mode)
        assert torch.equal(lab_r.cpu(), lab_l.cpu())
        err = float((got - loop).abs().max())
        print(f"describe_images vs demo loop: VLAD max-abs {err:.2e}")
        assert err <= 1e-5
        q, db = got[:10], got[10:]
        top = ops.topk(q.to(DEV), db.to(DEV), 20)[1].cpu()
        s64 = q.double() @ db.double().t()
        ref = torch.argsort(-s64, dim=1, stable=True)[:, :20]
        assert torch.equal(top.to(torch.int64), ref)
    finally:
        weights.unregister_state_dict(name)
