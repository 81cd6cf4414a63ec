"""DINOv2 with registers (``dinov2_vit*14_reg``) on the HIP forward, against the float64 restatement of
``tests/_reg_restatement.py`` (GPU box only).

Tolerances are those of test_gpu_fullsize_parity.py: unit-norm tokens within 2e-5 max-abs of the fp32 restatement, and
within 3x + 1e-7 of the fp32 restatement's own distance to float64 -- in all three block arithmetics.  The sizes put the
register rows where they matter: 210 x 238 has 255 patches, so T goes 256 -> 260 and the four registers alone carry the
sequence across a 64-row tile; B = 1 runs the small-M plans."""
import os
import sys

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from anyloc_amd import synth, weights
from oracle import vlad_ref

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _reg_restatement as regref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ("h3", "x6", "f32")
TOKEN_ATOL = 2e-5
GAP_TOL = 1e-6


def _images(hw, n, seed):
    g = torch.Generator().manual_seed(seed + 31 * hw[0] + hw[1])
    h, w = hw
    x = torch.randn(n, 3, max(1, h // 14), max(1, w // 14), generator=g)
    return (F.interpolate(x, size=(h, w), mode="bilinear", align_corners=False) + 0.3 * torch.randn(n, 3, h, w, generator=g))


class RegCase:
    """One _reg model: the restatement in fp32 and float64 (per-image hooked outputs cached) and the HIP model per
    arithmetic."""

    def __init__(self, name, depth, seed, layers, stress=False):
        torch.set_num_threads(max(1, min(16, torch.get_num_threads() * 2)))
        self.name, self.depth, self.layers = name, depth, sorted(set(layers))
        sd = synth.synthetic_state_dict(name, seed, depth=depth)
        self.sd = synth.outlier_state_dict(sd, name, seed + 1) if stress else sd
        self.R = synth.n_registers(name)
        self.ref = {torch.float32: regref.build(name, self.sd, depth, torch.float32),
                    torch.float64: regref.build(name, self.sd, depth, torch.float64)}
        self._raw, self._models = {}, {}

    def model(self, mode):
        from anyloc_amd.extractor import HipDinoV2
        if mode not in self._models:
            self._models[mode] = HipDinoV2(self.name, {k: v.to(DEV) for k, v in self.sd.items()}, torch.device(DEV), gemm=mode)
        return self._models[mode]

    def raw(self, img, dtype):
        key = (tuple(img.shape), float(img.flatten()[:64].double().sum()), dtype)
        if key not in self._raw:
            self._raw[key] = regref.hooked(self.ref[dtype], img[None].to(dtype), self.layers)
        return self._raw[key]

    def oracle(self, imgs, taps, use_cls=False, dtype=torch.float32):
        """[B, N(+1), len(taps)*D]: each image alone (B = 1, the reference's calling convention); several taps are
        concatenated in the given order and normalised again (norm_concat)."""
        outs = []
        for im in imgs:
            raw = self.raw(im, dtype)
            t = torch.cat([regref.tap(raw, l, f, self.R, use_cls)[0] for l, f in taps], dim=-1)
            outs.append(F.normalize(t, dim=-1) if len(taps) > 1 else t)
        return torch.stack(outs)

    def check(self, got, imgs, taps, use_cls=False, what=""):
        ref32 = self.oracle(imgs, taps, use_cls, torch.float32)
        ref64 = self.oracle(imgs, taps, use_cls, torch.float64)
        got = got.cpu()
        assert got.shape == ref32.shape, (what, got.shape, ref32.shape)
        err = float((got - ref32).abs().max())
        err64 = float((got.double() - ref64).abs().max())
        err32 = float((ref32.double() - ref64).abs().max())
        print(f"[{self.name} {what}] err vs fp32 {err:.2e}, vs float64 {err64:.2e} (fp32 restatement {err32:.2e})")
        assert err <= TOKEN_ATOL, (what, err)
        assert err64 <= 3.0 * err32 + 1e-7, (what, err64, err32)


_CASES = {}


def _case(key):
    if key not in _CASES:
        if key == "s":
            _CASES[key] = RegCase("dinov2_vits14_reg", 12, 11, [5, 11])
        elif key == "g4":
            _CASES[key] = RegCase("dinov2_vitg14_reg", 4, 13, [1, 3])
        elif key == "g4_stress":
            _CASES[key] = RegCase("dinov2_vitg14_reg", 4, 17, [3], stress=True)
    return _CASES[key]


# ---------------------------------------------------------------- ViT-S_reg, full depth ----

S_COMBOS = [((224, 224), "query", False), ((322, 322), "key", True), ((518, 518), "value", False),
            ((476, 630), "token", True), ((210, 238), "token", False), ((210, 238), "value", True)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hw,facet,use_cls", S_COMBOS)
def test_vits_reg_full_depth(mode, hw, facet, use_cls):
    """Every facet, with and without the CLS row, at B = 2 and B = 1: the patch rows (and CLS), never a register row."""
    c = _case("s")
    m = c.model(mode)
    imgs = _images(hw, 2, 1)
    taps = [(11, facet)]
    got2 = m.forward_taps(imgs.to(DEV), taps, use_cls=use_cls)
    n = (hw[0] // 14) * (hw[1] // 14)
    assert got2.shape == (2, n + (1 if use_cls else 0), 384)
    c.check(got2, imgs, taps, use_cls, f"{mode} {hw} {facet} cls={use_cls} B=2")
    got1 = m.forward_taps(imgs[:1].to(DEV), taps, use_cls=use_cls)
    c.check(got1, imgs[:1], taps, use_cls, f"{mode} {hw} {facet} cls={use_cls} B=1")


def test_vits_reg_model_call_and_extractor(monkeypatch):
    """``hub_load`` / ``HipDinoV2.__call__`` (final LayerNorm of CLS) and ``utilities.DinoV2ExtractFeatures`` with a _reg
    name; the extractor's multi-tap call with two layers out of order and norm_concat."""
    import utilities
    from anyloc_amd import extractor
    c = _case("s")
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url",
                        lambda *a, **k: (_ for _ in ()).throw(RuntimeError("no download in tests")))
    weights.register_state_dict(c.name, c.sd)
    try:
        model = extractor.hub_load("facebookresearch/dinov2", c.name).eval().to(DEV)
        imgs = _images((224, 308), 3, 2)
        got = model(imgs.to(DEV)).cpu()
        with torch.no_grad():
            want = c.ref[torch.float32](imgs)
        assert got.shape == (3, 384)
        err = float((got - want).abs().max())
        print(f"model call: max-abs {err:.2e} (scale {float(want.abs().max()):.2f})")
        assert err < 2e-5 * float(want.abs().max())
        ext = utilities.DinoV2ExtractFeatures(c.name, 11, "value", device=DEV)
        got = ext(imgs.to(DEV))
        c.check(got, imgs, [(11, "value")], False, "extractor")
        multi = ext.extract_multi(imgs.to(DEV), [11, 5], "key", norm_concat=True)
        c.check(multi, imgs, [(11, "key"), (5, "key")], False, "extract_multi 11,5")
    finally:
        weights.unregister_state_dict(c.name)


# ---------------------------------------------------------------- ViT-g_reg (SwiGLU), 4 blocks ----

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hw", [(224, 224), (210, 238), (322, 322)])
def test_vitg_reg_four_blocks(mode, hw):
    c = _case("g4")
    m = c.model(mode)
    imgs = _images(hw, 2, 3)
    for B in (2, 1):
        got = m.forward_taps(imgs[:B].to(DEV), [(3, "value")])
        c.check(got, imgs[:B], [(3, "value")], False, f"{mode} {hw} B={B}")


@pytest.mark.parametrize("mode", MODES)
def test_vitg_reg_two_taps_out_of_order_norm_concat(mode):
    c = _case("g4")
    m = c.model(mode)
    imgs = _images((210, 238), 2, 3)
    taps = [(3, "token"), (1, "key")]
    got = m.forward_taps(imgs.to(DEV), taps, use_cls=True, norm_concat=True)
    c.check(got, imgs, taps, True, f"{mode} taps 3,1 norm_concat")


def test_vitg_reg_outlier_weights_and_ffn_rerun(monkeypatch):
    """The outlier-weight stress on a _reg model in the h3 arithmetic: as it comes, and with the FFN-bound threshold at 0 so
    that every image is run again with its blocks on the exact quantiser -- the re-run's rows meet the same bar."""
    from anyloc_amd import extractor as ex
    c = _case("g4_stress")
    m = c.model("h3")
    imgs = _images((322, 322), 2, 5)
    got = m.forward_taps(imgs.to(DEV), [(3, "token")])
    c.check(got, imgs, [(3, "token")], False, "stress h3")
    monkeypatch.setattr(ex, "FFN_LOOSENESS_MAX", 0.0)
    runs0 = m.ffn_reruns
    got = m.forward_taps(imgs.to(DEV), [(3, "token")])
    assert m.ffn_reruns - runs0 == 2 and m.ffn_exact_blocks
    c.check(got, imgs, [(3, "token")], False, "stress h3, every image re-run")


# ---------------------------------------------------------------- ViT-g_reg, full depth ----

@pytest.fixture(scope="module")
def vitg_full():
    """ViT-g/14_reg, all 40 blocks, one 322 x 322 image: the restatement's tokens at layer 39 in fp32 and float64."""
    name = "dinov2_vitg14_reg"
    sd = synth.synthetic_state_dict(name, 19)
    img = _images((322, 322), 1, 7)
    refs = {}
    for dtype in (torch.float32, torch.float64):
        model = regref.build(name, sd, 40, dtype)
        refs[dtype] = regref.tap(regref.hooked(model, img.to(dtype), [39]), 39, "token", 4)
        del model
    return name, sd, img, refs


@pytest.mark.parametrize("mode", MODES)
def test_vitg_reg_full_depth_322(vitg_full, mode):
    from anyloc_amd.extractor import HipDinoV2
    name, sd, img, refs = vitg_full
    m = HipDinoV2(name, {k: v.to(DEV) for k, v in sd.items()}, torch.device(DEV), gemm=mode)
    got = m.forward_taps(img.to(DEV), [(39, "token")]).cpu()
    del m
    assert got.shape == refs[torch.float32].shape == (1, 529, 1536)
    err = float((got - refs[torch.float32]).abs().max())
    err64 = float((got.double() - refs[torch.float64]).abs().max())
    err32 = float((refs[torch.float32].double() - refs[torch.float64]).abs().max())
    print(f"[vitg_reg full {mode}] err vs fp32 {err:.2e}, vs float64 {err64:.2e} (fp32 restatement {err32:.2e})")
    assert err <= TOKEN_ATOL
    assert err64 <= 3.0 * err32 + 1e-7


# ---------------------------------------------------------------- ragged batches ----

RAGGED_SIZES = [(224, 224), (210, 238), (14, 28), (476, 630), (322, 322), (210, 238)]


def _ragged_imgs():
    return [_images(hw, 1, 9 + i)[0] for i, hw in enumerate(RAGGED_SIZES)]


def _check_ragged(c, packed, offsets, imgs, taps, use_cls, what):
    off = offsets.cpu().tolist()
    rows = [(h // 14) * (w // 14) + (1 if use_cls else 0) for h, w in RAGGED_SIZES]
    assert off == [0] + np.cumsum(rows).tolist()
    for i, im in enumerate(imgs):
        c.check(packed[off[i]:off[i + 1]][None], [im], taps, use_cls, f"{what} image {i} {RAGGED_SIZES[i]}")


@pytest.mark.parametrize("mode", MODES)
def test_ragged_reg_vs_restatement(mode):
    c = _case("s")
    m = c.model(mode)
    imgs = _ragged_imgs()
    packed, offsets = m.forward_taps_ragged(imgs, [(11, "value")])
    _check_ragged(c, packed, offsets, imgs, [(11, "value")], False, f"ragged {mode}")


@pytest.mark.parametrize("facet", ["token", "query"])
def test_ragged_reg_with_cls(facet):
    c = _case("s")
    m = c.model("h3")
    imgs = _ragged_imgs()
    packed, offsets = m.forward_taps_ragged(imgs, [(11, facet)], use_cls=True)
    _check_ragged(c, packed, offsets, imgs, [(11, facet)], True, f"ragged cls {facet}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("use_cls", [False, True])
def test_ragged_reg_equal_sizes_match_the_uniform_forward(mode, use_cls):
    c = _case("s")
    m = c.model(mode)
    x = _images((210, 238), 3, 21).to(DEV)
    uni = m.forward_taps(x, [(11, "value")], use_cls=use_cls)
    rag, off = m.forward_taps_ragged(list(x), [(11, "value")], use_cls=use_cls)
    n = 255 + (1 if use_cls else 0)
    assert off.cpu().tolist() == [i * n for i in range(4)]
    assert torch.equal(uni.reshape(-1, 384).cpu(), rag.cpu())


# ---------------------------------------------------------------- end to end ----

def test_describe_images_with_registers():
    """describe_images with a _reg extractor = the demo's per-image loop on the same library; a K=32 VLAD over the
    restatement's tokens of the same inputs gives the same hard cluster ids, except at fp32 ties."""
    import utilities
    from anyloc_amd import ops, preprocess
    from anyloc_amd.describe import describe_images
    name = "dinov2_vits14_reg"
    sd = synth.synthetic_state_dict(name, 41, depth=3)
    weights.register_state_dict(name, {k: v.to(DEV) for k, v in sd.items()})
    try:
        ext = utilities.DinoV2ExtractFeatures(name, 2, "value", device=DEV)
        rng = np.random.default_rng(3)
        shapes = [(240, 320), (300, 200), (500, 380), (224, 224), (610, 470), (150, 290)] * 2
        images = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in shapes]
        max_img = 448
        inputs = [preprocess.images_to_input(im, max_img_size=max_img) for im in images]
        per = [ext(x)[0] for x in inputs]
        vlad = utilities.VLAD(32, None, cache_dir=None)
        utilities.seed_everything(42)
        vlad.fit(torch.cat(per).cpu())
        loop = torch.stack([vlad.generate(t) for t in per]).cpu()
        got = describe_images(ext, vlad, images, max_img_size=max_img).cpu()
        assert got.shape == loop.shape
        err = float((got - loop).abs().max())
        print(f"describe_images vs demo loop: VLAD max-abs {err:.2e}")
        assert err <= 1e-5
        # the restatement's tokens of the same inputs, and the cluster ids of both
        ref = regref.build(name, sd, 3, torch.float32)
        centers = vlad._centers_dev().cpu()
        for x, t in zip(inputs, per):
            want = regref.tap(regref.hooked(ref, x.cpu(), [2]), 2, "value", 4)[0]
            assert float((t.cpu() - want).abs().max()) <= TOKEN_ATOL
            _, lab = ops.vlad(t[None], centers.to(DEV), return_labels=True)
            lab = lab.cpu().reshape(-1)
            lab_ref = vlad_ref.vlad_hard(want, centers)[1]
            flips = lab != lab_ref
            if flips.any():
                sc = vlad_ref.fpk_cosine_scores(want[flips], centers).topk(2, dim=1)[0]
                gap = float((sc[:, 0] - sc[:, 1]).max())
                assert gap < GAP_TOL, f"{int(flips.sum())} cluster-id flips, largest restatement gap {gap:.3e}"
    finally:
        weights.unregister_state_dict(name)
