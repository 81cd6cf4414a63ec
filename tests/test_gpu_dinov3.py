"""DINOv3 (``dinov3_vit*16``: rotary positions, patch 16, four registers, LayerNorm eps 1e-5) on the HIP forward, against
the restatement of ``tests/_dinov3_restatement.py`` (GPU box only; ``tests/test_dinov3_cpu.py`` holds that restatement
against ``transformers`` in float64).

Bars: unit-norm tokens within 2e-5 max-abs of the fp32 restatement, and no further from the float64
restatement than 3 x the fp32 restatement's own distance + 1e-7.  The second bar is the one that sees a wrong eps (1e-6 for
1e-5 moves the tokens by ~1.5e-5: under the first bar, far over the second); a missing rotation moves them by 6e-3, a
rotated prefix row by 3e-3."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from anyloc_amd import synth, weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dinov3_restatement as v3ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOKEN_ATOL = 2e-5
GAP_TOL = 1e-6
FACETS = ("value", "query", "key", "token")
# the block arithmetics; "h3_nofuse" = h3 with option h3_fuse = 0 (q | k | v, attention output and FFN activation in fp32)
MODES = ("h3", "x6", "f32", "h3_nofuse")


@pytest.fixture(autouse=True)
def _cpu_threads_and_rng():
    """The oracle runs on the CPU: at most 16 threads, whatever a module imported at collection set torch to (the machine's
    CPU count oversubscribes a box that grants 16 and stalls every parallel region).  And the process-wide random states
    (python, NumPy, torch) leave every test as they entered it: the seeding of the end-to-end test would otherwise hand the
    tests that run later in the session, some of which draw from NumPy's global generator, another stream than they get
    without this file."""
    import random
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    state = (random.getstate(), np.random.get_state(), torch.get_rng_state(),
             torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None)
    yield
    random.setstate(state[0])
    np.random.set_state(state[1])
    torch.set_rng_state(state[2])
    if state[3] is not None:
        torch.cuda.set_rng_state_all(state[3])


def _images(hw, n, seed):
    g = torch.Generator().manual_seed(seed + 31 * hw[0] + hw[1])
    h, w = hw
    x = torch.randn(n, 3, max(1, h // 16), max(1, w // 16), generator=g)
    return F.interpolate(x, size=(h, w), mode="bilinear", align_corners=False) + 0.3 * torch.randn(n, 3, h, w, generator=g)


class mode_options:
    """The process-wide options a mode needs, put back on exit."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from anyloc_amd import ops
        self.prev = ops.get_option("h3_fuse")
        if self.mode == "h3_nofuse":
            ops.set_option("h3_fuse", 0)

    def __exit__(self, *exc):
        from anyloc_amd import ops
        ops.set_option("h3_fuse", self.prev)


class V3Case:
    """One model: the restatement in fp32 and float64 (hooked outputs cached per image batch) and the HIP model per
    arithmetic."""

    def __init__(self, name, depth, seed, layers, sd=None):
        self.name, self.depth, self.layers = name, depth, sorted(set(layers))
        self.sd = synth.synthetic_state_dict(name, seed, depth=depth) if sd is None else sd
        self.R = synth.n_registers(name)
        self.dim = synth.ARCH[name][0]
        self.ref = {dt: v3ref.Model(self.sd, depth, dt) for dt in (torch.float32, torch.float64)}
        self._raw, self._models = {}, {}

    def model(self, mode):
        from anyloc_amd.extractor import HipDinoV2
        gemm = "h3" if mode == "h3_nofuse" else mode
        if gemm not in self._models:
            self._models[gemm] = HipDinoV2(self.name, {k: v.to(DEV) for k, v in self.sd.items()}, torch.device(DEV), gemm=gemm)
        return self._models[gemm]

    def raw(self, imgs, dtype):
        """The restatement's hooked outputs of a batch of equal-sized images (the restatement treats every image of a batch
        on its own: no image attends to another)."""
        key = (tuple(imgs.shape), float(imgs.flatten()[:64].double().sum()), float(imgs.flatten()[-64:].double().sum()), dtype)
        if key not in self._raw:
            self._raw[key] = self.ref[dtype].hooked(imgs, self.layers)
        return self._raw[key]

    def oracle(self, imgs, taps, use_cls, dtype):
        raw = self.raw(imgs, dtype)
        t = torch.cat([v3ref.tap(raw, l, f, self.R, use_cls) for l, f in taps], dim=-1)
        return F.normalize(t, dim=-1) if len(taps) > 1 else t

    def check(self, got, imgs, taps, use_cls=False, what="", norm_concat=True):
        if len(taps) > 1 and not norm_concat:
            refs = [torch.cat([v3ref.tap(self.raw(imgs, dt), l, f, self.R, use_cls) for l, f in taps], dim=-1)
                    for dt in (torch.float32, torch.float64)]
        else:
            refs = [self.oracle(imgs, taps, use_cls, dt) for dt in (torch.float32, torch.float64)]
        ref32, ref64 = refs
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
            _CASES[key] = V3Case("dinov3_vits16", 3, 11, [1, 2])
        elif key == "splus":
            _CASES[key] = V3Case("dinov3_vits16plus", 3, 13, [1, 2])
        elif key == "s2":
            _CASES[key] = V3Case("dinov3_vits16", 2, 17, [1])
        elif key == "hplus":
            _CASES[key] = V3Case("dinov3_vith16plus", 2, 19, [1])
    return _CASES[key]


# ---------------------------------------------------------------- 1. extractor parity ----

# B = 2 at 48 x 80: T = 20, image 1 starts inside image 0's 32-row group and its prefix rows share a tile with rotated rows;
# B = 3 at 112 x 160: T = 75, 225 rows cross a 128-row tile and leave a partial last one; B = 1 at 16 x 16: one patch
SHAPES = [(2, (48, 80)), (3, (112, 160)), (1, (16, 16))]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,hw", SHAPES)
@pytest.mark.parametrize("key", ["s", "splus"])
def test_extractor_parity(key, B, hw, mode):
    c = _case(key)
    m = c.model(mode)
    imgs = _images(hw, B, 1)
    n = (hw[0] // 16) * (hw[1] // 16)
    with mode_options(mode):
        for facet in FACETS:
            for use_cls in (False, True):
                got = m.forward_taps(imgs.to(DEV), [(2, facet)], use_cls=use_cls)
                assert got.shape == (B, n + (1 if use_cls else 0), 384)
                c.check(got, imgs, [(2, facet)], use_cls, f"{mode} B={B} {hw} {facet} cls={use_cls}")


# ---------------------------------------------------------------- 2. every route of the qkv epilogue ----

# batch of 224 x 224 images (T = 201) -> the (route, tile rows, tile cols, ring depth) the plan function gives the qkv GEMM of
# ViT-S (N = 1152, K = 384) in the fused forward (split-K workspace at hand, a LayerNorm in front); each batch is the smallest
# that lands there: the small-M table's three tile shapes (one of them on both ring depths) and the batched 128 x 256 kernel
H3_ROUTE_SMALL, H3_ROUTE_BATCHED = 0, 2
QKV_PLANS = {1: (H3_ROUTE_SMALL, 64, 64, 6), 3: (H3_ROUTE_SMALL, 64, 128, 6), 9: (H3_ROUTE_SMALL, 64, 64, 3),
             18: (H3_ROUTE_SMALL, 128, 128, 3), 65: (H3_ROUTE_BATCHED, 128, 256, 3)}


def _qkv_plan(B):
    from anyloc_amd import _lib
    d = _lib.H3PlanDesc()
    _lib.check(_lib.load().anyloc_h3_plan_describe(201 * B, 1152, 384, b"qkv_planes", 1,
                                                   _lib.H3_PLAN_SPLIT_WS | _lib.H3_PLAN_LN_IN_FRONT, C.byref(d)), "plan")
    return (d.route, d.tile_rows, d.tile_cols, d.stages)


@pytest.mark.parametrize("B", sorted(QKV_PLANS))
def test_every_qkv_route_rotates(B):
    """2 blocks, token at layer 1, one batch per distinct (route, tile) of the qkv epilogue; the host asserts first that the
    batch lands where it is meant to, that no smaller batch does, and that the table holds every plan up to the largest."""
    assert _qkv_plan(B) == QKV_PLANS[B]
    assert all(_qkv_plan(b) != QKV_PLANS[B] for b in range(1, B))
    assert {_qkv_plan(b) for b in range(1, max(QKV_PLANS) + 1)} == set(QKV_PLANS.values())
    c = _case("s2")
    m = c.model("h3")
    imgs = _images((224, 224), B, 5)
    got = m.forward_taps(imgs.to(DEV), [(1, "token")])
    c.check(got, imgs, [(1, "token")], False, f"plan {QKV_PLANS[B]} B={B} M={201 * B}")


def _v3_gemms():
    """the block GEMMs of dinov3_vits16 as the fused forward launches them (the rotating qkv epilogue has the plans of
    "qkv_planes": csrc/common.hpp plan_epilogue)"""
    import _plan_edges as pe
    return pe, _lib_handle(), pe.block_gemms("dinov3_vits16")


def _lib_handle():
    from anyloc_amd import _lib
    return _lib.load()


def _token_forward(c, imgs, what, check=True):
    """layer-1 tokens of the 2-block model on the h3 kernels, without the FFN re-run that would hide which kernels produced
    them; held to the restatement under the bars of test_every_qkv_route_rotates"""
    m = c.model("h3")
    prev, m.ffn_check = m.ffn_check, False
    try:
        got = m.forward_taps(imgs.to(DEV), [(1, "token")]).clone()
    finally:
        m.ffn_check = prev
    if check:
        c.check(got, imgs, [(1, "token")], False, what)
    return got


@pytest.mark.parametrize("B", [1, 3])
def test_every_small_m_plan_rotates(B):
    """The rotating qkv epilogue on every small-M kernel (tile x k-blocks per stage x ring depth), where
    test_every_qkv_route_rotates meets the table's choices only: the forced plans of
    tests/test_gpu_vit.py::test_small_m_plans_agree_with_the_plain_kernels on one and three 224 x 224 images (201 and 603
    rows), each held to the restatement under this file's bars and bit-identical on a second run; a combination the plan
    refuses is asserted as a refusal and not launched."""
    from anyloc_amd import ops
    pe, lib, gemms = _v3_gemms()
    c = _case("s2")
    imgs = _images((224, 224), B, 5)
    launched = 0
    for forced in pe.FORCED_PLANS:
        cfg, kb, ks, st = forced
        with ops.options(h3s_cfg=cfg, h3s_kb=kb, h3s_ksplit=ks, h3s_stages=st):
            if not pe.forced_plan_is_served(lib, 201 * B, gemms, forced):
                continue
            got = _token_forward(c, imgs, f"forced plan {forced} B={B}")
            assert torch.equal(got, _token_forward(c, imgs, "", check=False)), (forced, "not reproducible")
        launched += 1
    assert launched == len(pe.FORCED_PLANS) - len(pe.REFUSED_PLANS) == 32


@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5])
def test_every_batched_tile_rotates(cfg):
    """Option h3_cfg = 1 ... 5 sends every GEMM to kH3Tile[cfg] at every size: the rotating qkv epilogue on those five tiles (three
    224 x 224 images, 603 rows: a partial last tile of 128 and of 256 rows), held to the restatement."""
    from anyloc_amd import ops
    pe, lib, gemms = _v3_gemms()
    c = _case("s2")
    imgs = _images((224, 224), 3, 5)
    with ops.options(h3_cfg=cfg):
        d = pe.describe(lib, 603, *gemms["qkv"])
        assert (d["route"], d["tile"], d["lead"]) == (H3_ROUTE_BATCHED, cfg, 0), d
        _token_forward(c, imgs, f"h3_cfg {cfg}")


@pytest.mark.parametrize("B", [1, 65])
def test_layernorm_lead_role_in_front_of_the_rotating_epilogue(B):
    """LayerNorm 1 as the lead role of the qkv GEMM's own launch with the rotating epilogue: one image (option h3s_ln_lead, on the
    one plan the small-M role is compiled for -- 128 x 128 tiles, 6-deep ring, forced on the qkv GEMM alone, since ViT-S's
    narrow qkv is not given that plan by the table) and 65 images (option h3_ln_lead, the batched role).  The library's plan
    must name the role; the tokens must be the bits of the separate launches -- the bar of
    tests/test_gpu_round6.py::test_layernorm_lead_role_gives_the_bits_of_the_separate_launch -- and meet the restatement."""
    from anyloc_amd import ops
    pe, lib, gemms = _v3_gemms()
    c = _case("s2")
    imgs = _images((224, 224), B, 5)
    plan = dict(h3s_mask=1, h3s_cfg=4, h3s_kb=1, h3s_ksplit=1, h3s_stages=6) if B == 1 else {}
    lead = "h3s_ln_lead" if B == 1 else "h3_ln_lead"
    with ops.options(**plan):
        with ops.options(**{lead: 0}):
            assert pe.describe(lib, 201 * B, *gemms["qkv"])["lead"] == 0
            want = _token_forward(c, imgs, f"separate LayerNorm B={B}")
        with ops.options(**{lead: 1}):
            d = pe.describe(lib, 201 * B, *gemms["qkv"])
            assert d["lead"] == (1 if B == 1 else 2), d
            for rep in range(5):
                assert torch.equal(_token_forward(c, imgs, "", check=False), want), (B, rep, "the lead-role forward differs")


# ---------------------------------------------------------------- 3. taps are pre-rotation, later layers see the rotation ----

@pytest.mark.parametrize("mode", MODES)
def test_tapped_layer_keeps_pre_rotation_facets(mode):
    c = _case("s")
    m = c.model(mode)
    imgs = _images((48, 80), 2, 3)
    taps = [(1, "query"), (1, "key"), (2, "token")]
    with mode_options(mode):
        got = m.forward_taps(imgs.to(DEV), taps, norm_concat=False)
    c.check(got, imgs, taps, False, f"{mode} taps q1 k1 t2", norm_concat=False)


# ---------------------------------------------------------------- 4. ragged ----

RAGGED_SIZES = [(48, 80), (80, 48), (112, 160), (16, 16), (48, 80)]


@pytest.mark.parametrize("mode", ["h3", "x6", "f32"])
def test_ragged_vs_restatement(mode):
    c = _case("s")
    m = c.model(mode)
    imgs = [_images(hw, 1, 9 + i)[0] for i, hw in enumerate(RAGGED_SIZES)]
    for facet, use_cls in (("token", False), ("key", True)):
        packed, offsets = m.forward_taps_ragged(imgs, [(2, facet)], use_cls=use_cls)
        off = offsets.cpu().tolist()
        rows = [(h // 16) * (w // 16) + (1 if use_cls else 0) for h, w in RAGGED_SIZES]
        assert off == [0] + np.cumsum(rows).tolist()
        for i, im in enumerate(imgs):
            c.check(packed[off[i]:off[i + 1]][None], im[None], [(2, facet)], use_cls, f"ragged {mode} {facet} image {i} {RAGGED_SIZES[i]}")


@pytest.mark.parametrize("mode", ["h3", "x6", "f32"])
@pytest.mark.parametrize("use_cls", [False, True])
def test_ragged_equal_sizes_match_the_uniform_forward(mode, use_cls):
    c = _case("s")
    m = c.model(mode)
    x = _images((112, 160), 3, 21).to(DEV)
    uni = m.forward_taps(x, [(2, "token")], use_cls=use_cls)
    rag, off = m.forward_taps_ragged(list(x), [(2, "token")], use_cls=use_cls)
    n = 70 + (1 if use_cls else 0)
    assert off.cpu().tolist() == [i * n for i in range(4)]
    assert torch.equal(uni.reshape(-1, 384).cpu(), rag.cpu())


# ---------------------------------------------------------------- 5. rope_rows alone ----

def _rope_rows_f64(qkv, table, tok_off, prefix, heads):
    """The formula in float64 on fp32 inputs; tok_off: row offsets of the images, tables packed in the same order."""
    out = qkv.double().clone()
    D = heads * 64
    at = 0
    for i in range(len(tok_off) - 1):
        r0, r1 = tok_off[i] + prefix, tok_off[i + 1]
        n = r1 - r0
        cos, sin = table[at:at + n, :32].double()[:, None, :], table[at:at + n, 32:].double()[:, None, :]
        at += n
        x = out[r0:r1, :2 * D].reshape(n, 2 * heads, 64).clone()
        a, b = x[..., :32].clone(), x[..., 32:].clone()
        x[..., :32] = a * cos - b * sin
        x[..., 32:] = b * cos + a * sin
        out[r0:r1, :2 * D] = x.reshape(n, 2 * D)
    return out


@pytest.mark.parametrize("ragged", [False, True])
def test_rope_rows_alone(ragged):
    """Two fp32 products and one sum per element: within 2e-7 of the row's largest magnitude of the float64 formula (each
    product rounds to 2^-24 relative, the sum once more: 1.5 * 2^-23 = 1.8e-7 of the larger operand); the prefix rows and
    the v third keep their bits."""
    from anyloc_amd import ops
    from anyloc_amd.extractor import ragged_offsets, rope_table
    heads, D = 6, 384
    g = torch.Generator().manual_seed(4)
    if ragged:
        sizes = [(48, 80), (16, 16), (80, 48), (48, 80)]
        tok, _, _ = ragged_offsets(sizes, False, patch=16, registers=4)
        tables = [rope_table(*hw) for hw in sizes]
        meta = np.zeros((5, len(sizes) + 1), dtype=np.int64)
        meta[0] = tok
        meta[2, :len(sizes)] = np.cumsum([0] + [t.shape[0] for t in tables])[:-1]
        table = torch.cat(tables)
        tok = tok.tolist()
    else:
        tok = [0, 20, 40, 60]
        table = rope_table(48, 80)
    M = tok[-1]
    qkv = torch.randn(M, 3 * D, generator=g) * (1.0 + 3.0 * torch.rand(M, 1, generator=g))
    if ragged:
        got = ops.rope_rows(qkv.to(DEV), heads, table.to(DEV), prefix=5, meta=torch.from_numpy(meta)).cpu()
        packed = table
    else:
        got = ops.rope_rows(qkv.to(DEV), heads, table.to(DEV), tokens=20, prefix=5).cpu()
        packed = torch.cat([table] * 3)
    want = _rope_rows_f64(qkv, packed, tok, 5, heads)
    assert torch.equal(got[:, 2 * D:], qkv[:, 2 * D:])                   # v
    for i in range(len(tok) - 1):
        assert torch.equal(got[tok[i]:tok[i] + 5], qkv[tok[i]:tok[i] + 5])      # CLS and the registers
    rel = ((got.double() - want).abs().amax(dim=1) / qkv.abs().amax(dim=1).double())
    print(f"rope_rows ragged={ragged}: worst row error {float(rel.max()):.2e} of the row's largest magnitude")
    assert float(rel.max()) <= 2e-7
    # every patch row moved, but the centre patch of an odd x odd grid: its coordinates, hence its angles, are exactly zero
    still = (packed[:, :32] == 1).all(dim=1) & (packed[:, 32:] == 0).all(dim=1)
    assert int(still.sum()) == (4 if ragged else 3)
    moved = (got[:, :2 * D] != qkv[:, :2 * D]).any(dim=1)
    assert int(moved.sum()) == M - 5 * (len(tok) - 1) - int(still.sum())


# ---------------------------------------------------------------- 6. the new block shape ----

@pytest.mark.parametrize("mode", ["h3", "f32", "x6"])
def test_vith16plus_block_shape(mode):
    """D = 1280, 20 heads, gated mlp with hidden 5120: 2 blocks, B = 2 at 64 x 96 (x6: the only width with five float4 per lane in
    layernorm_x3_kernel)."""
    from anyloc_amd import ops
    c = _case("hplus")
    m = c.model(mode)
    imgs = _images((64, 96), 2, 7)
    with ops.options(**({"x6_min_rows": 0} if mode == "x6" else {})):       # (few rows would run the fp32 kernels under "x6")
        got = m.forward_taps(imgs.to(DEV), [(1, "token")])
    assert got.shape == (2, 24, 1280)
    c.check(got, imgs, [(1, "token")], False, f"vith16plus {mode}")


# ---------------------------------------------------------------- 7. the FFN-bound re-run rotates too ----

def test_ffn_bound_rerun_rotates():
    """A planted fc1 row trips the Cauchy-Schwarz bound of block 1 (as tests/test_gpu_vit.py plants it): every image is
    run again with that block on the exact quantiser, and the re-run's tokens meet the bars."""
    from anyloc_amd import extractor as ex
    name = "dinov3_vits16"
    sd = synth.synthetic_state_dict(name, 23, depth=3)
    w, b = sd["blocks.1.norm2.weight"].double(), sd["blocks.1.norm2.bias"].double()
    d = (1.0 / w) / (1.0 / w).norm()
    f1 = sd["blocks.1.mlp.fc1.weight"].double()
    c_ = 3000.0 * float(f1.norm(dim=1).max())
    f1[7] = c_ * d
    sd["blocks.1.mlp.fc1.weight"] = f1.float()
    sd["blocks.1.mlp.fc1.bias"][7] = float(-c_ * (d * b).sum())
    c = V3Case(name, 3, 23, [2], sd=sd)
    m = c.model("h3")
    imgs = _images((112, 160), 3, 2)
    got = m.forward_taps(imgs.to(DEV), [(2, "token")])
    assert m.ffn_looseness is not None and m.ffn_looseness[1] > ex.FFN_LOOSENESS_MAX, m.ffn_looseness
    assert m.ffn_exact_blocks == {1} and m.ffn_reruns == 3, (m.ffn_exact_blocks, m.ffn_reruns)
    c.check(got, imgs, [(2, "token")], False, "ffn re-run")


# ---------------------------------------------------------------- 8. end to end ----

def test_end_to_end_vlad_and_retrieval():
    """DinoV2ExtractFeatures("dinov3_vits16", 2, "value") -> VLAD(K = 8) fitted on its own tokens -> get_top_k_recall over 12
    images of 96 x 128, against the restatement's tokens through the oracle's VLAD and flat search."""
    # the classes `utilities` re-exports, taken from their own modules: importing `utilities` seeds every global generator
    # as a side effect of the import, and where in a session that first happens is not this file's to decide
    from anyloc_amd import ops
    from anyloc_amd.extractor import DinoV2ExtractFeatures
    from anyloc_amd.retrieval import get_top_k_recall
    from anyloc_amd.vlad import VLAD
    from oracle import vlad_ref
    name = "dinov3_vits16"
    sd = synth.synthetic_state_dict(name, 29, depth=3)
    weights.register_state_dict(name, {k: v.to(DEV) for k, v in sd.items()})
    try:
        ext = DinoV2ExtractFeatures(name, 2, "value", device=DEV)
        db, qu, gt = synth.synthetic_places(8, 4, 96, 128, seed=42)
        imgs = torch.cat([db, qu])
        toks = ext(imgs.to(DEV))
        assert toks.shape == (12, 48, 384)
        ref = v3ref.Model(sd, 3, torch.float32)
        want = v3ref.tap(ref.hooked(imgs, [2]), 2, "value", 4)
        assert float((toks.cpu() - want).abs().max()) <= TOKEN_ATOL
        vlad = VLAD(8, 384, cache_dir=None)
        np.random.seed(42)                  # k-means draws its first centres from NumPy's global generator
        torch.manual_seed(42)
        vlad.fit(toks.reshape(-1, 384).cpu())
        centers = vlad._centers_dev().cpu()
        v = vlad.generate_multi(toks).cpu()
        v_ref = torch.stack([vlad_ref.vlad_hard(t, centers)[0] for t in want])
        for t, w_ in zip(toks, want):
            _, lab = ops.vlad(t[None], centers.to(DEV), return_labels=True)
            lab = lab.cpu().reshape(-1)
            lab_ref = vlad_ref.vlad_hard(w_, centers)[1]
            flips = lab != lab_ref
            if flips.any():
                sc = vlad_ref.fpk_cosine_scores(w_[flips], centers).topk(2, dim=1)[0]
                gap = float((sc[:, 0] - sc[:, 1]).max())
                assert gap < GAP_TOL, f"{int(flips.sum())} cluster-id flips, largest restatement gap {gap:.3e}"
        rel = float(((v - v_ref).norm(dim=1) / v_ref.norm(dim=1)).max())
        print(f"end to end: VLAD rel err {rel:.2e}")
        assert rel <= 1e-5
        d, i, r = get_top_k_recall([1, 5], v[:8], v[8:], gt)
        d0, i0, r0 = vlad_ref.top_k_recall([1, 5], v_ref[:8], v_ref[8:], gt)
        assert np.array_equal(np.asarray(i)[:, :5], np.asarray(i0)[:, :5]) and r == r0
    finally:
        weights.unregister_state_dict(name)
