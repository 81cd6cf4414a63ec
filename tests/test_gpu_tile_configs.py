"""Every GEMM kernel that only an option can reach, against float64 and between guard bands.

Options gemm_f32_cfg, x6_cfg, h3_cfg, h3_group_m and h3_fast_silu select other compiled code than the defaults: wider tiles,
deeper or shallower rings, loads two slabs ahead, LDS-DMA staging, other workgroup -> tile maps, the exact SiLU.  The sweep
tools pick winners among exactly these values, and ANYLOC_OPTIONS makes them reachable by a user, so each value is held to
what the default kernels are held to:

  * the three direct entry points (anyloc_gemm_nt, anyloc_gemm_nt_x6, anyloc_gemm_nt_h3) under every value, with and without
    bias, the output in the arena of tests/_guard_arena.py with ldc in {N, N + 4}: no finding, and the float64 criterion of
    the family's own parity test (tests/test_gpu_kernels.py::test_gemm_nt, tests/test_gpu_x6.py) on that test's operands;
  * the fused epilogues (GELU, LayerScale-residual, SwiGLU, patch, the plane-image ones), which only the ViT forward reaches:
    a 2-block ViT-S/14 and ViT-g/14 on two 224 x 224 images (257 token rows each) against the CPU oracle, in every data flow
    that reaches other epilogue instantiations (fused and x6_fuse / h3_fuse = 0, both SwiGLU weight layouts of h3): the
    table in front of the forward tests says which epilogues each flow runs under the option.

Shapes: (257, 257) = 2 x 2 tiles of 256 (3 x 3 of 128) with one live row and column in the last; (1, 33) = one row, the
narrowest N the wide fp32 kernels serve; (300, 200); (1153, 257) = 10 tile rows of 128, more than one scheduling group of 8
and a tile count that is no multiple of 8.  K: one partial slab, tail slabs at BK 32 and 16, 2 / 3 / 5 slabs for the two-ahead
prefetch (fp32); 1, 3, 4 and 7 k-blocks against rings 2, 3 and 4 deep (h3).  gemm_f32_cfg 5 ... 8 are timing-only ablations
whose results are wrong by construction (csrc/gemm_f32.hip: launch_wide) and are not run.

Every configuration prints one line, ``TILECFG <family> cfg <n>: <shape> err <e> ...``, with its worst error and the shape that
gave it (and, for information, at how many of its cases the bits equal those of configuration 0).
"""
import itertools

import pytest
import torch

import _plan_edges as PE
import test_gpu_guard_bands as GB
import test_h3_plan_cpu as HP
from _guard_arena import Arena
from _stream_harness import same_bits
from anyloc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOKEN_ATOL = 2e-5            # tests/test_gpu_vit.py: unit-norm token rows against the oracle
MODE_RTOL = 2e-6             # tests/test_gpu_x6.py: un-normalised tokens of two kernel variants, relative to their scale

F32_CFGS = (1, 2, 3, 4, 10, 11, 20)
X6_CFGS = tuple(range(1, 10))
H3_CFGS = tuple(range(1, 6))
MN = ((257, 257), (1, 33), (300, 200), (1153, 257))
K_OF = {"f32": (4, 36, 64, 96, 160), "x6": (3, 16, 48, 100), "h3": (16, 48, 64, 112)}
OPTION_OF = {"f32": "gemm_f32_cfg", "x6": "x6_cfg", "h3": "h3_cfg"}
P, S = GB.P, GB.S


@pytest.fixture(scope="module")
def lib():
    from anyloc_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------ operands, references and the default kernels' results ----
_CASES = {}


def _case(family, M, N, K):
    """Operands, float64 reference and magnitude (with and without bias), e32 and the result of configuration 0 for one
    shape: computed once under the default options (every test starts from them) and left unchanged."""
    key = (family, M, N, K)
    if key in _CASES:
        return _CASES[key]
    from anyloc_amd import ops
    c = {}
    if family == "f32":                                                    # generator of tests/test_gpu_kernels.py::test_gemm_nt
        g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
        a, w, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
        a, w, bias = a.to(DEV), w.to(DEV), bias.to(DEV)
    elif family == "x6":
        a, w, bias = GB._x6_operands(M, N, K)
    else:
        a, w, bias = GB._h3_operands(M, N, K)
    c["a"], c["w"], c["bias"] = a, w, bias
    prod, mag = a.double() @ w.double().t(), a.double().abs() @ w.double().abs().t()
    c["ref"] = {True: prod + bias.double(), False: prod}
    c["mag"] = {True: mag + bias.double().abs(), False: mag}
    c["prod_mag"] = mag
    if family == "x6":
        c["a3"], c["w3"] = ops.split_x3(a), ops.split_x3(w)
    if family == "h3":
        c["a2"], c["w2"] = ops.split_h2(a), ops.split_h2(w)
    c["base"], c["e32"] = {}, {}
    for with_bias in (True, False):
        b = bias if with_bias else None
        if family == "x6":
            c["base"][with_bias] = ops.gemm_nt_x6(c["a3"], c["w3"], M, N, K, b)
        if family == "h3":
            c["base"][with_bias] = ops.gemm_nt_h3(c["a2"], c["w2"], M, N, K, b)
        if K % 4 == 0:                                                     # (anyloc_gemm_nt needs K % 4 == 0)
            c32 = ops.gemm_nt(a, w, b)
            c["e32"][with_bias] = float(((c32.double() - c["ref"][with_bias]).abs() / c["mag"][with_bias]).max())
            if family == "f32":
                c["base"][with_bias] = c32
    _CASES[key] = c
    return c


def _launch(lib, family, c, ar, out, ldc, M, N, K, with_bias):
    """one guarded call of the family's entry point: operands as inputs of the arena ``ar``, result into its view ``out``"""
    bin_ = ar.input("bias", c["bias"]) if with_bias else None
    if family == "f32":
        ain, win = ar.input("A", c["a"]), ar.input("W", c["w"])
        return lib.anyloc_gemm_nt(P(ain), K, P(win), K, P(bin_), P(out), ldc, M, N, K, S())
    if family == "x6":
        ain, win = ar.input("a3", c["a3"]), ar.input("w3", c["w3"])
        return lib.anyloc_gemm_nt_x6(P(ain), P(win), P(bin_), P(out), ldc, M, N, K, S())
    ain, ainv = ar.input("a2", c["a2"][0]), ar.input("a_inv", c["a2"][1])
    win, winv = ar.input("w2", c["w2"][0]), ar.input("w_inv", c["w2"][1])
    return lib.anyloc_gemm_nt_h3(P(ain), P(ainv), P(win), P(winv), P(bin_), P(out), ldc, M, N, K, S())


def _guarded(lib, family, M, N, K, ldc, with_bias, what):
    """-> (relative error against float64, the result) of one guarded call that met every assertion of its family"""
    c = _case(family, M, N, K)
    guard = GB._guard_for(ldc)
    ar = Arena(DEV, (8 << 20) + 8 * guard, guard=guard)
    out = ar.output("C", torch.float32, (M, N), (ldc, 1))
    st = _launch(lib, family, c, ar, out, ldc, M, N, K, with_bias)
    torch.cuda.synchronize()
    assert st == 0, (what, st, lib.anyloc_last_error())
    findings = ar.check({"C": None})
    assert findings == [], (what, findings)
    got = out.contiguous()
    ref, mag = c["ref"][with_bias], c["mag"][with_bias]
    diff = (got.double() - ref).abs()
    err = float((diff / mag).max())
    print(f"  {what}: err {err:.3e}" + (f" e32 {c['e32'][with_bias]:.3e}" if with_bias in c["e32"] else ""))
    if family == "f32":                                                    # tests/test_gpu_kernels.py::test_gemm_nt
        bound = 1.5e-6 * c["prod_mag"] + 1e-6
        assert bool((diff <= bound).all()), (what, float((diff / bound).max()))
    elif family == "x6":                                                   # tests/test_gpu_x6.py::test_gemm_x6_as_accurate_as_fp32
        assert err < 6e-7, (what, err)
        if K % 4 == 0:
            assert err < 1.5 * c["e32"][with_bias] + 1e-7, (what, err, c["e32"][with_bias])
    else:                                                                  # tests/test_gpu_x6.py::test_gemm_h3_as_accurate_as_fp32
        assert err < 1.5 * c["e32"][with_bias] + 1e-7, (what, err, c["e32"][with_bias])
        again = torch.full((M, ldc), float("nan"), device=DEV)[:, :N]
        st = lib.anyloc_gemm_nt_h3(P(c["a2"][0]), P(c["a2"][1]), P(c["w2"][0]), P(c["w2"][1]), P(c["bias"] if with_bias else None),
                                   P(again), ldc, M, N, K, S())
        assert st == 0 and same_bits(again.contiguous(), got), (what, "a repeated call gives other bits")
    return err, got


def _sweep(lib, family, label, before_launch=None):
    """every (M, N) x K x bias x ldc of the family under the options in force -> the TILECFG line's figures"""
    worst, worst_at, same, calls = -1.0, None, 0, 0
    for (M, N), K in itertools.product(MN, K_OF[family]):
        if before_launch:
            before_launch(M, N, K)
        for with_bias, ldc in itertools.product((True, False), (N, N + 4)):
            err, got = _guarded(lib, family, M, N, K, ldc, with_bias, (label, M, N, K, ldc, with_bias))
            calls, same = calls + 1, same + int(same_bits(got, _case(family, M, N, K)["base"][with_bias]))
            if err > worst:
                worst, worst_at = err, (M, N, K)
    return worst, worst_at, same, calls


def _references(family, shapes):
    """operands, references and configuration 0's results of ``shapes``, made while the options are still the defaults
    (every test starts from them)"""
    from anyloc_amd import ops
    assert all(ops.get_option(n) == 0 for n in OPTION_OF.values()) and ops.get_option("h3_group_m") == 8
    for M, N, K in shapes:
        _case(family, M, N, K)


def _shapes(family):
    return [(M, N, K) for (M, N), K in itertools.product(MN, K_OF[family])]


# ------------------------------------------------------------------------------------------------------ 1. direct GEMMs ----

@pytest.mark.parametrize("cfg", F32_CFGS)
def test_gemm_nt_every_configuration(lib, cfg):
    """anyloc_gemm_nt under gemm_f32_cfg = 1 ... 4 (256 x 128 with 4 and 8 waves, 128 x 128 at BK 16, 256 x 256), 10 / 11 (loads
    two slabs ahead on the default and on the 256 x 256 tile) and 20 (LDS-DMA staging where K % 32 == 0, the default kernel
    otherwise: K = 4 and 36 take that branch): bound of test_gemm_nt, clean guard bands."""
    from anyloc_amd import ops
    _references("f32", _shapes("f32"))
    ops.set_option("gemm_f32_cfg", cfg)
    assert ops.get_option("gemm_f32_cfg") == cfg
    worst, at, same, calls = _sweep(lib, "f32", f"gemm_nt cfg {cfg}")
    print(f"TILECFG f32 cfg {cfg}: {at} err {worst:.3e} (|out - ref| / |a||w|^T; bound 1.5e-6 + 1e-6 absolute); "
          f"{calls} guarded calls clean, bits of cfg 0 at {same}")


@pytest.mark.parametrize("cfg", X6_CFGS)
def test_gemm_nt_x6_every_configuration(lib, cfg):
    """anyloc_gemm_nt_x6 under x6_cfg = 1 ... 9: 128 x 128, 256 x 128 and 256 x 256 (8 waves, both wave layouts) tiles, 2- and
    3-deep rings (K = 3 and 16 are ONE k-block: fewer than the ring is deep), the three refill schedules; measure and bounds of
    test_gemm_x6_as_accurate_as_fp32, clean guard bands."""
    from anyloc_amd import ops
    _references("x6", _shapes("x6"))
    ops.set_option("x6_cfg", cfg)
    assert ops.get_option("x6_cfg") == cfg
    worst, at, same, calls = _sweep(lib, "x6", f"gemm_nt_x6 cfg {cfg}")
    print(f"TILECFG x6 cfg {cfg}: {at} err {worst:.3e} (bounds 6e-7 and 1.5 e32 + 1e-7); {calls} guarded calls clean, "
          f"bits of cfg 0 at {same}")


def _assert_h3_tile(lib, cfg, M, N, K):
    """the plan of anyloc_gemm_nt_h3 at this shape under the options in force: the batched route on kH3Tile[cfg]"""
    d = PE.describe(lib, M, N, K, "store", 0, 0)
    t = HP.H3_TILES[cfg]
    assert (d["mfma16"], d["route"], d["tile"]) == (0, HP.ROUTE_BATCHED, cfg), (cfg, M, N, K, d)
    assert (d["tile_rows"], d["tile_cols"], d["stages"]) == (HP._bm(t), HP._bn(t), t[4]), (cfg, M, N, K, d)


@pytest.mark.parametrize("cfg", H3_CFGS)
def test_gemm_nt_h3_every_configuration(lib, cfg):
    """anyloc_gemm_nt_h3 under h3_cfg = 1 ... 5 (kH3Tile[1 ... 5]: 128 x 256 on a 2-deep ring, 256 x 256 with 8 or 4 waves on 3- and
    4-deep rings; K = 16 ... 112 are 1, 3, 4 and 7 k-blocks).  Before each launch the library's own plan for the shape must name
    that tile (h3_cfg != 0 bypasses the small-M table, so also at one row); bound of test_gemm_h3_as_accurate_as_fp32, the same
    bits when repeated, clean guard bands."""
    from anyloc_amd import ops
    _references("h3", _shapes("h3"))
    ops.set_option("h3_cfg", cfg)
    assert ops.get_option("h3_cfg") == cfg
    worst, at, same, calls = _sweep(lib, "h3", f"gemm_nt_h3 cfg {cfg}", lambda M, N, K: _assert_h3_tile(lib, cfg, M, N, K))
    print(f"TILECFG h3 cfg {cfg}: {at} err {worst:.3e} (bound 1.5 e32 + 1e-7); {calls} guarded calls clean and reproducible, "
          f"bits of cfg 0 at {same}")


GROUP_M_SHAPES = ((1153, 257, 64), (1153, 700, 48))


@pytest.mark.parametrize("cfg,group_m", [(0, 1), (0, 3), (0, 100), (2, 3)], ids=lambda v: str(v))
def test_gemm_nt_h3_group_m_changes_no_bit(lib, cfg, group_m):
    """Option h3_group_m is the tile rows per XCD scheduling group of the workgroup -> tile map (csrc/tile_order.hpp:
    xcd_grouped_tile), read by the small-M plans' kernels (h3_cfg = 0 sends both shapes there) and by the kH3Tile ones
    (h3_cfg = 2: 5 tile rows of 256) alike.  The plan of each shape is asked of the library and printed: 1 and 3 must cut
    its tile rows into several groups with a shorter last one for 3, 100 is more than there are tile rows.  Every value
    visits every tile once like the default 8 -- the float64 criterion, clean guard bands, and the bits of h3_group_m = 8
    under the same plan, since the order of the tiles changes no arithmetic."""
    from anyloc_amd import ops
    _references("h3", GROUP_M_SHAPES)
    ops.set_option("h3_mfma16", 0)
    ops.set_option("h3_cfg", cfg)
    want = {}
    for (M, N, K), with_bias in itertools.product(GROUP_M_SHAPES, (True, False)):
        c = _case("h3", M, N, K)
        assert ops.get_option("h3_group_m") == 8
        want[(M, N, K, with_bias)] = ops.gemm_nt_h3(c["a2"], c["w2"], M, N, K, c["bias"] if with_bias else None)
    ops.set_option("h3_group_m", group_m)
    assert ops.get_option("h3_group_m") == group_m and ops.get_option("h3_cfg") == cfg
    worst, at, calls = -1.0, None, 0
    for (M, N, K) in GROUP_M_SHAPES:
        if cfg:
            _assert_h3_tile(lib, cfg, M, N, K)
        d = PE.describe(lib, M, N, K, "store", 0, 0)
        print(f"  group_m {group_m} at {(M, N, K)}: route {d['route']} tile {d['tile']} = {d['tile_rows']} x {d['tile_cols']}, "
              f"{d['tiles_m']} x {d['tiles_n']} tiles, split-K {d['ksplit']}")
        assert d["mfma16"] == 0 and d["route"] == (HP.ROUTE_BATCHED if cfg else HP.ROUTE_SMALL), d
        assert d["tiles_m"] == -(-M // d["tile_rows"]) and d["tiles_n"] == -(-N // d["tile_cols"]) and d["tiles_n"] > 1, d
        if group_m < 100:                                                  # several groups; 3: the last one is shorter
            assert d["tiles_m"] > group_m and (group_m == 1 or d["tiles_m"] % group_m != 0), (group_m, d)
        else:
            assert d["tiles_m"] < group_m, (group_m, d)
        for with_bias, ldc in itertools.product((True, False), (N, N + 4)):
            what = (f"gemm_nt_h3 cfg {cfg} group_m {group_m}", M, N, K, ldc, with_bias)
            err, got = _guarded(lib, "h3", M, N, K, ldc, with_bias, what)
            assert same_bits(got, want[(M, N, K, with_bias)]), (what, "differs from h3_group_m = 8")
            calls += 1
            if err > worst:
                worst, at = err, (M, N, K)
    print(f"TILECFG h3 cfg {cfg} group_m {group_m}: {at} err {worst:.3e} (bound 1.5 e32 + 1e-7); {calls} shapes x bias x ldc "
          f"clean, bits of group_m 8 at all")


# ------------------------------------------------------------------------------------- 2. the epilogues, through the forward ----
# Which epilogue instantiations a forward reaches under the option of its family (csrc/vit.hip):
#   f32               patch, store, LayerScale-residual, GELU (ViT-S) / SwiGLU (ViT-g) of csrc/gemm_f32.hip;
#   x6 "fused"        store and LayerScale-residual -- the FFN input GEMM writes fc2's plane image from ONE fixed kernel that
#                     does not read x6_cfg (csrc/gemm_x6.hip: dispatch_x6, p.C3);
#   x6 "unfused"      (x6_fuse = 0) also the fp32 GELU / SwiGLU epilogues of every tile;
#   h3 "fused"        patch, store, q|k|v planes, LayerScale-residual, GELU_H2 (ViT-S) / SWIGLU_T_H2 (ViT-g);
#   h3 "unfused"      (h3_fuse = 0) store, LayerScale-residual, fp32 GELU / SWIGLU_T;
#   h3 "interleaved"  ViT-g built under h3_swiglu_t = 0 (the 32 / 32 gate / value interleave): SWIGLU_H2, and with
#                     h3_fuse = 0 the fp32 SWIGLU.
# A variant = (options at model build, options at the forward); each is compared with ITS OWN forward at configuration 0.

MODELS = ("dinov2_vits14", "dinov2_vitg14")
HW = (224, 224)              # 257 token rows per image: one live row in the last tile of 128 and of 256
LAYER = 1
CFGS_OF = {"f32": F32_CFGS, "x6": X6_CFGS, "h3": H3_CFGS}
VARIANTS = {
    "f32": {"fused": ({}, {})},
    "x6": {"fused": ({}, {"x6_min_rows": 0}), "unfused": ({}, {"x6_min_rows": 0, "x6_fuse": 0})},
    "h3": {"fused": ({}, {}), "unfused": ({}, {"h3_fuse": 0}),
           "interleaved": ({"h3_swiglu_t": 0}, {}), "interleaved-unfused": ({"h3_swiglu_t": 0}, {"h3_fuse": 0})},
}
# the epilogue of the FFN input GEMM per (SwiGLU model, fc1_layout, fused): what csrc/vit.hip asks of gemm_h3
H3_FC1_EPILOGUE = {(False, 0, True): "gelu_h2", (False, 0, False): "gelu", (True, 1, True): "swiglu_t_h2", (True, 1, False): "swiglu_t",
                   (True, 0, True): "swiglu_h2", (True, 0, False): "swiglu"}
_FWD = {}


def _forward_cases():
    for name in MODELS:
        for family in ("f32", "x6", "h3"):
            for variant in VARIANTS[family]:
                if variant.startswith("interleaved") and name != "dinov2_vitg14":
                    continue                                               # (h3_swiglu_t is read for SwiGLU models only)
                for cfg in CFGS_OF[family]:
                    yield pytest.param(name, family, variant, cfg, id=f"{name}-{family}-{variant}-{cfg}")


def _images():
    if "imgs" not in _FWD:
        _FWD["imgs"] = torch.cat(synth.synthetic_places(1, 1, HW[0], HW[1], seed=5)[:2])
    return _FWD["imgs"]


def _state_dict(name):
    if ("sd", name) not in _FWD:
        _FWD[("sd", name)] = synth.synthetic_state_dict(name, 0, depth=2)
    return _FWD[("sd", name)]


def _oracle(name):
    """-> (unit-norm block-1 tokens with CLS, unit-norm layer-1 values) of the CPU oracle, once per model"""
    if ("oracle", name) not in _FWD:
        from oracle import dinov2_ref
        sd = _state_dict(name)
        with torch.device("meta"):                                        # (no random init of ViT-g's 40 blocks: 9 s)
            full = dinov2_ref.DinoVisionTransformer(name)
        full.blocks = full.blocks[:2]
        full.load_state_dict(sd, strict=True, assign=True)
        full.eval()
        _FWD[("oracle", name)] = (dinov2_ref.extract_facet(full, _images(), LAYER, "token", use_cls=True).to(DEV),
                                  dinov2_ref.extract_facet(full, _images(), LAYER, "value").to(DEV))
    return _FWD[("oracle", name)]


def _model(name, mode, build_options):
    """one HipDinoV2 per (model, GEMM mode, options read at build), without the FFN re-run that would hide which kernels
    produced the tokens"""
    key = ("model", name, mode, tuple(sorted(build_options.items())))
    if key not in _FWD:
        from anyloc_amd import extractor, ops
        with ops.options(**build_options):
            m = extractor.HipDinoV2(name, _state_dict(name), torch.device(DEV), gemm=mode)
        m.ffn_check = False
        assert m.gemm == mode
        if mode == "h3":                                                   # the option was read: the handle got that layout
            assert m.fc1_layout == (1 if m.ffn_kind == 1 and build_options.get("h3_swiglu_t", 1) else 0), (name, build_options)
        _FWD[key] = m
    return _FWD[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_the_models():
    yield
    _FWD.clear()
    _CASES.clear()


def _forward(model):
    """-> (un-normalised block-1 tokens with CLS, unit-norm layer-1 values) under the options in force"""
    imgs = _images().to(DEV)
    tok = model.forward_taps(imgs, [(LAYER, "token")], use_cls=True, norm_taps=False).clone()
    val = model.forward_taps(imgs, [(LAYER, "value")]).clone()
    return tok, val


def _check_forward(name, got, base, what):
    """finite; unit-norm rows within TOKEN_ATOL of the oracle; un-normalised tokens within 2e-6 x their scale of the same
    model's forward at configuration 0 -> (error against the oracle, error against configuration 0 over the scale)"""
    want_tok, want_val = _oracle(name)
    tok, val = got
    assert tuple(tok.shape) == tuple(want_tok.shape) and tuple(val.shape) == tuple(want_val.shape), what
    assert bool(torch.isfinite(tok).all()) and bool(torch.isfinite(val).all()), what
    unit = torch.nn.functional.normalize(tok.double(), dim=-1)
    e_tok, e_val = float((unit - want_tok.double()).abs().max()), float((val - want_val).abs().max())
    scale = float(base[0].abs().max())
    e_base = float((tok - base[0]).abs().max()) / scale
    print(f"  {what}: oracle err token {e_tok:.3e} value {e_val:.3e}; against cfg 0 {e_base:.3e} of scale {scale:.3e}")
    assert e_tok < TOKEN_ATOL and e_val < TOKEN_ATOL, (what, e_tok, e_val)
    assert e_base < MODE_RTOL, (what, e_base)
    return max(e_tok, e_val), e_base


def _base_forward(name, family, variant, model):
    """the variant's forward at configuration 0 (itself held to the oracle), once; the variant's options are in force"""
    from anyloc_amd import ops
    key = ("base", name, family, variant)
    if key not in _FWD:
        assert ops.get_option(OPTION_OF[family]) == 0
        base = _forward(model)
        _check_forward(name, base, base, (name, family, variant, 0))
        _FWD[key] = base
    return _FWD[key]


def _assert_h3_forward_plans(lib, name, model, fused, cfg):
    """the library's plan of every GEMM of the forward under the options in force: the batched route on kH3Tile[cfg]"""
    dim, _, _, ffn, hidden = synth.ARCH[name]
    swiglu = ffn == "swiglu"
    fc1 = H3_FC1_EPILOGUE[(swiglu, model.fc1_layout, fused)]
    gemms = {"qkv": (3 * dim, dim, "qkv_planes" if fused else "store"), "proj": (dim, dim, "ls_resid"),
             "fc1": (2 * hidden if swiglu else hidden, dim, fc1), "fc2": (dim, hidden, "ls_resid"), "facet": (dim, dim, "store")}
    for label, (N, K, epi) in gemms.items():
        d = PE.describe(lib, 2 * 257, N, K, epi, PE.KIND_OTHER, PE.WS)
        assert (d["route"], d["tile"], d["lead"]) == (HP.ROUTE_BATCHED, cfg, 0), (name, cfg, label, epi, d)
    return fc1


@pytest.mark.parametrize("name,family,variant,cfg", list(_forward_cases()))
def test_forward_epilogues_every_configuration(lib, name, family, variant, cfg):
    """One configuration of the mode's GEMM family through a 2-block forward on 2 x 257 token rows, in every data flow that
    reaches other epilogue instantiations (the table above): finite, within TOKEN_ATOL of the oracle, un-normalised tokens
    within 2e-6 x scale of the same flow at configuration 0."""
    from anyloc_amd import ops
    build_options, run_options = VARIANTS[family][variant]
    model = _model(name, family, build_options)
    for k, v in run_options.items():
        ops.set_option(k, v)
    base = _base_forward(name, family, variant, model)
    ops.set_option(OPTION_OF[family], cfg)
    assert ops.get_option(OPTION_OF[family]) == cfg and all(ops.get_option(k) == v for k, v in run_options.items())
    fc1 = ""
    if family == "h3":
        fc1 = " fc1 epilogue " + _assert_h3_forward_plans(lib, name, model, "unfused" not in variant, cfg)
    got = _forward(model)
    e_ref, e_base = _check_forward(name, got, base, (name, family, variant, cfg))
    same = torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    print(f"TILECFG fwd-{family} {variant} cfg {cfg}: {name} {HW}{fc1} err {e_ref:.3e} (oracle, bound {TOKEN_ATOL}); against cfg 0 "
          f"{e_base:.3e} (bound {MODE_RTOL}); bits of cfg 0: {same}")


def test_forward_data_flows_are_different_kernels(lib):
    """The variants above are only worth running if their options are read: the unfused flows and the interleaved SwiGLU
    layout must give other bits than the fused / transposed ones on the same weights (every one within TOKEN_ATOL of the
    oracle), and the two ViT-g h3 models were handed different fc1 layouts."""
    from anyloc_amd import ops
    name = "dinov2_vitg14"
    for family in ("x6", "h3"):
        tokens = {}
        for variant, (build_options, run_options) in VARIANTS[family].items():
            model = _model(name, family, build_options)
            with ops.options(**run_options):
                tokens[variant] = _base_forward(name, family, variant, model)[0]
        assert not torch.equal(tokens["fused"], tokens["unfused"]), (family, "x6_fuse / h3_fuse = 0 changed no bit")
        if family == "h3":
            assert _model(name, "h3", {}).fc1_layout == 1 and _model(name, "h3", {"h3_swiglu_t": 0}).fc1_layout == 0
            assert not torch.equal(tokens["interleaved"], tokens["interleaved-unfused"])
            print("TILECFG fwd-h3 layouts: transposed == interleaved bits:", torch.equal(tokens["fused"], tokens["interleaved"]))


@pytest.mark.parametrize("swiglu_t", [1, 0], ids=["transposed", "interleaved"])
def test_forward_exact_silu(lib, swiglu_t):
    """h3_fast_silu = 0: the exact SiLU (expf + IEEE division) in both fused SwiGLU epilogues of the two-term fp16 forward --
    SWIGLU_T_H2 on transposed accumulators (h3_swiglu_t = 1 when the model is built: fc1_layout 1) and the LDS-transposing
    SWIGLU_H2 (0).  Same two assertions as the tile configurations, and other bits than the fast SiLU: otherwise the option
    was not read."""
    from anyloc_amd import ops
    name = "dinov2_vitg14"
    variant = "fused" if swiglu_t else "interleaved"
    model = _model(name, "h3", VARIANTS["h3"][variant][0])
    assert model.fc1_layout == swiglu_t
    base = _base_forward(name, "h3", variant, model)
    with ops.options(h3_fast_silu=0):
        assert ops.get_option("h3_fast_silu") == 0
        got = _forward(model)
    e_ref, e_base = _check_forward(name, got, base, (name, "h3", "exact silu", variant))
    assert not torch.equal(got[0], base[0]), "h3_fast_silu = 0 gives the bits of the fast SiLU: the option was not read"
    print(f"TILECFG fwd-h3 fast_silu 0 swiglu_t {swiglu_t}: {name} {HW} err {e_ref:.3e} (oracle, bound {TOKEN_ATOL}); against the "
          f"fast SiLU {e_base:.3e} (bound {MODE_RTOL}); bits differ")
