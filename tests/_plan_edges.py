"""What tests/test_h3_plan_cpu.py (no GPU) and tests/test_gpu_plan_edges.py share: the block GEMMs of the four DINOv2 sizes as
the fused two-term fp16 forward launches them, the library's own answer for the plan of one launch
(``anyloc_h3_plan_describe``), the committed list of row counts at which a plan changes, and the image sizes that reach a
given row count.  Not a test module."""
import ctypes as C
import math

from anyloc_amd import _lib, synth

MODELS = ("dinov2_vits14", "dinov2_vitb14", "dinov2_vitl14", "dinov2_vitg14")
KIND_OTHER, KIND_QKV, KIND_PROJ, KIND_FC1, KIND_FC2 = range(5)           # csrc/common.hpp H3_KIND_*
WS, ACC, LN = _lib.H3_PLAN_SPLIT_WS, _lib.H3_PLAN_ACCUMULATE, _lib.H3_PLAN_LN_IN_FRONT
# what decides how a launch runs; tiles_m / tiles_n / grid follow from these and the shape
DECISION = ("mfma16", "route", "tile", "kb", "stages", "ksplit", "kper", "lead")

# Row counts M in 2 ... 1900 at which the plan of some block GEMM (qkv, proj, fc1 / w12, fc2) of the fused forward differs
# from that of M - 1, default options: derived from the library by tests/test_h3_plan_cpu.py, which fails until this literal
# follows a change of the plan table (csrc/gemm_h3s.hip: choose) -- the GPU tests run M - 1 and M for every entry.
EDGES = {
    "dinov2_vits14": (601, 1701, 1729),
    "dinov2_vitb14": (601, 1101, 1281, 1701, 1793),
    "dinov2_vitl14": (601, 1101, 1281, 1701),
    "dinov2_vitg14": (129, 193, 385, 601, 1101, 1701),
}
# one live row in the last 64-, 128- and 192-row tile at once (k * 384 + 1) next to the counts that fill every tile, and
# the ln_direct_rows boundary of the LayerNorm launches of the same forward
TILE_FILL = (384, 385, 768, 769, 1152, 1153, 1536, 1537)
ONE_LIVE_ROW = (385, 769, 1153, 1537)
LN_DIRECT = (1200, 1201)
# M - 1 = gh x gw with a near-square grid: these also run as ONE image through the uniform forward
ONE_IMAGE = {385: (16, 24), 577: (24, 24), 601: (24, 25), 769: (24, 32), 1101: (25, 44), 1153: (32, 36), 1537: (32, 48),
             1701: (34, 50)}


def block_gemms(name):
    """-> {label: (N, K, epilogue, kind, flags)}: the launches of one fused h3 block (csrc/vit.hip) and the facet GEMM of a
    forward that ends in a q / k / v tap."""
    dim, _, _, ffn, hidden = synth.ARCH[name]
    swiglu = ffn == "swiglu"
    return {
        "qkv": (3 * dim, dim, "qkv_planes", KIND_QKV, WS | LN),
        "proj": (dim, dim, "ls_resid", KIND_PROJ, WS),
        "fc1": (2 * hidden if swiglu else hidden, dim, "swiglu_t_h2" if swiglu else "gelu_h2", KIND_FC1, WS | LN),
        "fc2": (dim, hidden, "ls_resid", KIND_FC2, WS),
        "facet": (dim, dim, "store", KIND_PROJ, WS),
    }


BLOCK = ("qkv", "proj", "fc1", "fc2")


def describe(lib, M, N, K, epilogue, kind, flags):
    """The library's plan for one launch as a dict (anyloc_h3_plan_desc), under the options in force."""
    d = _lib.H3PlanDesc()
    st = lib.anyloc_h3_plan_describe(M, N, K, epilogue.encode(), kind, flags, C.byref(d))
    assert st == 0, (M, N, K, epilogue, kind, flags, lib.anyloc_last_error())
    return {f: int(getattr(d, f)) for f in _lib.H3_PLAN_FIELDS + ("grid",)}


# the forced small-M plans of tests/test_gpu_vit.py::test_small_m_plans_agree_with_the_plain_kernels: (h3s_cfg, h3s_kb, h3s_ksplit,
# h3s_stages) -- every tile of kSmallTile x five (k-blocks per stage, split-K factor, ring depth) triples
FORCED_PLANS = [(c, kb, ks, st) for c in range(8) for kb, ks, st in ((1, 1, 3), (2, 3, 6), (4, 2, 3), (1, 8, 6), (2, 5, 3))]


# the forced plans the plan function refuses, on every GEMM alike: the four widest tiles (128 x 128, 64 x 256 twice, 192 x 128) hold
# neither a 6-deep ring of two k-blocks per stage nor a 3-deep ring of four in the CU's 160 KiB of LDS, and fall back to the
# 3-deep ring / two k-blocks per stage -- what (2, 5, 3) forces anyway
REFUSED_PLANS = {(c, kb, ks, st) for c in (4, 5, 6, 7) for kb, ks, st in ((2, 3, 6), (4, 2, 3))}


H3_SPLIT_PART_BYTES, H3_SPLIT_TICKETS = 48 << 20, 4096       # csrc/common.hpp: the split-K workspace of one launch


def forced_ksplit(K, kb, ks, tiles, tile_elems):
    """the split-K factor h3_plan makes of a forced one (csrc/gemm_h3s.hip): no more splits than k-blocks or than the workspace
    holds partial tiles for, k-blocks per split a multiple of the forced k-blocks per stage, no empty split"""
    k16 = K // 16
    ks = min(ks, k16)
    while ks > 1 and (ks * tiles * tile_elems * 4 > H3_SPLIT_PART_BYTES or tiles > H3_SPLIT_TICKETS):
        ks -= 1
    if ks <= 1:
        return 1
    kper = -(-(-(-k16 // ks)) // kb) * kb
    return max(1, -(-k16 // kper))


def forced_plan_is_served(lib, rows, gemms, forced):
    """Under the options of ``forced`` = (cfg, kb, ksplit, stages), already in force: how would the library run each of ``gemms``
    ({label: (N, K, epilogue, kind, flags)}, each with the split-K workspace at hand) at ``rows`` rows?  Every GEMM on the small-M
    route, the forced tile and the split-K factor forced_ksplit restates; then either the forced k-blocks per stage and ring depth
    -> True (launch it), or, for every GEMM alike, fewer k-blocks / the 3-deep ring because the tile's ring would not fit the
    LDS -- the plan refuses the combination and names another entry of FORCED_PLANS -> False (asserted here, not to be
    launched again).  Which combinations are refused is pinned: exactly REFUSED_PLANS."""
    cfg, kb, ks, st = forced
    plans = {label: describe(lib, rows, *g) for label, g in gemms.items()}
    assert all(p["route"] == 0 and p["tile"] == cfg for p in plans.values()), (forced, plans)
    for label, (N, K, _, _, flags) in gemms.items():
        assert flags & WS and not flags & ACC, label
        p = plans[label]
        assert p["ksplit"] == forced_ksplit(K, kb, ks, p["tiles_m"] * p["tiles_n"], p["tile_rows"] * p["tile_cols"]), (forced, label, p)
    took = {(p["kb"], p["stages"]) for p in plans.values()}
    assert len(took) == 1, (forced, took)                  # what a tile's ring can hold does not depend on the GEMM
    served = took == {(kb, st)}
    assert served == (forced not in REFUSED_PLANS), (forced, took)
    if not served:
        (kb1, st1), = took
        assert kb1 <= kb and st1 <= st and (kb1, st1) in {(k, s) for c, k, _, s in FORCED_PLANS if c == cfg}, (forced, took)
    return served


def decision(plan):
    return tuple(plan[f] for f in DECISION)


def block_plans(lib, name, M):
    """-> {label: plan} of the four block GEMMs of ``name`` at M token rows"""
    g = block_gemms(name)
    return {k: describe(lib, M, *g[k]) for k in BLOCK}


def row_counts(name):
    """The row counts the GPU tests run for ``name``, ascending."""
    rows = set(TILE_FILL) | set(LN_DIRECT)
    for m in EDGES[name]:
        rows |= {m - 1, m}
    return tuple(sorted(rows))


def _shapes_by_area(max_side=73):
    """patch count -> its most nearly square grid (gh <= gw <= 73 patches: sides of at most 1022 px)"""
    best = {}
    for gh in range(1, max_side + 1):
        for gw in range(gh, max_side + 1):
            a = gh * gw
            if a not in best or gw - gh < best[a][1] - best[a][0]:
                best[a] = (gh, gw)
    return best


_AREAS = _shapes_by_area()


def _aspect(a):
    gh, gw = _AREAS[a]
    return gw / gh


def _two_parts(patches):
    """patches = a + b, both grids of at most 73 x 73: the split nearest to equal parts whose grids are no longer than twice
    their height, the least elongated one where there is none; None when no pair exists"""
    best = None
    for a in range(patches // 2, 0, -1):
        b = patches - a
        if a in _AREAS and b in _AREAS:
            worst = max(_aspect(a), _aspect(b))
            if worst <= 2.0:
                return [a, b]
            if best is None or worst < best[0]:
                best = (worst, [a, b])
    return best and best[1]


def image_sizes(M):
    """M token rows as two images (three where no pair exists): -> [(H, W), ...] in pixels with
    sum(1 + (H / 14) (W / 14)) == M and every side <= 1022.  Deterministic."""
    parts = _two_parts(M - 2)
    if parts is None:
        side = max(1, min(73, math.isqrt(max(1, (M - 3) // 3))))
        rest = _two_parts(M - 3 - side * side)
        if rest is None:
            raise ValueError(f"no two or three images of at most 1022 px a side have {M} token rows")
        parts = [side * side] + rest
    return [(14 * _AREAS[p][0], 14 * _AREAS[p][1]) for p in parts]


def rows_of(sizes):
    return sum(1 + (h // 14) * (w // 14) for h, w in sizes)

