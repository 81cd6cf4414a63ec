"""The plan of every launch of the two-term fp16 GEMM (csrc/gemm_h3s.hip: h3_plan), asked of the library itself through the
host-only ``anyloc_h3_plan_describe`` -- no GPU needed.  A plan that names a (tile, k-blocks per stage, ring depth) the launcher
does not compile is an error at launch; one whose split-K partial sums outgrow the workspace writes past it; neither may be
reachable from any row count, block GEMM shape, flag combination or option set.  The same file derives the row counts at
which a plan changes and holds them against the literal the GPU tests run (tests/_plan_edges.py), so that a change of the
table fails here until the GPU list follows."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import _plan_edges as pe
from anyloc_amd import _lib

ERR_INVALID_ARG = -1
# csrc/common.hpp
H3_SPLIT_PART_BYTES = 48 << 20
H3_SPLIT_TICKETS = 4096
ROUTE_SMALL, ROUTE_FIXED, ROUTE_BATCHED = 0, 1, 2
SMALL_EPILOGUES = ("store", "ls_resid", "qkv_planes", "gelu_h2", "swiglu_h2", "swiglu_t_h2")
# csrc/gemm_h3_kernel.hpp: (MI, NI, WM, WN) of kSmallTile, + ring depth of kH3Tile
SMALL_TILES = ((1, 2, 2, 1), (2, 2, 1, 2), (1, 2, 2, 2), (1, 4, 2, 1), (2, 2, 2, 2), (2, 2, 1, 4), (1, 4, 2, 2), (3, 2, 2, 2))
H3_TILES = ((2, 4, 2, 2, 3), (2, 4, 2, 2, 2), (2, 4, 4, 2, 3), (2, 4, 4, 2, 4), (4, 4, 2, 2, 4), (4, 4, 2, 2, 3), (1, 2, 2, 1, 3),
            (2, 2, 2, 2, 3))
LDS_BYTES = 160 * 1024
LN_LEAD_MAX_TILES = 200
FLAGS = tuple(range(8))                                  # every combination of workspace at hand / accumulating / LayerNorm in front
# the forced plans of tests/test_gpu_vit.py::test_small_m_plans_agree_with_the_plain_kernels
FORCED = [dict(h3s_cfg=c, h3s_kb=kb, h3s_ksplit=ks, h3s_stages=st)
          for c in range(8) for kb, ks, st in ((1, 1, 3), (2, 3, 6), (4, 2, 3), (1, 8, 6), (2, 5, 3))]
OPTION_SETS = [{}, {"h3s_enable": 0}, {"h3s_w12_tall": 0}, {"h3s_ln_lead": 1}]
ALL_M = np.arange(1, 3001)
# forced plans x every flag combination: the row counts around every 64-row tile edge and every threshold of the table
EDGE_M = np.array(sorted({m for m in range(1, 3001) if m % 64 in (0, 1, 63)} | {384, 385, 600, 601, 1100, 1101, 1700, 1701, 3000}))


def _bm(t):
    return 32 * t[0] * t[2]


def _bn(t):
    return 32 * t[1] * t[3]


def _lds(t, st, kb):
    return st * kb * 64 * (_bm(t) + _bn(t))


def _ndma(t, kb):
    return kb * 2 * (_bm(t) // 32 + _bn(t) // 32) // (t[2] * t[3])


def small_kb(t, kb):
    """four k-blocks per ring stage where a 3-deep ring of them fits the 160 KiB of LDS, two otherwise"""
    return (4 if _lds(t, 3, 4) <= LDS_BYTES else 2) if kb >= 4 else 2 if kb == 2 else 1


def small_stages(t, kb, stages):
    """a 6-deep ring where it fits the 160 KiB and the counted wait's 6 bits"""
    return 6 if stages >= 6 and _lds(t, 6, kb) <= LDS_BYTES and 4 * _ndma(t, kb) <= 63 else 3


def _tables():
    """compiled[route, tile, kb, stages], rows[route, tile], cols[route, tile], waves[tile] (small tiles)"""
    compiled = np.zeros((3, 8, 5, 7), dtype=bool)
    rows = np.zeros((3, 8), dtype=np.int64)
    cols = np.zeros((3, 8), dtype=np.int64)
    for i, t in enumerate(SMALL_TILES):
        rows[ROUTE_SMALL, i], cols[ROUTE_SMALL, i] = _bm(t), _bn(t)
        for kb in (1, 2, 4):
            for st in (3, 6):
                compiled[ROUTE_SMALL, i, kb, st] = small_kb(t, kb) == kb and small_stages(t, kb, st) == st
    for i, t in enumerate(H3_TILES):
        route = ROUTE_FIXED if i >= 6 else ROUTE_BATCHED
        rows[route, i], cols[route, i] = _bm(t), _bn(t)
        compiled[route, i, 1, t[4]] = True
    waves = np.array([t[2] * t[3] for t in SMALL_TILES])
    return compiled, rows, cols, waves


COMPILED, TILE_ROWS, TILE_COLS, SMALL_WAVES = _tables()
FIELDS = _lib.H3_PLAN_FIELDS + ("grid",)
DTYPE = np.dtype([(f, np.int32) for f in _lib.H3_PLAN_FIELDS] + [("grid", np.int64)])


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.fail("libanyloc_hip.so not built (python -m anyloc_amd.build)")
    assert C.sizeof(_lib.H3PlanDesc) == DTYPE.itemsize
    return _lib.load()


def shapes():
    """every distinct (N, K, epilogue, kind) among the block GEMMs and the facet GEMM of the four models"""
    return sorted({g[:4] for name in pe.MODELS for g in pe.block_gemms(name).values()})


def sweep(lib, N, K, epilogue, kind, flags, rows):
    """the library's plans for one GEMM at every row count of ``rows`` -> structured array"""
    out = (_lib.H3PlanDesc * len(rows))()
    fn, size, epi, first = lib.anyloc_h3_plan_describe, C.sizeof(_lib.H3PlanDesc), epilogue.encode(), out[0]
    for i, m in enumerate(rows.tolist()):
        if fn(m, N, K, epi, kind, flags, C.byref(first, i * size)) != 0:
            raise AssertionError((m, N, K, epilogue, kind, flags, lib.anyloc_last_error()))
    return np.frombuffer(out, dtype=DTYPE).copy()


def check(lib, p, M, N, K, epilogue, flags, case):
    """every assertion on the plans ``p`` of one GEMM at the row counts ``M``"""
    def ok(cond, what):
        if not np.all(cond):
            i = int(np.argmin(cond))
            raise AssertionError((what, case, int(M[i]), {f: int(p[f][i]) for f in FIELDS}))
    K16 = K // 16
    route, tile, kb, st, ks = p["route"], p["tile"], p["kb"], p["stages"], p["ksplit"]
    ok((route >= 0) & (route <= 2) & (tile >= 0) & (tile < 8) & (kb >= 1) & (kb <= 4) & (st >= 2) & (st <= 6), "field range")
    ok(COMPILED[route, tile, kb, st], "a (tile, k-blocks per stage, ring depth) the launcher does not compile")
    small = epilogue in SMALL_EPILOGUES
    ok((route != ROUTE_SMALL) | small, "small-M plan for an epilogue without one")
    ok((route != ROUTE_FIXED) | (not small), "fixed shapes for an epilogue that has small-M plans")
    ok((p["tile_rows"] == TILE_ROWS[route, tile]) & (p["tile_cols"] == TILE_COLS[route, tile]) & (p["tile_rows"] > 0), "tile shape")
    ok(p["tiles_m"] == -(-M // p["tile_rows"]), "tiles_m")
    ok(p["tiles_n"] == -(-N // p["tile_cols"]), "tiles_n")
    tiles = p["tiles_m"].astype(np.int64) * p["tiles_n"]
    lead = p["lead"]
    extra = p["grid"] - tiles * ks
    ok((lead == 1) | (extra == 0), "grid = tiles_m * tiles_n * ksplit")
    # split-K
    ok(ks >= 1, "ksplit")
    ok((ks > 1) | (p["kper"] == K16), "unsplit: kper = K16")
    ok((ks == 1) | (route == ROUTE_SMALL), "split-K outside the small-M plans")
    ok((ks == 1) | (p["kper"] % kb == 0), "kper is a multiple of the ring stage's k-blocks")
    ok((ks == 1) | (((ks - 1) * p["kper"] < K16) & (K16 <= ks * p["kper"])), "the splits cover the contraction, none empty")
    ok((ks == 1) | bool(flags & pe.WS and not flags & pe.ACC), "split-K without the workspace / on an accumulating launch")
    ok((ks == 1) | (ks * tiles * p["tile_rows"] * p["tile_cols"] * 4 <= H3_SPLIT_PART_BYTES), "split-K partial sums outgrow the workspace")
    ok((ks == 1) | (tiles <= H3_SPLIT_TICKETS), "more split-K tiles than tickets")
    # LayerNorm lead role
    ok((lead >= 0) & (lead <= 2), "lead")
    ok((lead == 0) | bool(flags & pe.LN), "lead role without a LayerNorm in front")
    ok((lead == 0) | (ks == 1), "lead role on a split plan")
    lead_compiled = (kb == 1) & (st == 6) & (((tile == 4) & (epilogue == "qkv_planes")) |
                                             ((tile == 7) & (epilogue in ("swiglu_t_h2", "swiglu_h2"))))
    ok((lead != 1) | ((route == ROUTE_SMALL) & lead_compiled), "small-M lead role on a plan it is not compiled for")
    ok((lead != 1) | (tiles <= LN_LEAD_MAX_TILES), "small-M lead role with more than 200 tiles")
    nw = SMALL_WAVES[tile]
    ok((lead != 1) | ((extra > 0) & (extra % 8 == 0) & (extra * nw >= M) & ((extra - 8) * nw < M)),
       "small-M lead workgroups: a multiple of 8 that covers one row per wave")
    ok((lead != 2) | ((route == ROUTE_BATCHED) & (tile == 0) & (K <= 1536) &
                      np.isin(epilogue, ("qkv_planes", "swiglu_t_h2", "swiglu_h2", "gelu_h2"))), "batched lead role")
    for i in np.nonzero(lead == 2)[0].tolist():
        g = C.c_uint32()
        assert lib.anyloc_h3_lead_plan_check(int(p["tiles_m"][i]), int(p["tiles_n"][i]), 8, int(M[i]), C.byref(g)) == 1
        assert g.value == p["grid"][i], (case, int(M[i]))


def _set(lib, options):
    assert lib.anyloc_reset_options() == 0
    for k, v in options.items():
        assert lib.anyloc_set_option(k.encode(), v) == 0, k


def test_describe_rejects_what_it_cannot_answer(lib):
    d = _lib.H3PlanDesc()
    good = (530, 1536, 1536, b"ls_resid", pe.KIND_PROJ, pe.WS)
    assert lib.anyloc_h3_plan_describe(*good, C.byref(d)) == 0
    for bad in ((0, 1536, 1536, b"ls_resid", 2, 1), (530, -1, 1536, b"ls_resid", 2, 1), (530, 1536, 0, b"ls_resid", 2, 1),
                (530, 1536, 1530, b"ls_resid", 2, 1), (530, 1536, 1536, b"resid", 2, 1), (530, 1536, 1536, b"", 2, 1),
                (530, 1536, 1536, None, 2, 1), (530, 1536, 1536, b"ls_resid", 5, 1), (530, 1536, 1536, b"ls_resid", -1, 1),
                (530, 1536, 1536, b"ls_resid", 2, 8)):
        assert lib.anyloc_h3_plan_describe(*bad, C.byref(d)) == ERR_INVALID_ARG, bad
        assert b"h3_plan_describe" in lib.anyloc_last_error()
    assert lib.anyloc_h3_plan_describe(*good, None) == ERR_INVALID_ARG
    # every epilogue name of the header is known
    for name in SMALL_EPILOGUES + ("gelu", "swiglu", "swiglu_t", "patch"):
        assert lib.anyloc_h3_plan_describe(530, 1536, 1536, name.encode(), 0, 0, C.byref(d)) == 0, name


@pytest.mark.parametrize("options", OPTION_SETS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "defaults")
def test_every_plan_of_the_block_gemms_can_be_launched(lib, options):
    """M = 1 ... 3000 x the block and facet GEMM shapes of the four models x every flag combination, under the default options
    and the three switches of the table."""
    try:
        _set(lib, options)
        for (N, K, epi, kind), flags in itertools.product(shapes(), FLAGS):
            check(lib, sweep(lib, N, K, epi, kind, flags, ALL_M), ALL_M, N, K, epi, flags, (N, K, epi, kind, flags, options))
    finally:
        lib.anyloc_reset_options()


def test_every_forced_plan_can_be_launched(lib):
    """The sweeps' overrides (h3s_cfg / h3s_kb / h3s_ksplit / h3s_stages) ask for combinations no kernel is compiled for (four
    k-blocks per stage on a 64 x 256 tile, a 6-deep ring of 192 x 128 tiles with two k-blocks) and for split factors the
    workspace cannot hold: the plan must come back clipped to what can run.  Every M with the flags of the GEMM in the fused
    forward; every flag combination at the row counts around each 64-row tile edge and each threshold of the table."""
    in_forward = {g[:4]: g[4] for name in pe.MODELS for g in pe.block_gemms(name).values()}
    try:
        for forced in FORCED:
            _set(lib, forced)
            for N, K, epi, kind in shapes():
                f = in_forward[(N, K, epi, kind)]
                check(lib, sweep(lib, N, K, epi, kind, f, ALL_M), ALL_M, N, K, epi, f, (N, K, epi, kind, f, forced))
                for flags in FLAGS:
                    check(lib, sweep(lib, N, K, epi, kind, flags, EDGE_M), EDGE_M, N, K, epi, flags, (N, K, epi, kind, flags, forced))
    finally:
        lib.anyloc_reset_options()


def test_the_other_epilogues_and_the_public_gemm_shapes(lib):
    """The epilogues without small-M plans (the unfused data flows: fixed 64 x 64 / 128 x 128 shapes while there are few tiles)
    and the plain-store GEMM of ``anyloc_gemm_nt_h3`` (no workspace, kind 0) at the widths of tests/test_gpu_plan_edges.py."""
    assert lib.anyloc_reset_options() == 0
    dim, hidden = 1536, 4096
    for N, K, epi in ((hidden, dim, "gelu"), (2 * hidden, dim, "swiglu"), (2 * hidden, dim, "swiglu_t"), (dim, 608, "patch"),
                      (3072, 768, "gelu"), (384, 592, "patch")):
        for flags in FLAGS:
            p = sweep(lib, N, K, epi, pe.KIND_OTHER, flags, ALL_M)
            check(lib, p, ALL_M, N, K, epi, flags, (N, K, epi, flags))
            assert np.all(p["route"] != ROUTE_SMALL) and np.all(p["ksplit"] == 1) and np.all(p["lead"] == 0)
    for N, K in ((2048, 256), (2049, 256), (8191, 64), (8192, 64), (768, 3072), (768, 3056)):
        p = sweep(lib, N, K, "store", pe.KIND_OTHER, 0, ALL_M)
        check(lib, p, ALL_M, N, K, "store", 0, (N, K, "store"))
        assert np.all(p["ksplit"] == 1)                                  # no workspace: the table's split-K 2 is dropped


H3_CFG_SHAPES = ((1, 33, 16), (5, 7, 48), (257, 257, 16), (300, 200, 48), (530, 1536, 1536), (1153, 257, 112), (1153, 700, 64),
                 (2051, 4608, 1536), (2999, 8192, 1536))


@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5])
def test_h3_cfg_names_its_tile_at_every_size(lib, cfg):
    """Option h3_cfg = 1 ... 5 (the sweeps' candidates, kH3Tile[1 ... 5]) bypasses the small-M table: whatever the shape -- a
    single row, a single k-block, the block GEMMs of ViT-g --, the epilogue, the kind and the flags, the plan is the batched
    route on exactly that tile with that tile's ring depth, unsplit, without a lead role, one workgroup per tile.  The GPU tests
    of tests/test_gpu_tile_configs.py rely on this to know which kernel they ran."""
    t = H3_TILES[cfg]
    rows, cols = _bm(t), _bn(t)
    assert (rows, cols, t[4]) == {1: (128, 256, 2), 2: (256, 256, 3), 3: (256, 256, 4), 4: (256, 256, 4), 5: (256, 256, 3)}[cfg]
    try:
        _set(lib, {"h3_cfg": cfg})
        for (M, N, K), epi, kind, flags in itertools.product(H3_CFG_SHAPES, SMALL_EPILOGUES + ("gelu", "swiglu", "swiglu_t", "patch"),
                                                             (pe.KIND_OTHER, pe.KIND_QKV, pe.KIND_FC2), FLAGS):
            p = pe.describe(lib, M, N, K, epi, kind, flags)
            case = (cfg, M, N, K, epi, kind, flags, p)
            assert p["route"] == ROUTE_BATCHED and p["tile"] == cfg, case
            assert (p["tile_rows"], p["tile_cols"], p["stages"]) == (rows, cols, t[4]), case
            assert p["kb"] == 1 and p["ksplit"] == 1 and p["kper"] == K // 16 and p["lead"] == 0, case
            assert p["tiles_m"] == -(-M // rows) and p["tiles_n"] == -(-N // cols), case
            assert p["grid"] == p["tiles_m"] * p["tiles_n"], case
            assert p["mfma16"] == 0, case                                   # (none of these shapes has 256 tiles of 256 x 256)
    finally:
        lib.anyloc_reset_options()


def test_documented_winners_of_the_table(lib):
    """The measured winners named in the comments of choose() (ViT-g, one / two 322 x 322 images and one 476 x 630 image)."""
    assert lib.anyloc_reset_options() == 0
    g = pe.block_gemms("dinov2_vitg14")

    def plan(label, M):
        return pe.describe(lib, M, *g[label])

    def shape(p):
        return p["route"], p["tile"], p["tile_rows"], p["tile_cols"], p["kb"], p["stages"], p["ksplit"]

    # fc2: 64 x 128 four-wave tiles, 6-deep ring; split-K 2 at one image, unsplit at two
    assert shape(plan("fc2", 530)) == (ROUTE_SMALL, 2, 64, 128, 1, 6, 2) and plan("fc2", 530)["kper"] == 128
    assert shape(plan("fc2", 1060)) == (ROUTE_SMALL, 2, 64, 128, 1, 6, 1)
    # proj: 64 x 64 / 6-deep at one image, 64 x 128 / 6-deep at two
    assert shape(plan("proj", 530)) == (ROUTE_SMALL, 0, 64, 64, 1, 6, 1)
    assert shape(plan("proj", 1060)) == (ROUTE_SMALL, 2, 64, 128, 1, 6, 1)
    # qkv: 128 x 128 / 6-deep at one image
    assert shape(plan("qkv", 530)) == (ROUTE_SMALL, 4, 128, 128, 1, 6, 1)
    # w12: 192 x 128 / 6-deep at 385 ... 600 rows, and not outside
    for M in range(385, 601):
        assert shape(plan("fc1", M)) == (ROUTE_SMALL, 7, 192, 128, 1, 6, 1), M
    assert plan("fc1", 384)["tile"] != 7 and plan("fc1", 601)["tile"] != 7
    # one 476 x 630 image: fc2 split-K 2, proj 64 x 128 / 6-deep
    assert shape(plan("fc2", 1531)) == (ROUTE_SMALL, 2, 64, 128, 1, 3, 2)
    assert shape(plan("proj", 1531)) == (ROUTE_SMALL, 2, 64, 128, 1, 6, 1)
    # default options: no lead role; with h3s_ln_lead the one-image qkv and w12 launches carry their LayerNorm
    assert all(plan(k, 530)["lead"] == 0 for k in pe.BLOCK)
    try:
        _set(lib, {"h3s_ln_lead": 1})
        assert plan("qkv", 530)["lead"] == 1 and plan("fc1", 530)["lead"] == 1
        assert plan("qkv", 1531)["lead"] == 0                            # 432 tiles: more than the lead role allows
        # w12 carries LN2 on its 192 x 128 plan while that has at most 200 tiles: 3 x 64 up to 576 rows, 4 x 64 from 577 on
        assert [M for M in range(1, 1901) if plan("fc1", M)["lead"]] == list(range(385, 577))
        for name in pe.MODELS[1:]:
            qkv = pe.block_gemms(name)["qkv"]
            assert [M for M in range(1, 1901) if pe.describe(lib, M, *qkv)["lead"]] == list(range(1, 601)), name
    finally:
        lib.anyloc_reset_options()


def derived_edges(lib, name):
    g = pe.block_gemms(name)
    rows = np.arange(1, 1901)
    changed = np.zeros(len(rows), dtype=bool)
    for label in pe.BLOCK:
        p = sweep(lib, *g[label], rows)
        for f in pe.DECISION:
            changed[1:] |= p[f][1:] != p[f][:-1]
    return tuple(int(m) for m in rows[changed])


def test_the_committed_edge_list_is_the_librarys(lib):
    """Every M in 2 ... 1900 at which some block GEMM's plan differs from that of M - 1, default options, per model: equal to
    the literal the GPU tests import.  Move a threshold of choose() and this fails until tests/_plan_edges.py follows."""
    assert lib.anyloc_reset_options() == 0
    derived = {name: derived_edges(lib, name) for name in pe.MODELS}
    assert derived == pe.EDGES, derived


def test_row_count_helper_reaches_every_listed_row_count():
    for name in pe.MODELS:
        for M in pe.row_counts(name):
            sizes = pe.image_sizes(M)
            assert len(sizes) in (2, 3) and pe.rows_of(sizes) == M, (M, sizes)
            assert all(14 <= s <= 1022 and s % 14 == 0 for hw in sizes for s in hw), (M, sizes)
    for M in range(4, 3001):
        assert pe.rows_of(pe.image_sizes(M)) == M
    for M, (gh, gw) in pe.ONE_IMAGE.items():
        assert 1 + gh * gw == M and gw <= 2 * gh and 14 * gw <= 1022
    assert all(m % 384 == 1 for m in pe.ONE_LIVE_ROW)
