"""The plan of every call of the fp32 MFMA GEMM (csrc/gemm_f32.hip: gemm_f32_plan), asked of the library itself through the
host-only ``anyloc_gemm_plan_describe`` -- no GPU needed.  A plan is one launch, or two that cut the rows into a part on 128-row
tiles and a rest on 64-row tiles; a plan whose parts miss or repeat a row computes a wrong product, one that names a kernel the
launcher does not compile is an error at launch.  Neither may be reachable from any shape, epilogue or ``gemm_f32_cfg``.  The
cost model that chooses the cut is restated here, literally, from the code it had before it moved into the plan function, and
the library's cut is held against it."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from anyloc_amd import _lib

ERR_INVALID_ARG = -1
EPILOGUES = ("store", "gelu", "ls_resid", "swiglu", "patch")
# the epilogues that have kernels with a K tail (K % 32 != 0); "gelu" / "ls_resid" / "swiglu" are refused there: the ViT forward,
# their only caller, contracts over dim or ffn_hidden, multiples of 64 (csrc/gemm_f32.hip: f32_epilogue_needs_k32)
K_TAIL_EPILOGUES = ("store", "patch")
SWEEP_M = np.concatenate([np.arange(1, 6001), np.arange(21000, 22001), np.arange(32000, 33001), np.arange(65000, 66001)])
SWEEP_N = (1, 32, 33, 128, 257, 384, 1152, 1536, 4608, 8192)
SWEEP_K = (4, 32, 36, 64, 8192, 8196)
OPTION_SETS = [{}] + [{"gemm_f32_cfg": c} for c in (1, 2, 3, 4, 5, 10, 11, 20)]

# csrc/gemm_f32.hip, kF32Tile: id -> (rows, cols, BK)
TILES = ((128, 128, 32), (256, 128, 32), (256, 128, 32), (128, 128, 16), (256, 256, 16), (64, 128, 32), (128, 32, 32), (128, 64, 32))
HALF, NARROW = 5, 6
# every (tile, KFULL, ROWSQ, ABL) gemm_nt has a kernel for -> the epilogues it is compiled with (f32_compiled)
COMPILED = {(NARROW, 0, 0, 0): ("store",), (NARROW, 0, 1, 0): ("store",),
            (0, 0, 1, 0): ("store",),                                   # row sums of squares
            (0, 1, 0, 32): ("store",),                                  # chunked summation
            (0, 1, 0, 1): ("store",), (0, 1, 0, 2): ("store",), (0, 1, 0, 3): ("store",), (0, 1, 0, 4): ("store",),
            (0, 1, 0, 64): EPILOGUES,
            (HALF, 1, 0, 0): ("store", "gelu", "ls_resid", "swiglu"),   # the 64-row part: no patch epilogue
            (4, 0, 0, 8): K_TAIL_EPILOGUES, (4, 1, 0, 8): EPILOGUES}
COMPILED.update({(t, kf, 0, 0): EPILOGUES if kf else K_TAIL_EPILOGUES for t in (0, 1, 2, 3, 4) for kf in (0, 1)})
COMPILED.update({(0, kf, 0, 8): EPILOGUES if kf else K_TAIL_EPILOGUES for kf in (0, 1)})
# option gemm_f32_cfg -> (tile, ABL) of a wide call (N > 32, no row sums); ABL of 5 and 20 where the kernel exists, else 0
CFG_TILE = {1: (1, 0), 2: (2, 0), 3: (3, 0), 4: (4, 0), 5: (0, 1), 10: (0, 8), 11: (4, 8), 20: (0, 64)}

PART = np.dtype([("row0", np.int64), ("rows", np.int64), ("grid", np.int64)] + [(f, np.int32) for f in _lib.GEMM_PLAN_PART_FIELDS])
DTYPE = np.dtype([("parts", np.int32), ("reserved", np.int32), ("part", PART, (2,))])

# (M, N) -> m1 (rows on 128-row tiles), evaluated from plan_row_split as it stood before the plan function
PINNED = {(768, 8192): 0, (769, 8192): 769, (1025, 8192): 1024, (1344, 4608): 0, (1345, 4608): 1345, (1793, 4608): 1792,
          (1028, 1536): 0, (5654, 1536): 5376, (5654, 8192): 5654, (21825, 384): 21760, (65537, 128): 65536}


def rounds_cost(tiles, unit):
    full, last = tiles // 512, tiles % 512
    return unit * (float(full) + (0.0 if last == 0 else (0.6 if last <= 256 else 1.0)))


def plan_row_split(M, N):
    """the cost model: rows [0, m1) on 128-row tiles, [m1, M) on 64-row tiles"""
    tn = (N + 127) // 128
    tm = (M + 127) // 128
    best, best_m1 = 1e30, M
    for k in range(tm, -1, -1):                      # ties -> the larger 128-row part
        m1 = k * 128 if k * 128 < M else M
        t128 = k * tn if k * 128 < M else tm * tn
        t64 = ((M - m1 + 63) // 64) * tn
        cost = rounds_cost(t128, 1.0) + rounds_cost(t64, 0.55) + (0.02 if t128 > 0 and t64 > 0 else 0.0)
        if cost < best - 1e-9:
            best, best_m1 = cost, m1
    return best_m1 if best < 0.96 * rounds_cost(tm * tn, 1.0) else M


def _rounds_cost_all(tiles, unit):
    full, last = tiles // 512, tiles % 512
    return unit * (full.astype(np.float64) + np.where(last == 0, 0.0, np.where(last <= 256, 0.6, 1.0)))


def plan_row_split_all(M, N):
    """plan_row_split for an array of row counts: the same loop over k, every M at once (the same double arithmetic)"""
    tn = (N + 127) // 128
    tm = (M + 127) // 128
    best, best_m1 = np.full(len(M), 1e30), M.copy()
    for k in range(int(tm.max()), -1, -1):
        live = k <= tm
        whole = k * 128 >= M
        m1 = np.where(whole, M, k * 128)
        t128 = np.where(whole, tm * tn, k * tn)
        t64 = ((M - m1 + 63) // 64) * tn
        cost = _rounds_cost_all(t128, 1.0) + _rounds_cost_all(t64, 0.55) + np.where((t128 > 0) & (t64 > 0), 0.02, 0.0)
        take = live & (cost < best - 1e-9)
        best, best_m1 = np.where(take, cost, best), np.where(take, m1, best_m1)
    return np.where(best < 0.96 * _rounds_cost_all(tm * tn, 1.0), best_m1, M)


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.fail("libanyloc_hip.so not built (python -m anyloc_amd.build)")
    assert C.sizeof(_lib.GemmPlanDesc) == DTYPE.itemsize and C.sizeof(_lib.GemmPlanPart) == PART.itemsize
    return _lib.load()


@pytest.fixture(scope="module")
def model_m1():
    """N -> the restated cost model's m1 at every M of the sweep"""
    return {N: plan_row_split_all(SWEEP_M, N) for N in SWEEP_N}


def describe(lib, M, N, K, epilogue, rowsq=0):
    d = _lib.GemmPlanDesc()
    st = lib.anyloc_gemm_plan_describe(M, N, K, epilogue.encode(), rowsq, C.byref(d))
    assert st == 0, (M, N, K, epilogue, rowsq, lib.anyloc_last_error())
    return np.frombuffer(bytes(d), dtype=DTYPE)[0]


_SWEEP = {}


def refused(lib, M, N, K, epilogue, rowsq=0):
    """the library refuses to plan this call, and says which epilogue needs what"""
    d = _lib.GemmPlanDesc()
    st = lib.anyloc_gemm_plan_describe(M, N, K, epilogue.encode(), rowsq, C.byref(d))
    return st == ERR_INVALID_ARG and b"needs K % 32 == 0" in lib.anyloc_last_error()


def sweep(lib, N, K, epilogue, rowsq):
    """the library's plans at every M of SWEEP_M -> structured array (one answer buffer and its references, reused)"""
    if not _SWEEP:
        out = (_lib.GemmPlanDesc * len(SWEEP_M))()
        size, first = C.sizeof(_lib.GemmPlanDesc), out[0]
        _SWEEP.update(out=out, rows=SWEEP_M.tolist(), refs=[C.byref(first, i * size) for i in range(len(SWEEP_M))])
    fn, epi = lib.anyloc_gemm_plan_describe, epilogue.encode()
    for m, ref in zip(_SWEEP["rows"], _SWEEP["refs"]):
        if fn(m, N, K, epi, rowsq, ref) != 0:
            raise AssertionError((m, N, K, epilogue, rowsq, lib.anyloc_last_error()))
    return np.frombuffer(_SWEEP["out"], dtype=DTYPE).copy()


def m1_of(p, M):
    """rows on 128-row tiles of an unablated default-tile plan: the first part of two, all or none of one"""
    return np.where(p["parts"] == 2, p["part"]["rows"][:, 0], np.where(p["part"]["tile"][:, 0] == HALF, 0, M))


def check(p, M, N, K, epilogue, rowsq, cfg, case):
    def ok(cond, what):
        if not np.all(cond):
            i = int(np.argmin(np.broadcast_to(cond, M.shape)))
            raise AssertionError((what, case, int(M[i]), p[i]))
    parts, a, b = p["parts"], p["part"][:, 0], p["part"][:, 1]
    two = parts == 2
    ok((parts == 1) | two, "one or two parts")
    # the parts tile [0, M) exactly once, in order
    ok((a["row0"] == 0) & (a["rows"] > 0), "the first part starts at row 0")
    ok(two | (a["rows"] == M), "one part: all rows")
    ok(~two | ((b["row0"] == a["rows"]) & (b["rows"] > 0) & (a["rows"] + b["rows"] == M)), "two parts: the second takes the rest")
    ok(~two | ((a["rows"] % 128 == 0) & (a["tile_rows"] == 128) & (b["tile_rows"] == 64)), "128-row tiles first, a 64-row rest")
    # two parts only where a launch can start at a row other than 0 and the default kernels run
    may_split = cfg == 0 and K % 32 == 0 and not rowsq and N > 32 and epilogue != "patch" and not (epilogue == "store" and K >= 8192)
    ok(~two | may_split, "a row split where there must be none")
    for q, live in ((a, parts >= 1), (b, two)):
        q = q[live]
        for t, kf, rs, abl in {tuple(int(v) for v in r) for r in np.unique(q[["tile", "kfull", "rowsq", "abl"]]).tolist()}:
            assert epilogue in COMPILED.get((t, kf, rs, abl), ()), ("a kernel gemm_nt does not compile", case, (t, kf, rs, abl))
        shape = np.array(TILES)[q["tile"]]
        assert np.all((q["tile_rows"] == shape[:, 0]) & (q["tile_cols"] == shape[:, 1]) & (q["bk"] == shape[:, 2])), ("tile shape", case)
        assert np.all((q["kfull"] == 0) | (K % q["bk"] == 0)), ("KFULL with a K tail", case)
        assert np.all((q["abl"] != 64) | (q["kfull"] == 1)), ("LDS-DMA staging with a K tail", case)
        assert np.all(q["rowsq"] == int(bool(rowsq) and epilogue == "store")), ("ROWSQ", case)
        grid = -(-q["rows"] // q["tile_rows"]) * -(-N // q["tile_cols"])
        assert np.all((q["grid"] == grid) & (grid < 2**31)), ("grid", case)
    # the routes of a plain-store call, then the option's tile
    if epilogue == "store" and N <= 32:
        ok(a["tile"] == NARROW, "N <= 32: the 32-column tile")
    elif epilogue == "store" and rowsq:
        ok((a["tile"] == 0) & (a["abl"] == 0), "row sums: the default tile")
    elif epilogue == "store" and K >= 8192 and K % 32 == 0 and cfg == 0:
        ok((a["tile"] == 0) & (a["abl"] == 32), "K >= 8192: chunked summation")
    elif cfg:
        tile, abl = CFG_TILE[cfg]
        if (cfg == 5 and not (epilogue == "store" and K % 32 == 0)) or (cfg == 20 and K % 32 != 0):
            abl = 0
        ok((a["tile"] == tile) & (a["abl"] == abl) & (a["kfull"] == int(K % 32 == 0)), "option gemm_f32_cfg names its kernel")
    else:
        ok((a["abl"] == 0) & (a["kfull"] == int(K % 32 == 0)) & ((a["tile"] == 0) | (a["tile"] == HALF)), "default kernels")
    return may_split


def _set(lib, options):
    assert lib.anyloc_reset_options() == 0
    for k, v in options.items():
        assert lib.anyloc_set_option(k.encode(), v) == 0, k


def test_restatement_of_the_cost_model():
    """The pinned cuts, and the all-at-once form of the loop against the literal one."""
    for (M, N), m1 in PINNED.items():
        assert plan_row_split(M, N) == m1, (M, N)
    some = np.concatenate([SWEEP_M[::97], np.array([m for m, _ in PINNED])])
    for N in SWEEP_N:
        assert plan_row_split_all(some, N).tolist() == [plan_row_split(int(m), N) for m in some], N


@pytest.mark.parametrize("options", OPTION_SETS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "defaults")
def test_every_plan_covers_its_rows_on_compiled_kernels(lib, model_m1, options):
    """Every M of the sweep x N x K x epilogue x (row sums asked or not): the parts tile the rows, every part names a compiled
    kernel, and wherever the call may be cut the cut is the restated cost model's."""
    cfg = options.get("gemm_f32_cfg", 0)
    try:
        _set(lib, options)
        for N, K, epi, rowsq in itertools.product(SWEEP_N, SWEEP_K, EPILOGUES, (0, 1)):
            case = (N, K, epi, rowsq, options)
            if K % 32 != 0 and epi not in K_TAIL_EPILOGUES:        # no kernel with a K tail: refused at every M, under every option
                assert all(refused(lib, int(m), N, K, epi, rowsq) for m in SWEEP_M[::61]), case
                continue
            p = sweep(lib, N, K, epi, rowsq)
            if check(p, SWEEP_M, N, K, epi, rowsq, cfg, case):
                got = m1_of(p, SWEEP_M)
                bad = np.nonzero(got != model_m1[N])[0]
                assert len(bad) == 0, (case, int(SWEEP_M[bad[0]]), int(got[bad[0]]), int(model_m1[N][bad[0]]))
    finally:
        lib.anyloc_reset_options()


def test_pinned_cuts(lib):
    assert lib.anyloc_reset_options() == 0
    for (M, N), m1 in PINNED.items():
        for epi in ("store", "gelu", "ls_resid", "swiglu"):
            p = describe(lib, M, N, 64, epi)
            assert int(m1_of(p[None], np.array([M]))[0]) == m1, (M, N, epi, p)
            assert p["parts"] == (2 if 0 < m1 < M else 1), (M, N, epi, p)
        assert describe(lib, M, N, 64, "patch")["parts"] == 1 and describe(lib, M, N, 36, "patch")["parts"] == 1
        assert refused(lib, M, N, 36, "gelu")


def test_describe_rejects_what_it_cannot_answer(lib):
    d = _lib.GemmPlanDesc()
    good = (1025, 8192, 32, b"store", 0)
    assert lib.anyloc_gemm_plan_describe(*good, C.byref(d)) == 0 and d.parts == 2
    for bad in ((0, 8192, 32, b"store", 0), (1025, -1, 32, b"store", 0), (1025, 8192, 0, b"store", 0), (-5, 8192, 32, b"store", 0),
                (1025, 8192, 30, b"store", 0), (1025, 8192, 32, b"stor", 0), (1025, 8192, 32, b"", 0), (1025, 8192, 32, b"qkv_planes", 0),
                (1025, 8192, 32, None, 0)):
        assert lib.anyloc_gemm_plan_describe(*bad, C.byref(d)) == ERR_INVALID_ARG, bad
        assert b"gemm_plan_describe" in lib.anyloc_last_error()
    assert lib.anyloc_gemm_plan_describe(*good, None) == ERR_INVALID_ARG
    assert b"gemm_plan_describe" in lib.anyloc_last_error()
    for name in EPILOGUES:
        assert lib.anyloc_gemm_plan_describe(1025, 8192, 32, name.encode(), 1, C.byref(d)) == 0, name
        assert refused(lib, 1025, 8192, 36, name) == (name not in K_TAIL_EPILOGUES), name
