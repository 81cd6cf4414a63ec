"""ANYLOC_TOPK_NO_WAIT without a GPU: the flag's value, which entry points accept it, what the size functions answer now that the
side batch of the overflowed queries lives in the workspace, and the stream lint over the sources (the flagged path may not
hold a blocking call; the waiting path keeps its one)."""
import ctypes as C
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from anyloc_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG = -1
NO_WAIT, RESCORE_PLANES, NORMALIZE_DB = 4, 2, 1


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.fail("libanyloc_hip.so not built (python -m anyloc_amd.build)")
    return _lib.load()


@pytest.fixture(autouse=True)
def _restore_options(lib):
    yield
    assert lib.anyloc_reset_options() == 0


def test_the_flag_is_four_in_the_header_and_in_python():
    header = open(os.path.join(ROOT, "include", "anyloc_hip.h")).read()
    m = re.search(r"^#define\s+ANYLOC_TOPK_NO_WAIT\s+(\d+)u\s*$", header, re.M)
    assert m and int(m.group(1)) == ops.TOPK_NO_WAIT == NO_WAIT
    assert re.search(r"^#define\s+ANYLOC_ABI_VERSION\s+10\s*$", header, re.M)              # additive: the ABI number stays


def _searches(lib, flags, f=None, i=None):
    """the three searches with (null or given) data pointers and ``flags`` -> {entry point: (status, message)}"""
    out = {}
    st = lib.anyloc_topk(f, 70, f, 300, 256, 5, 0, flags, 0, f, i, None, 0, None)
    out["anyloc_topk"] = (st, lib.anyloc_last_error().decode())
    st = lib.anyloc_topk_search_index(f, 70, f, 300, 256, 5, 0, flags, 0, f, i, None, 0, None)
    out["anyloc_topk_search_index"] = (st, lib.anyloc_last_error().decode())
    st = lib.anyloc_topk_search_index_rows(f, 70, f, f, 300, 256, 5, 0, flags, 0, f, i, None, 0, None)
    out["anyloc_topk_search_index_rows"] = (st, lib.anyloc_last_error().decode())
    return out


def test_all_three_searches_accept_the_flag(lib):
    """with null data pointers the complaint is about the pointers (the null checks come first); with real ones the call gets as
    far as the workspace check, under every combination with the other two flags an entry point takes"""
    for flags in (NO_WAIT, NO_WAIT | NORMALIZE_DB):
        for name, (st, msg) in _searches(lib, flags).items():
            assert st == ERR_INVALID_ARG and "flags" not in msg and "ANYLOC_TOPK" not in msg, (name, flags, msg)
            assert "null" in msg or "no index" in msg, (name, msg)
    fbuf, ibuf = (C.c_float * 64)(), (C.c_int64 * 64)()
    f, i = C.addressof(fbuf), C.addressof(ibuf)
    for flags in (NO_WAIT, NO_WAIT | NORMALIZE_DB, NO_WAIT | RESCORE_PLANES, NO_WAIT | RESCORE_PLANES | NORMALIZE_DB):
        for name, (st, msg) in _searches(lib, flags, f, i).items():
            if name == "anyloc_topk" and flags & RESCORE_PLANES:
                continue
            assert st == -2 and re.fullmatch(r"topk: workspace 0 < \d+", msg), (name, flags, st, msg)


def test_the_one_shot_search_still_refuses_rescore_planes(lib):
    fbuf, ibuf = (C.c_float * 64)(), (C.c_int64 * 64)()
    f, i = C.addressof(fbuf), C.addressof(ibuf)
    for flags in (RESCORE_PLANES, RESCORE_PLANES | NO_WAIT, RESCORE_PLANES | NO_WAIT | NORMALIZE_DB):
        st = lib.anyloc_topk(f, 70, f, 300, 256, 5, 0, flags, 0, f, i, None, 0, None)
        assert st == ERR_INVALID_ARG
        assert lib.anyloc_last_error().decode() == ("topk: ANYLOC_TOPK_RESCORE_PLANES needs a prepared index "
                                                    "(anyloc_topk_search_index / anyloc_topk_search_index_rows)")


def test_bit_eight_is_still_unknown(lib):
    fbuf, ibuf = (C.c_float * 64)(), (C.c_int64 * 64)()
    f, i = C.addressof(fbuf), C.addressof(ibuf)
    for flags in (8, 8 | NO_WAIT):
        for name, (st, msg) in _searches(lib, flags, f, i).items():
            assert st == ERR_INVALID_ARG and msg == f"topk: unknown flags {flags}", (name, flags, msg)


# What anyloc_topk_workspace_bytes / anyloc_topk_index_workspace_bytes answered on the PARENT commit of the change that added the
# flag, recorded from a build of that commit: per shape of tests/test_topk_workspace_cpu.py, for k in its KS = (1, 10, 128, 129,
# 1024), under the default options and with the fp16 panels and the screened search forced.  The size functions take no flags,
# so they now cover the side batch wherever a shape screens: never less than this, and the same where it does not screen.
PARENT_KS = (1, 10, 128, 129, 1024)
PARENT_SIZES = {
    "defaults": {
        (9, 103, 64): ((10240, 10240, 10240, 10240, 10240),
                           (12288, 12288, 12288, 12288, 12288)),
        (70, 32868, 64): ((9574912, 9574912, 9574912, 9574912, 9574912),
                              (2711552, 2711552, 2711552, 2711552, 2711552)),
        (5, 300, 4096): ((2572800, 2572800, 2572800, 2572800, 2572800),
                             (96512, 96512, 96512, 96512, 96512)),
        (5, 32868, 4096): ((138679808, 138679808, 138679808, 138679808, 138679808),
                               (645120, 645120, 645120, 645120, 645120)),
        (70, 300, 256): ((93184, 93184, 93184, 93184, 93184),
                             (164864, 164864, 164864, 164864, 164864)),
        (70, 8492, 64): ((2485248, 2485248, 2485248, 2485248, 2485248),
                             (2418944, 2418944, 2418944, 2418944, 2418944)),
        (70, 300, 8208): ((93184, 93184, 93184, 93184, 93184),
                              (2391552, 2391552, 2391552, 2391552, 2391552)),
        (5, 8492, 64): ((276992, 276992, 276992, 276992, 276992),
                            (271872, 271872, 271872, 271872, 271872)),
        (70, 8492, 256): ((2485248, 2485248, 2485248, 2485248, 2485248),
                              (2472704, 2472704, 2472704, 2472704, 2472704)),
        (70, 131372, 64): ((10756864, 10756864, 10756864, 10756864, 10756864),
                               (3893504, 3893504, 3893504, 3893504, 3893504)),
        (70, 300, 24592): ((93184, 93184, 93184, 93184, 93184),
                               (6979072, 6979072, 6979072, 6979072, 6979072)),
        (70, 1000, 256): ((297472, 297472, 297472, 297472, 297472),
                              (369152, 369152, 369152, 369152, 369152)),
        (300, 20000, 4096): ((180080640, 180112896, 180537600, 149242624, 149242624),
                                 (45718272, 45750528, 46175232, 14992640, 14992640)),
        (256, 2048, 1024): ((11572736, 11572736, 11572736, 11572736, 11572736),
                                (3176448, 3176448, 3176448, 3176448, 3176448)),
        (255, 2048, 1024): ((2119168, 2119168, 2119168, 2119168, 2119168),
                                (3164160, 3164160, 3164160, 3164160, 3164160)),
        (64, 300, 4096): ((2643456, 2643456, 2643456, 2643456, 2643456),
                              (1133824, 1133824, 1133824, 1133824, 1133824)),
        (65, 300, 4096): ((87040, 87040, 87040, 87040, 87040),
                              (1152000, 1152000, 1152000, 1152000, 1152000)),
        (9, 0, 64): ((5888, 5888, 5888, 5888, 5888),
                         (0, 0, 0, 0, 0)),
        (9, 5, 64): ((5888, 5888, 5888, 5888, 5888),
                         (7936, 7936, 7936, 7936, 7936)),
    },
    "topk_h3=1,topk_screen=1": {
        (9, 103, 64): ((10240, 10240, 10240, 10240, 10240),
                           (343296, 344064, 356608, 12288, 12288)),
        (70, 32868, 64): ((16761088, 16768256, 16867328, 4840960, 4840960),
                              (14467840, 14475008, 14574080, 2711552, 2711552)),
        (5, 300, 4096): ((2572800, 2572800, 2572800, 2572800, 2572800),
                             (280064, 280320, 287232, 96512, 96512)),
        (5, 32868, 4096): ((138679808, 138679808, 138679808, 138679808, 138679808),
                               (1484032, 1484288, 1491200, 645120, 645120)),
        (70, 300, 256): ((3056128, 3063296, 3162368, 472832, 472832),
                             (2746112, 2753280, 2852352, 164864, 164864)),
        (70, 8492, 64): ((9489664, 9496832, 9595904, 4548352, 4548352),
                             (7293952, 7301120, 7400192, 2418944, 2418944)),
        (70, 300, 8208): ((14825216, 14832384, 14931456, 12241920, 12241920),
                              (4972800, 4979968, 5079040, 2391552, 2391552)),
        (5, 8492, 64): ((276992, 276992, 276992, 276992, 276992),
                            (619264, 619520, 626432, 271872, 271872)),
        (70, 8492, 256): ((15834880, 15842048, 15941120, 10893568, 10893568),
                              (7347712, 7354880, 7453952, 2472704, 2472704)),
        (70, 131372, 64): ((43568384, 43575552, 43674624, 6022912, 6022912),
                               (40881152, 40888320, 40987392, 3893504, 3893504)),
        (70, 300, 24592): ((39073536, 39080704, 39179776, 36490240, 36490240),
                               (9560320, 9567488, 9666560, 6979072, 6979072)),
        (70, 1000, 256): ((3985664, 3992832, 4091904, 1396736, 1396736),
                              (2950400, 2957568, 3056640, 369152, 369152)),
        (300, 20000, 4096): ((180080640, 180112896, 180537600, 149242624, 149242624),
                                 (45718272, 45750528, 46175232, 14992640, 14992640)),
        (256, 2048, 1024): ((21029888, 21057536, 21420032, 11572736, 11572736),
                                (12617728, 12645376, 13007872, 3176448, 3176448)),
        (255, 2048, 1024): ((20980736, 21008384, 21369344, 11560448, 11560448),
                                (12568576, 12596224, 12957184, 3164160, 3164160)),
        (64, 300, 4096): ((2643456, 2643456, 2643456, 2643456, 2643456),
                              (3492608, 3499520, 3590144, 1133824, 1133824)),
        (65, 300, 4096): ((8466944, 8473856, 8565504, 6067968, 6067968),
                              (3548928, 3555840, 3647488, 1152000, 1152000)),
        (9, 0, 64): ((5888, 5888, 5888, 5888, 5888),
                         (0, 0, 0, 0, 0)),
        (9, 5, 64): ((5888, 5888, 5888, 5888, 5888),
                         (338944, 339712, 352256, 7936, 7936)),
    },
}
SCREEN_KMAX = 128


def test_the_size_functions_answer_no_less_than_before(lib):
    import test_topk_workspace_cpu as TW
    assert TW.KS == PARENT_KS and set(TW.SHAPES) == set(PARENT_SIZES["defaults"])
    grew = 0
    for key, table in PARENT_SIZES.items():
        lib.anyloc_reset_options()
        for pair in (key.split(",") if key != "defaults" else []):
            name, value = pair.split("=")
            assert lib.anyloc_set_option(name.encode(), int(value)) == 0
        for (nq, ndb, dim), (one_shot, indexed) in table.items():
            for k, was_a, was_b in zip(PARENT_KS, one_shot, indexed):
                now_a, now_b = lib.anyloc_topk_workspace_bytes(nq, ndb, dim, k), lib.anyloc_topk_index_workspace_bytes(nq, ndb, dim, k)
                assert now_a >= was_a and now_b >= was_b, (key, nq, ndb, dim, k)
                if k > SCREEN_KMAX:                         # never screened: nothing to add
                    assert (now_a, now_b) == (was_a, was_b), (key, nq, ndb, dim, k)
                # the side batch: at most 64 gathered rows, their lists, a mark per query and the plan, each rounded up to 256
                side = min(nq, 64)
                most = 4 * side * dim + 12 * side * k + 4 * nq + 4 * 68 + 5 * 256
                assert now_a - was_a <= most and now_b - was_b <= most, (key, nq, ndb, dim, k, now_a - was_a, now_b - was_b)
                grew += (now_a > was_a) + (now_b > was_b)
    assert grew > 0


def test_no_blocking_call_outside_the_documented_exceptions():
    """the scanner of tests/test_stream_contract_cpu.py over the sources as they are now: the device-side fallback added no
    blocking call and no null stream, and the waiting path still holds exactly its hipStreamSynchronize"""
    import test_stream_contract_cpu as L
    hits = L.scan(L._sources())
    assert [h for h in hits if (h[0], h[1]) not in L.ALLOWED] == []
    assert {h[2] for h in hits if h[:2] == ("topk.hip", "topk_impl")} == {"hipStreamSynchronize"}
    assert not [h for h in hits if h[1] in ("device_fallback", "screened_search", "panel_search", "prologue")]
