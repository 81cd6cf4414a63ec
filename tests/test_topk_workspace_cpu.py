"""Workspace sizes, scoring path and panel height of the retrieval entry points (csrc/topk.hip), no GPU needed: a search
called with ``workspace = NULL`` returns ANYLOC_ERR_WORKSPACE from its size check, after the argument checks and before
the first HIP call, and names the bytes it needs in ``anyloc_last_error()``.  What a call needs must be what the size
function of the ABI answers for its shape under the same options -- the hazard on record (tests/test_vlad_workspace_cpu.py)
is a workspace sized under one option value and a run under another."""
import ctypes as C
import itertools
import os
import re

import pytest

from anyloc_amd import _lib

ERR_WORKSPACE = -2
SLACK = 256                                             # what every size function adds to the carved bytes
RESCORE_PLANES = 2
# (nq, ndb, dim): the shapes of tools/topk_digest.py, each the smallest that reaches one decision of the host code
SHAPES = ((9, 103, 64), (70, 32868, 64),                                    # fp32 panels: one, two
          (5, 300, 4096), (5, 32868, 4096),                                 # few queries: one panel, two
          (70, 300, 256), (70, 8492, 64), (70, 300, 8208),                  # fp16 panels: one, two, two k-chunks
          (5, 8492, 64),                                                    # few queries against a prepared index
          (70, 8492, 256), (70, 131372, 64), (70, 300, 24592), (70, 1000, 256),   # screened
          (300, 20000, 4096), (256, 2048, 1024), (255, 2048, 1024),         # where the defaults choose fp16 panels / screening
          (64, 300, 4096), (65, 300, 4096), (9, 0, 64), (9, 5, 64))
KS = (1, 10, 128, 129, 1024)
OPTION_SETS = ({}, {"topk_h3": 0}, {"topk_h3": 1}, {"topk_screen": 0}, {"topk_screen": 1}, {"topk_h3": 1, "topk_screen": 1},
               {"topk_h3": 1, "topk_screen": 0}, {"topk_fewq_x6": 0}, {"topk_fewq_x6": 1}, {"topk_fewq_x6": 2},
               {"topk_fewq_x6": 2, "topk_fewq_qdma": 0})


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.fail("libanyloc_hip.so not built (python -m anyloc_amd.build)")
    return _lib.load()


@pytest.fixture(autouse=True)
def _restore_options(lib):
    yield
    assert lib.anyloc_reset_options() == 0


@pytest.fixture(scope="module")
def host():
    """small host buffers for the pointers a call checks for NULL; none is read before the workspace check"""
    f = (C.c_float * 64)()
    i = (C.c_int64 * 64)()
    return dict(f=C.addressof(f), i=C.addressof(i), keep=(f, i))


def _needed(lib, status):
    assert status == ERR_WORKSPACE, (status, lib.anyloc_last_error())
    m = re.fullmatch(r"topk: workspace 0 < (\d+)", lib.anyloc_last_error().decode())
    assert m, lib.anyloc_last_error()
    return int(m.group(1))


def _rows_limit(dim):
    """rows of `dim` columns one two-plane fp16 operand image can hold inside 2 GiB of buffer addressing"""
    return ((1 << 31) - 1) // (4 * dim) // 256 * 256


def _expected_path(nq, ndb, dim, h3_mode):
    """the documented rule of option topk_h3 and of the few-query path: 2 = fp16 panels, 1 = few-query split-K, 0 = fp32 panels"""
    if h3_mode != 0 and nq > 64 and dim % 16 == 0 and _rows_limit(dim) >= 256 and \
            (h3_mode > 0 or (nq >= 256 and dim >= 1024 and ndb >= 2048)):
        return 2
    return 1 if nq <= 64 and dim % 32 == 0 and dim >= 4096 else 0


def _set(lib, options):
    for name, value in options.items():
        assert lib.anyloc_set_option(name.encode(), value) == 0


@pytest.mark.parametrize("options", OPTION_SETS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "defaults")
def test_every_search_needs_exactly_what_its_size_function_answers(lib, host, options):
    _set(lib, options)
    f, i = host["f"], host["i"]
    for (nq, ndb, dim), k, metric, flags in itertools.product(SHAPES, KS, (0, 1), (0, 1)):
        case = (nq, ndb, dim, k, metric, flags, options)
        assert lib.anyloc_topk_path(nq, ndb, dim) == _expected_path(nq, ndb, dim, options.get("topk_h3", -1)), case
        st = lib.anyloc_topk(f, nq, f, ndb, dim, k, metric, flags, 0, f, i, None, 0, None)
        assert _needed(lib, st) + SLACK == lib.anyloc_topk_workspace_bytes(nq, ndb, dim, k), case
        if ndb == 0 or dim % 16:
            assert lib.anyloc_topk_index_workspace_bytes(nq, ndb, dim, k) == 0, case
            continue
        sized = lib.anyloc_topk_index_workspace_bytes(nq, ndb, dim, k)
        st = lib.anyloc_topk_search_index(f, nq, f, ndb, dim, k, metric, flags, 0, f, i, None, 0, None)
        assert _needed(lib, st) + SLACK == sized, case
        for rows, fl in ((f, flags), (None, flags | RESCORE_PLANES), (f, flags | RESCORE_PLANES)):
            st = lib.anyloc_topk_search_index_rows(f, nq, rows, f, ndb, dim, k, metric, fl, 0, f, i, None, 0, None)
            assert _needed(lib, st) + SLACK == sized, case


def test_a_workspace_sized_under_one_option_value_is_not_assumed_under_another(lib, host):
    """the sizes do follow the options (so a caller has to size under the options it runs with): fp16 panels and the screened
    search each need more than the path they replace"""
    f, i = host["f"], host["i"]
    nq, ndb, dim, k = 70, 8492, 256, 10
    sizes = {}
    for h3, screen in ((0, 0), (1, 0), (1, 1)):
        _set(lib, {"topk_h3": h3, "topk_screen": screen})
        sizes[h3, screen] = lib.anyloc_topk_workspace_bytes(nq, ndb, dim, k)
        st = lib.anyloc_topk(f, nq, f, ndb, dim, k, 0, 0, 0, f, i, None, 0, None)
        assert _needed(lib, st) + SLACK == sizes[h3, screen]
    assert sizes[1, 1] > sizes[1, 0] > 0 and sizes[1, 0] != sizes[0, 0]


@pytest.mark.parametrize("options", OPTION_SETS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "defaults")
def test_index_panel_is_the_panel_the_index_and_its_workspace_are_sized_for(lib, options):
    _set(lib, options)
    for dim in (64, 4096, 49152, 98304):
        panel = lib.anyloc_topk_index_panel(dim)
        assert panel == min(8192, _rows_limit(dim)) and panel % 64 == 0, dim
        # the index holds one image slot per panel: one row past a panel boundary costs a whole slot
        at, past = lib.anyloc_topk_index_bytes(panel, dim), lib.anyloc_topk_index_bytes(panel + 1, dim)
        assert past - at > 4 * dim * panel > lib.anyloc_topk_index_bytes(panel - 1, dim) - lib.anyloc_topk_index_bytes(panel - 2, dim) >= 0, dim
        # the workspace holds the [nq, min(panel, ndb)] score block and three floats per database row (k = 1024: never
        # screened): it grows by nq + 3 floats per row up to the panel and by 3 beyond it
        for nq in (5, 70):
            ws = [lib.anyloc_topk_index_workspace_bytes(nq, panel + d, dim, 1024) for d in (-64, 0, 64)]
            assert ws[1] - ws[0] == 64 * 4 * (nq + 3) and ws[2] - ws[1] == 64 * 4 * 3, (dim, nq, ws)
    for dim in (8, 24, 100):
        assert lib.anyloc_topk_index_panel(dim) == 0 and lib.anyloc_topk_index_bytes(1000, dim) == 0, dim
