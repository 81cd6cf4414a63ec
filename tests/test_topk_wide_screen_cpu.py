"""The screened search on rows wider than 49 152 columns, as far as it shows without a GPU (csrc/topk.hip: topk_plan, carve):
the technique of tests/test_topk_workspace_cpu.py -- a search called with ``workspace = NULL`` names the bytes it needs, after
the argument checks and before the first HIP call.  A shape screens exactly when its workspace under ``topk_screen = 1`` is
larger than under ``topk_screen = 0`` (the leading-plane score buffer, the candidate lists, the side batch); while rows above
49 152 columns were not screened the two sizes were equal at every width here.  The column range of a screened search must be
a whole number of panels: from 65 536 columns on the panel (rows of one operand image inside 2 GiB) no longer divides 131 072,
and a second range that began inside a panel could not be served from a prepared index.  Two column ranges at these widths
need more than 130 000 rows of >= 256 KiB each: no GPU test reaches them, this file pins their sizes."""
import ctypes as C
import itertools
import os
import re

import pytest

from anyloc_amd import _lib

ERR_ARG = -1
ERR_WORKSPACE = -2
SLACK = 256                                             # what every size function adds to the carved bytes
NORMALIZE_DB, RESCORE_PLANES, NO_WAIT = 1, 2, 4
SHAPES = ((70, 3000, 65536), (70, 4000, 81920), (70, 4000, 98304), (70, 4000, 131072), (70, 2700, 196608))
PANELS = {49152: 8192, 65536: 7936, 81920: 6400, 98304: 5376, 131072: 3840, 196608: 2560}
SCREEN = {"topk_screen": 1, "topk_h3": 1}
UNSCREENED = {"topk_screen": 0, "topk_h3": 1}


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


def _set(lib, options):
    for name, value in options.items():
        assert lib.anyloc_set_option(name.encode(), value) == 0, (name, value, lib.anyloc_last_error())


def _get(lib, name):
    v = C.c_int64(-12345)
    assert lib.anyloc_get_option(name.encode(), C.byref(v)) == 0
    return v.value


@pytest.mark.parametrize("nq,ndb,dim", SHAPES)
def test_wide_rows_screen_up_to_k_128(lib, nq, ndb, dim):
    """topk_screen = 1 plans the screened search at every width the fp16 panels serve: for k <= 128 the one-shot and the
    indexed workspace are larger than under topk_screen = 0, by at least the [nq, range] buffer of leading-plane scores;
    at k = 129 (never screened) they are equal.  The slice width of the re-scoring kernels changes no size."""
    sizes = {}
    for cols, (tag, options) in itertools.product((0, 4096), (("screen", SCREEN), ("plain", UNSCREENED))):
        _set(lib, dict(options, topk_rescore_cols=cols))
        for k in (1, 10, 128, 129):
            sizes[cols, tag, k] = (lib.anyloc_topk_workspace_bytes(nq, ndb, dim, k), lib.anyloc_topk_index_workspace_bytes(nq, ndb, dim, k))
    panel = PANELS[dim]
    covered = -(-ndb // panel) * panel                      # the panels that cover the database: one column range
    for cols, k in itertools.product((0, 4096), (1, 10, 128)):
        for which in (0, 1):
            assert sizes[cols, "screen", k][which] >= sizes[cols, "plain", k][which] + 4 * nq * covered > 0, (cols, k, which, sizes)
    for cols in (0, 4096):
        assert sizes[cols, "screen", 129] == sizes[cols, "plain", 129], (cols, sizes)
    for tag, k in itertools.product(("screen", "plain"), (1, 10, 128, 129)):
        assert sizes[0, tag, k] == sizes[4096, tag, k], (tag, k, sizes)


@pytest.mark.parametrize("options", [SCREEN, dict(SCREEN, topk_rescore_cols=4096), UNSCREENED, {}],
                         ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "defaults")
def test_every_search_of_wide_rows_needs_exactly_what_its_size_function_answers(lib, host, options):
    _set(lib, options)
    f, i = host["f"], host["i"]
    for (nq, ndb, dim), k, metric, flags in itertools.product(SHAPES, (1, 10, 128, 129), (0, 1),
                                                              (0, NORMALIZE_DB, NO_WAIT, NORMALIZE_DB | NO_WAIT)):
        case = (nq, ndb, dim, k, metric, flags, options)
        st = lib.anyloc_topk(f, nq, f, ndb, dim, k, metric, flags, 0, f, i, None, 0, None)
        assert _needed(lib, st) + SLACK == lib.anyloc_topk_workspace_bytes(nq, ndb, dim, k), case
        sized = lib.anyloc_topk_index_workspace_bytes(nq, ndb, dim, k)
        assert sized > 0, case
        st = lib.anyloc_topk_search_index(f, nq, f, ndb, dim, k, metric, flags, 0, f, i, None, 0, None)
        assert _needed(lib, st) + SLACK == sized, case
        for rows, fl in ((f, flags), (None, flags | RESCORE_PLANES), (f, flags | RESCORE_PLANES)):
            st = lib.anyloc_topk_search_index_rows(f, nq, rows, f, ndb, dim, k, metric, fl, 0, f, i, None, 0, None)
            assert _needed(lib, st) + SLACK == sized, case


@pytest.mark.parametrize("dim", sorted(PANELS))
def test_a_column_range_is_a_whole_number_of_panels(lib, dim):
    """E(m) = what screening adds to the indexed workspace of 70 queries against m panels.  Only the [70, range] score buffer
    grows with the database (an indexed search keeps no per-row residuals of its own), and the range is
    min(the panels that cover the database, the largest panel multiple <= 131 072): one more panel adds 4 * 70 * panel bytes
    while the database fits one range (m < M = 131 072 // panel) and nothing from there on.  (m starts at 1: no index holds an
    empty database.)  49 152 columns: the 8192-row panel divides 131 072, M = 16, as before."""
    panel = lib.anyloc_topk_index_panel(dim)
    assert panel == PANELS[dim]
    M = 131072 // panel
    nq, k = 70, 10

    def extra(m):
        _set(lib, SCREEN)
        a = lib.anyloc_topk_index_workspace_bytes(nq, m * panel, dim, k)
        _set(lib, UNSCREENED)
        b = lib.anyloc_topk_index_workspace_bytes(nq, m * panel, dim, k)
        assert a > b > 0, (dim, m, a, b)
        return a - b
    e = {m: extra(m) for m in range(1, M + 3)}
    for m in range(1, M):
        assert e[m + 1] - e[m] == 4 * nq * panel, (dim, m, e[m], e[m + 1])
    for m in (M, M + 1):
        assert e[m + 1] - e[m] == 0, (dim, m, e[m], e[m + 1])


def test_option_topk_rescore_cols(lib):
    """0 (default: 49 152 columns per slice, narrower rows on the single-slice kernels) or a positive multiple of 4096 up to
    49 152; anything else is refused and leaves the value as it was."""
    assert _get(lib, "topk_rescore_cols") == 0
    for bad in (-1, -4096, 1, 16, 4095, 4097, 6144, 49152 + 4096):
        assert lib.anyloc_set_option(b"topk_rescore_cols", bad) == ERR_ARG, bad
        assert b"topk_rescore_cols" in lib.anyloc_last_error()
        assert _get(lib, "topk_rescore_cols") == 0, bad
    for good in (4096, 8192, 49152, 0):
        assert lib.anyloc_set_option(b"topk_rescore_cols", good) == 0, good
        assert _get(lib, "topk_rescore_cols") == good
    _set(lib, {"topk_rescore_cols": 4096})
    assert lib.anyloc_reset_options() == 0
    assert _get(lib, "topk_rescore_cols") == 0
