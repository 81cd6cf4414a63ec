"""The rows-free screened retrieval (ANYLOC_TOPK_RESCORE_PLANES, ``FlatIndex(rescore="planes")``, an index built by ranges)
on a machine without a GPU: header, binding and library agree on the new flag and entry points; the panel size; argument
validation before any HIP call; the Python surface; and the numerics the feature rests on -- the two fp16 planes of a
row-scaled split hold every element within 2^-23 of the row maximum, so the float64 scores over those rows (what the new
kernel computes) are within 1e-7 of the scores over the fp32 rows.  The kernel itself: tests/test_gpu_screen_rowsfree.py."""
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import split_fp16_study as sh  # noqa: E402
from _retrieval_refs import planted_rows  # noqa: E402

ERR_ARG, ERR_WORKSPACE = -1, -2


@pytest.fixture(scope="module")
def lib():
    from anyloc_amd import _lib, build
    build.build_library(verbose=False)
    return _lib.load()


def test_header_binding_and_library_agree_on_the_flag_and_the_entry_points(lib):
    from anyloc_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "anyloc_hip.h")).read()
    assert int(re.search(r"#define ANYLOC_TOPK_RESCORE_PLANES (\d+)u", header).group(1)) == 2 == ops.TOPK_RESCORE_PLANES
    assert int(re.search(r"#define ANYLOC_ABI_VERSION (\d+)", header).group(1)) == 10 == lib.anyloc_version()   # additive
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("anyloc_topk_index_panel", "anyloc_topk_index_build_range"):
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S)), name


def test_index_panel(lib):
    assert lib.anyloc_topk_index_panel(49152) == 8192
    assert lib.anyloc_topk_index_panel(64) == 8192
    assert lib.anyloc_topk_index_panel(24) == 0 and lib.anyloc_topk_index_bytes(1000, 24) == 0
    from anyloc_amd import ops
    assert ops.topk_index_panel(49152) == 8192 and ops.topk_index_panel(24) == 0


def test_argument_validation_needs_no_gpu(lib):
    # every data pointer is null: what is rejected here is rejected before any HIP call
    st = lib.anyloc_topk(None, 4, None, 4, 64, 1, 0, 2, 0, None, None, None, 0, None)
    assert st == ERR_ARG and b"ANYLOC_TOPK_RESCORE_PLANES" in lib.anyloc_last_error()
    st = lib.anyloc_topk(None, 4, None, 4, 64, 1, 0, 3, 0, None, None, None, 0, None)
    assert st == ERR_ARG and b"ANYLOC_TOPK_RESCORE_PLANES" in lib.anyloc_last_error()
    st = lib.anyloc_topk(None, 4, None, 4, 64, 1, 0, 4, 0, None, None, None, 0, None)     # (today's path, today's message)
    assert st == ERR_ARG and b"ANYLOC_TOPK_RESCORE_PLANES" not in lib.anyloc_last_error()
    ndb, dim = 20000, 64
    big = lib.anyloc_topk_index_bytes(ndb, dim)
    assert big > 0

    def build_range(row0, nrows, nbytes=big, ndb=ndb, dim=dim):
        return lib.anyloc_topk_index_build_range(None, row0, nrows, ndb, dim, None, nbytes, None), lib.anyloc_last_error()
    st, msg = build_range(100, 8192)
    assert st == ERR_ARG and b"row0" in msg, msg                      # off a panel boundary
    st, msg = build_range(8192, 5000)
    assert st == ERR_ARG and b"nrows" in msg, msg                     # neither whole panels nor the tail
    st, msg = build_range(16384, 8192)
    assert st == ERR_ARG and b"inside" in msg, msg                    # past the last row
    st, msg = build_range(0, 0)
    assert st == ERR_ARG, msg
    st, msg = build_range(-8192, 8192)
    assert st == ERR_ARG, msg
    st, msg = build_range(8192, 8192, nbytes=big - 4096)
    assert st == ERR_WORKSPACE and b"index buffer" in msg, msg        # a short buffer
    for row0, nrows in ((0, 8192), (8192, 8192), (16384, ndb - 16384), (0, ndb), (8192, ndb - 8192)):
        st, msg = build_range(row0, nrows)                            # valid ranges get as far as the pointers
        assert st == ERR_ARG and b"null pointer" in msg, (row0, nrows, msg)
    assert build_range(0, 8192, ndb=20000, dim=24)[0] == -4           # no panels for this width: unsupported


def test_python_surface():
    from anyloc_amd import ops, retrieval
    sig = inspect.signature(retrieval.FlatIndex.__init__)
    assert sig.parameters["rescore"].default == "rows"
    assert list(sig.parameters)[1:6] == ["db", "method", "norm_descs", "planes", "keep_fp32"]     # today's arguments, in place
    assert callable(retrieval.FlatIndex.from_chunks)
    assert list(inspect.signature(retrieval.FlatIndex.from_chunks).parameters) == ["chunks", "ntotal", "dim", "method", "norm_descs"]
    assert inspect.signature(ops.topk_indexed).parameters["rescore_planes"].default is False
    assert list(inspect.signature(ops.topk_index_build_range).parameters) == ["index", "rows", "row0", "ndb"]


@pytest.mark.parametrize("nq,ndb,dim", [(64, 4000, 4096), (16, 600, 49152), (64, 4000, 512)])
def test_scores_over_the_rows_the_planes_hold(nq, ndb, dim):
    """(hi + lo) 2^-e: every element within 2^-23 of its row's maximum.  The row is scaled so that its maximum lies in
    [2^14, 2^15); hi = fp16 of an element leaves a rest of at most half an ulp of hi, <= 8; lo = fp16 of that rest is off by at
    most half an ulp of a number below 8, 2^-9 (8 itself is exact) -- against a maximum of at least 2^14.  The normalised
    float64 score of a unit query then moves by < 1e-7 (measured 3.5e-9 / 9.6e-10 / 9.7e-9 at these widths): thirty times under
    the 3e-6 bar of the retrieval tests."""
    qu, db = planted_rows(nq, ndb, dim, nq + ndb + dim, device="cpu")
    h, l, scale = sh.split_h2(db)
    amax = db.abs().amax(dim=1, keepdim=True).double()
    held = (h.double() + l.double()) / scale.double()
    elem = float(((held - db.double()).abs() / amax).max())
    assert elem <= 2.0 ** -23, elem
    nrm = db.double().norm(dim=1)
    s = qu.double() @ (db.double() / nrm[:, None]).t()
    s_held = qu.double() @ (held / nrm[:, None]).t()
    moved = float((s - s_held).abs().max())
    print(f"dim {dim}: element error {elem:.3e} of the row maximum (2^-23 = {2.0 ** -23:.3e}), scores move by {moved:.2e}")
    assert moved < 1e-7, moved
