"""Workspace sizes and workgroups-per-image of the VLAD / k-means entry points (csrc/vlad.hip), no GPU needed: every entry
point called with ``workspace = NULL`` returns ANYLOC_ERR_WORKSPACE from its size check, before any launch, and names the
bytes it needs in ``anyloc_last_error()``.  What a call needs must fit what the size function of the ABI answers for it --
the hazard on record here is a workspace sized for one workgroups-per-image count and a run with another."""
import ctypes as C
import itertools
import os
import re

import pytest

from anyloc_amd import _lib

ERR_INVALID_ARG, ERR_WORKSPACE = -1, -2
DS = (64, 384, 1536)
KS = (1, 32, 33, 129, 256)
BATCHES = ((1, 40), (5, 400), (300, 158_700))           # (images, tokens of all images)
ASKED = (0, 3, 64)                                      # ANYLOC_VLAD_PARTS of the call (0 = the library's count)
OPTION_SETS = ({}, {"vlad_parts": 4}, {"vlad_two_pass": 1})
SLACK = 256                                             # what every size function adds to the carved bytes


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.fail("libanyloc_hip.so not built (python -m anyloc_amd.build)")
    return _lib.load()


@pytest.fixture(scope="module")
def host():
    """small host buffers for the pointers a call checks for NULL; none is read before the workspace check"""
    f = (C.c_float * 64)()
    offsets = (C.c_int64 * 301)()
    labels = (C.c_int64 * 64)()
    return dict(f=C.addressof(f), offsets=C.addressof(offsets), labels=C.addressof(labels), keep=(f, offsets, labels))


def _needed(lib, status, who):
    assert status == ERR_WORKSPACE, (who, status, lib.anyloc_last_error())
    m = re.fullmatch(rf"{who}: workspace 0 < (\d+)", lib.anyloc_last_error().decode())
    assert m, lib.anyloc_last_error()
    return int(m.group(1))


def _fused_shape(D, K):
    return 1 <= K <= 32 and D in (384, 768, 1024, 1536)


def _library_parts(lib, total, n_img, D, K):
    """the library's own count for the batch (option vlad_parts included): auto_parts with the two-pass option off"""
    saved = C.c_int64()
    assert lib.anyloc_get_option(b"vlad_two_pass", C.byref(saved)) == 0
    lib.anyloc_set_option(b"vlad_two_pass", 0)
    p = lib.anyloc_vlad_auto_parts(total, n_img, D, K)
    lib.anyloc_set_option(b"vlad_two_pass", saved.value)
    return p


@pytest.mark.parametrize("options", OPTION_SETS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "defaults")
def test_every_vlad_call_fits_the_workspace_its_size_function_answers(lib, host, options):
    for name, value in options.items():
        assert lib.anyloc_set_option(name.encode(), value) == 0
    two_pass = bool(options.get("vlad_two_pass"))
    for D, K, (n_img, total), asked in itertools.product(DS, KS, BATCHES, ASKED):
        case = (D, K, n_img, total, asked, options)
        fused = _fused_shape(D, K)
        own = _library_parts(lib, total, n_img, D, K)
        assert own == 1 or fused, case
        if "vlad_parts" in options and fused:
            assert own == options["vlad_parts"], case
        assert lib.anyloc_vlad_auto_parts(total, n_img, D, K) == (1 if two_pass else own), case
        sized = max(own, asked) if fused else 1                                      # what ..._bytes_parts sizes for
        runs = 1 if (not fused or two_pass) else (asked or own)                     # what anyloc_vlad_hard runs with
        size_parts = lib.anyloc_vlad_workspace_bytes_parts(total, n_img, D, K, asked)
        size_own = lib.anyloc_vlad_workspace_bytes(total, n_img, D, K)
        assert size_own == lib.anyloc_vlad_workspace_bytes_parts(total, n_img, D, K, 0) <= size_parts, case

        st = lib.anyloc_vlad_hard(host["f"], host["offsets"], n_img, total, D, host["f"], K, 3 | (asked << 8), host["f"], None,
                                  None, 0, None)
        need = _needed(lib, st, "vlad_hard")
        assert need + SLACK <= size_parts, case
        if runs == sized:
            assert need + SLACK == size_parts, case

        # soft assignment and the given-assignment call run one workgroup per image whatever the shape
        st = lib.anyloc_vlad_soft(host["f"], host["offsets"], n_img, total, D, host["f"], K, 1.0, 3, host["f"], None, 0, None)
        if K > 64:
            assert st == ERR_INVALID_ARG, case
        else:
            need = _needed(lib, st, "vlad_soft")
            assert need + SLACK <= size_own, case
            if own == 1:
                assert need + SLACK == size_own, case
        if n_img == 1:
            size_one = lib.anyloc_vlad_workspace_bytes(total, 1, D, K)
            for labels, soft in ((host["labels"], None), (None, host["f"])):
                st = lib.anyloc_vlad_assigned(host["f"], total, D, host["f"], K, labels, soft, 3, host["f"], None, 0, None)
                if soft and K > 64:
                    assert st == ERR_INVALID_ARG, case
                    continue
                need = _needed(lib, st, "vlad_assigned")
                assert need + SLACK <= size_one, case
                if own == 1:
                    assert need + SLACK == size_one, case
            if K <= 64:
                st = lib.anyloc_vlad_soft_weights(host["f"], total, D, host["f"], K, 1.0, host["f"], None, 0, None)
                assert _needed(lib, st, "vlad_soft_weights") + SLACK <= size_one, case


@pytest.mark.parametrize("max_chunks", (0, 1, 3))
def test_kmeans_step_needs_exactly_what_its_size_function_answers(lib, host, max_chunks):
    """anyloc_kmeans_step compares against anyloc_kmeans_workspace_bytes itself: the figure in its message is that value, slack
    included (both take the chunk count from the same function, whatever option kmeans_max_chunks says)"""
    assert lib.anyloc_set_option(b"kmeans_max_chunks", max_chunks) == 0
    for D, K, n, mode in itertools.product(DS, KS, (1, 1024, 3000, 300_000), (0, 1)):
        st = lib.anyloc_kmeans_step(host["f"], n, D, host["f"], K, mode, host["f"], host["f"], None, None, 0, None)
        assert _needed(lib, st, "kmeans_step") == lib.anyloc_kmeans_workspace_bytes(n, D, K), (D, K, n, mode)
    # more rows never need less, and one chunk is the floor
    assert lib.anyloc_kmeans_workspace_bytes(300_000, 1536, 32) >= lib.anyloc_kmeans_workspace_bytes(3000, 1536, 32)


def test_auto_parts_follows_the_options(lib):
    for D, K, (n_img, total) in itertools.product(DS, KS, BATCHES):
        fused = _fused_shape(D, K)
        free = lib.anyloc_vlad_auto_parts(total, n_img, D, K)
        assert 1 <= free <= 8 and (fused or free == 1), (D, K, n_img)
        lib.anyloc_set_option(b"vlad_parts", 4)
        assert lib.anyloc_vlad_auto_parts(total, n_img, D, K) == (4 if fused else 1), (D, K, n_img)
        lib.anyloc_set_option(b"vlad_two_pass", 1)
        assert lib.anyloc_vlad_auto_parts(total, n_img, D, K) == 1, (D, K, n_img)
        lib.anyloc_reset_options()
    assert lib.anyloc_vlad_auto_parts(0, 0, 1536, 32) == 1
