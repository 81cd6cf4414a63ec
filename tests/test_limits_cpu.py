"""The far side of every documented argument limit (include/anyloc_hip.h), no GPU needed: a call one step outside a range
returns ANYLOC_ERR_INVALID_ARG from its argument checks, in front of the first HIP call, and says so in
``anyloc_last_error()``.  Small host buffers stand in for the pointers (tests/test_topk_workspace_cpu.py): none is read.
The near side of the same limits runs on the GPU, tests/test_gpu_limits.py; its k-means inputs are checked here for the
two properties that test relies on."""
import ctypes as C
import os

import pytest
import torch

import _limits_cases as LC
from anyloc_amd import _lib

ERR_INVALID_ARG = -1
WS = 1 << 20               # workspace bytes claimed (never touched: the argument checks come first)


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.fail("libanyloc_hip.so not built (python -m anyloc_amd.build)")
    return _lib.load()


@pytest.fixture(scope="module")
def host():
    """small host buffers for the pointers a call checks for NULL; none is read before the argument checks"""
    f = (C.c_float * 64)()
    i = (C.c_int64 * 64)()
    return dict(f=C.addressof(f), i=C.addressof(i), f3=C.cast(f, C.POINTER(C.c_float)), keep=(f, i))


def _refused(lib, status, *words):
    """the status is ANYLOC_ERR_INVALID_ARG and the message of THIS call names what was wrong"""
    msg = lib.anyloc_last_error().decode()
    assert status == ERR_INVALID_ARG, (status, msg)
    for w in words:
        assert w in msg, (w, msg)


def _clear(lib):
    """leave a message of another call behind, so that a stale one cannot pass for the refusal under test"""
    assert lib.anyloc_set_option(b"no_such_option", 0) == ERR_INVALID_ARG
    assert b"1025" not in lib.anyloc_last_error() and b"65535" not in lib.anyloc_last_error()


@pytest.mark.parametrize("k", [0, 1025])
def test_topk_list_length_outside_1_1024(lib, host, k):
    f, i = host["f"], host["i"]
    for nq, ndb, dim in ((9, 103, 64), (5, 300, 4096), (70, 8492, 256)):      # a shape of each scoring path
        _clear(lib)
        _refused(lib, lib.anyloc_topk(f, nq, f, ndb, dim, k, 0, 0, 0, f, i, f, WS, None), f"k={k}", "[1,1024]")
        if dim % 16 == 0:
            _clear(lib)
            _refused(lib, lib.anyloc_topk_search_index(f, nq, f, ndb, dim, k, 0, 0, 0, f, i, f, WS, None), f"k={k}", "[1,1024]")
            _clear(lib)
            _refused(lib, lib.anyloc_topk_search_index_rows(f, nq, f, f, ndb, dim, k, 1, 0, 0, f, i, f, WS, None), f"k={k}", "[1,1024]")


def test_topk_accepts_both_ends_of_the_range_up_to_its_workspace_check(lib, host):
    """k = 1 and 1024 pass the argument checks: with no workspace the call gets as far as the size check (-2)."""
    f, i = host["f"], host["i"]
    for k in (1, 1024):
        assert lib.anyloc_topk(f, 9, f, 103, 64, k, 0, 0, 0, f, i, None, 0, None) == -2, lib.anyloc_last_error()


@pytest.mark.parametrize("K,D,words", [(0, 64, ("num_clusters 0", "[1,256]")), (257, 64, ("num_clusters 257", "[1,256]")),
                                       (32, 6, ("desc_dim 6", "multiple of 4"))])
def test_vlad_hard_cluster_count_and_width(lib, host, K, D, words):
    f, i = host["f"], host["i"]
    _clear(lib)
    _refused(lib, lib.anyloc_vlad_hard(f, i, 1, 4, D, f, K, 3, f, None, f, WS, None), *words)


def test_vlad_soft_serves_64_clusters_at_most(lib, host):
    f, i = host["f"], host["i"]
    _clear(lib)
    _refused(lib, lib.anyloc_vlad_soft(f, i, 1, 4, 64, f, 65, 1.0, 3, f, f, WS, None), "65", "64")
    _clear(lib)
    _refused(lib, lib.anyloc_vlad_soft_weights(f, 4, 64, f, 65, 1.0, f, f, WS, None), "K <= 64")
    _clear(lib)
    _refused(lib, lib.anyloc_vlad_soft(f, i, 1, 4, 64, f, 257, 1.0, 3, f, f, WS, None), "257", "[1,256]")


def test_vlad_assigned_cluster_counts(lib, host):
    f, i = host["f"], host["i"]
    _clear(lib)
    _refused(lib, lib.anyloc_vlad_assigned(f, 4, 64, f, 65, None, f, 3, f, f, WS, None), "soft weights", "K <= 64")
    _clear(lib)
    _refused(lib, lib.anyloc_vlad_assigned(f, 4, 64, f, 257, i, None, 3, f, f, WS, None), "K in [1, 256]")
    _clear(lib)
    _refused(lib, lib.anyloc_vlad_assigned(f, 4, 64, f, 257, None, f, 3, f, f, WS, None), "K in [1, 256]")


def test_kmeans_step_cluster_count_and_rows(lib, host):
    f, i = host["f"], host["i"]
    _clear(lib)
    _refused(lib, lib.anyloc_kmeans_step(f, 8, 64, f, 257, 0, f, f, i, f, WS, None), "K 257", "[1,256]")
    _clear(lib)
    _refused(lib, lib.anyloc_kmeans_step(f, 0, 64, f, 16, 0, f, f, i, f, WS, None), "no rows")


def test_65536_images_or_planes(lib, host):
    """one more than a 16-bit grid dimension holds: refused by name, in front of every HIP call"""
    f, i = host["f"], host["i"]
    n = 65536
    _clear(lib)
    _refused(lib, lib.anyloc_pool_tokens(f, None, n, 2, 8, 0, 3.0, f, None), "n_img=65536", "[1, 65535]")
    _clear(lib)
    _refused(lib, lib.anyloc_pool_tokens(f, i, n, -1, 8, 2, 3.0, f, None), "n_img=65536", "[1, 65535]")
    _clear(lib)
    _refused(lib, lib.anyloc_attention(f, f, n, 2, 64, 1, None), "batch 65536", "[1, 65535]")
    _clear(lib)
    _refused(lib, lib.anyloc_attention_h3(f, f, f, n, 2, 64, 1, f, 1 << 40, None), "batch 65536", "[1, 65535]")
    _clear(lib)
    _refused(lib, lib.anyloc_preprocess_u8(f, n, 14, 14, 14, 14, host["f3"], host["f3"], f, None), "batch 65536", "[1, 65535]")
    _clear(lib)
    _refused(lib, lib.anyloc_resize_bicubic(f, n, 14, 14, 7, 7, 0, 0, 7, 7, f, None), "planes 65536", "[1, 65535]")


def test_ops_pool_names_the_image_limit():
    """ops.pool refuses 65 536 images itself -- a ValueError that names the limit, raised before a device is asked for."""
    from anyloc_amd import ops
    with pytest.raises(ValueError, match="65535"):
        ops.pool(torch.zeros(65536, 1, 4), "average")
    offsets = torch.arange(65537, dtype=torch.int64)
    with pytest.raises(ValueError, match="65535"):
        ops.pool((torch.zeros(65536, 4), offsets), "max")


@pytest.mark.parametrize("K,D,n,mode", LC.KMEANS_CASES)
def test_kmeans_cases_of_the_gpu_module_keep_their_premises(K, D, n, mode):
    """What tests/test_gpu_limits.py::test_kmeans_step_large_k relies on, from the oracle alone: its fp32 arg-max and a
    float64 arg-max differ on at most LABEL_TIE_CAP rows (so at most that many labels can sit on an fp32 near-tie), the
    two far centres -- and only clusters nobody needs -- stay empty, and every other cluster pattern is ordinary."""
    x, c = LC.kmeans_case(K, D, n)
    lab32 = LC.oracle_sim(x, c, mode).max(dim=-1)[1]
    lab64 = LC.oracle_sim(x.double(), c.double(), mode).max(dim=-1)[1]
    differ = int((lab32 != lab64).sum())
    counts = torch.bincount(lab32, minlength=K)
    print(f"[kmeans K={K} D={D} {mode}] fp32 / float64 arg-max differ on {differ} rows; {int((counts == 0).sum())} empty clusters")
    assert differ <= LC.LABEL_TIE_CAP
    assert int(counts[K - 2:].sum()) == 0 and int((counts > 0).sum()) >= K // 2
