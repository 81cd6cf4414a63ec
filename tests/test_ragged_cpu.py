"""Ragged batches on a GPU-less host: the new C entry points are declared, bound and exported, reject bad arguments
before any device work, and the Python packing rule (chunks, offsets, tap order) holds on shapes alone."""
import ctypes as C

import numpy as np
import pytest
import torch

RAGGED_SYMBOLS = ("anyloc_vit_workspace_bytes_ragged", "anyloc_vit_forward_ragged", "anyloc_attention_ragged",
                  "anyloc_attention_h3_ragged")


@pytest.fixture(scope="module")
def lib():
    from anyloc_amd import _lib, build
    build.build_library(verbose=False)
    return _lib.load()


def test_ragged_symbols_declared_bound_exported(lib):
    import os
    import re
    from anyloc_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "anyloc_hip.h")).read()
    assert int(re.search(r"#define ANYLOC_ABI_VERSION (\d+)", header).group(1)) == 10
    assert _lib.ABI_VERSION == 10 and lib.anyloc_version() == 10
    raw = C.CDLL(_lib.LIB_PATH)
    for name in RAGGED_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(raw, name), name


@pytest.fixture()
def handle(lib):
    """A ViT-S geometry handle with placeholder (never dereferenced) weight pointers: creating it and validating calls
    touch no device."""
    from anyloc_amd import _lib
    cfg = _lib.VitConfig(384, 2, 6, 0, 1536, 14, 588)
    blocks = (_lib.VitBlockWeights * 2)()
    for i in range(2):
        for f in _lib.BLOCK_FIELDS:
            setattr(blocks[i], f, 4096)
    h = C.c_void_p()
    assert lib.anyloc_vit_create(C.byref(h), C.byref(cfg), 4096, 4096, 4096, blocks) == 0
    yield h
    lib.anyloc_vit_destroy(h)


def _hw(*sizes):
    flat = [v for s in sizes for v in s]
    return (C.c_int32 * max(1, len(flat)))(*flat)


def _forward(lib, h, n_img, hw):
    layers = (C.c_int32 * 1)(1)
    facets = (C.c_int32 * 1)(2)
    return lib.anyloc_vit_forward_ragged(h, 4096, n_img, hw, 4096, 4096, 1, layers, facets, 0, 4096, 4096, 1 << 30, None)


def test_ragged_forward_rejects_bad_arguments(lib, handle):
    assert _forward(lib, None, 1, _hw((224, 224))) == -1
    assert b"null handle" in lib.anyloc_last_error()
    assert _forward(lib, handle, 0, _hw((224, 224))) == -1
    assert b"n_img" in lib.anyloc_last_error()
    assert _forward(lib, handle, -3, _hw((224, 224))) == -1
    assert _forward(lib, handle, 2, _hw((224, 224), (224, 230))) == -1
    msg = lib.anyloc_last_error()
    assert b"image 1" in msg and b"multiple of the patch size 14" in msg
    assert _forward(lib, handle, 1, _hw((0, 224))) == -1
    assert lib.anyloc_vit_forward_ragged(handle, 4096, 1, None, 4096, 4096, 1, (C.c_int32 * 1)(1), (C.c_int32 * 1)(2), 0,
                                         4096, 4096, 1 << 30, None) == -1
    # a valid shape with a null device table is refused too
    assert lib.anyloc_vit_forward_ragged(handle, 4096, 1, _hw((224, 224)), None, 4096, 1, (C.c_int32 * 1)(1),
                                         (C.c_int32 * 1)(2), 0, 4096, 4096, 1 << 30, None) == -1


def test_ragged_workspace_bytes(lib, handle):
    assert lib.anyloc_vit_workspace_bytes_ragged(None, 1, _hw((224, 224))) == 0
    assert lib.anyloc_vit_workspace_bytes_ragged(handle, 0, _hw((224, 224))) == 0
    assert lib.anyloc_vit_workspace_bytes_ragged(handle, 1, _hw((15, 224))) == 0
    assert b"multiple" in lib.anyloc_last_error()
    one = lib.anyloc_vit_workspace_bytes_ragged(handle, 1, _hw((224, 224)))
    # one image: the uniform call's workspace; equal sizes: the uniform batch's
    assert one == lib.anyloc_vit_workspace_bytes(handle, 1, 224, 224) > 0
    assert lib.anyloc_vit_workspace_bytes_ragged(handle, 3, _hw((224, 308), (224, 308), (224, 308))) == \
        lib.anyloc_vit_workspace_bytes(handle, 3, 224, 308)
    mixed = lib.anyloc_vit_workspace_bytes_ragged(handle, 2, _hw((224, 224), (476, 630)))
    assert mixed > lib.anyloc_vit_workspace_bytes(handle, 1, 476, 630)


def test_ragged_attention_rejects_bad_arguments(lib):
    tok = (C.c_int32 * 2)(5, 0)
    assert lib.anyloc_attention_ragged(4096, 4096, 2, tok, 4096, 128, 2, None) == -1
    assert b"image 1" in lib.anyloc_last_error()
    assert lib.anyloc_attention_ragged(4096, 4096, 0, tok, 4096, 128, 2, None) == -1
    assert lib.anyloc_attention_h3_ragged(4096, 4096, 4096, 1, (C.c_int32 * 1)(5), 4096, 100, 2, 4096, 1 << 20, None) == -1


def test_ragged_packing_rule():
    from anyloc_amd.extractor import ragged_chunks, ragged_offsets
    sizes = [(224, 224), (476, 630), (14, 14), (322, 322), (98, 154)]
    T = [257, 1531, 2, 530, 78]
    # greedy in input order; an image above the budget alone
    assert ragged_chunks(sizes, 10 ** 6) == [(0, 5)]
    assert ragged_chunks(sizes, 1600) == [(0, 1), (1, 3), (3, 5)]
    assert ragged_chunks(sizes, 1000) == [(0, 1), (1, 2), (2, 5)]
    assert ragged_chunks(sizes, 1) == [(i, i + 1) for i in range(5)]
    assert ragged_chunks([], 100) == []
    for budget in (1, 300, 800, 1600, 2400, 10 ** 6):
        ch = ragged_chunks(sizes, budget)
        assert ch[0][0] == 0 and ch[-1][1] == len(sizes)
        assert all(a < b and b == c for (a, b), (c, _) in zip(ch, ch[1:] + [(ch[-1][1], None)]))
        for a, b in ch:
            assert b - a == 1 or sum(T[a:b]) <= budget
    tok, out, pix = ragged_offsets(sizes, use_cls=False)
    assert tok.tolist() == np.concatenate([[0], np.cumsum(T)]).tolist()
    assert out.tolist() == np.concatenate([[0], np.cumsum([t - 1 for t in T])]).tolist()
    assert pix.tolist() == np.concatenate([[0], np.cumsum([3 * h * w for h, w in sizes])]).tolist()
    tok_c, out_c, _ = ragged_offsets(sizes, use_cls=True)
    assert out_c.tolist() == tok_c.tolist() == tok.tolist()


def test_packed_pair_is_taken_without_a_copy():
    from anyloc_amd import ops
    packed = torch.randn(10, 8)
    offsets = torch.tensor([0, 3, 3, 10])
    assert ops.is_packed_pair((packed, offsets))
    assert not ops.is_packed_pair([packed, offsets])
    assert not ops.is_packed_pair((torch.randn(3, 8), torch.randn(4, 8)))      # two images, not a pair
    p, off, n_img, D = ops._offsets_for((packed, offsets), torch.device("cpu"))
    assert p.data_ptr() == packed.data_ptr() and n_img == 3 and D == 8
    assert off.dtype == torch.int64 and off.tolist() == [0, 3, 3, 10]


def test_generate_multi_refuses_a_packed_pair_with_cache_ids():
    from anyloc_amd.vlad import VLAD
    v = VLAD(2, 4, cache_dir=None)
    with pytest.raises(ValueError, match="cache ids"):
        v.generate_multi((torch.randn(5, 4), torch.tensor([0, 2, 5])), cache_ids=["a", "b"])


def test_demo_size_rule():
    from anyloc_amd.preprocess import demo_size
    assert demo_size(480, 640) == (None, (476, 630))
    assert demo_size(480, 640, 1024) == (None, (476, 630))
    assert demo_size(1200, 900, 1024) == ((1024, 768), (1022, 756))
    assert demo_size(700, 1500, 1024) == ((477, 1024), (476, 1022))
