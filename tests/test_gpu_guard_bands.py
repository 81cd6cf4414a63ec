"""Guard bands: no entry point writes outside its buffers (include/anyloc_hip.h, "Buffers").

Every case calls one entry point through ``_lib.load()`` with pointers into the arena of tests/_guard_arena.py: outputs and
the workspace are views of EXACTLY the documented size (the header's own size functions, called under the options of the
run), 0xFF-filled, between 0xA5 guard bands; inputs lie there too and are compared with their copies.  A case asserts

  * status 0;
  * no findings: no guard byte, no gap byte of a strided output (columns [N, ldc)) and no input changed, every element of
    an output's documented extent written;
  * the result is bit-equal to the same entry called the ordinary way (the ops.* wrapper, or the same call on plain
    ``torch.empty`` tensors where no wrapper reaches the entry): independent of placement and stride;
  * where there is a workspace, a second guarded run with twice the bytes gives the same bits.

The strided GEMM / split cases are new code paths: they are also held against float64 with the error measure and bound of
the entry's parity test (tests/test_gpu_kernels.py::test_gemm_nt, tests/test_gpu_x6.py).

What the harness cannot see: a store that lands beyond the 4 MiB guard at either end of the arena, and a store into a live
output element or workspace byte that the call is allowed to write anyway.  tests/test_guard_arena_cpu.py proves that each
kind of finding is reported.  All writes a case can provoke stay inside its own arena; no buffer is ever smaller than the
documented size.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import _plan_edges as PE
from _guard_arena import ALIGN, GUARD, Arena, guarded_workspace
from _stream_harness import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_INVALID_ARG = -1
COUNTS = {}                  # family -> guarded calls made (printed by the last test of the file)
COVERS = {}                  # entry point -> the test functions that declare a guarded case of it


def covers(*names):
    def deco(fn):
        for n in names:
            COVERS.setdefault(n, []).append(fn.__name__)
        return fn
    return deco


@pytest.fixture(scope="module")
def lib():
    from anyloc_amd import _lib
    return _lib.load()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def S():
    from anyloc_amd import _lib
    return _lib.stream_ptr()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _guard_for(ld, item=4):
    """the between-region guard of a case whose widest output row has ``ld`` elements: more than one 256-row tile row"""
    return max(GUARD, (256 * ld * item + ALIGN) // ALIGN * ALIGN)


def _arena(row_bytes, payload, regions=8):
    """an arena for ``payload`` bytes of regions whose guards exceed one 256-row tile row of the widest output row
    (``row_bytes``) -- the condition of tests/_guard_arena.py, met case by case.  A plane image counts with ALL the bytes it
    holds per matrix row (planes x K padded to 16 x 2 bytes), whatever its blocked layout."""
    guard = max(GUARD, (256 * row_bytes + ALIGN) // ALIGN * ALIGN)
    return Arena(DEV, payload + (regions + 1) * (guard + ALIGN), guard=guard)


def _finish(family, ar, st, lib, refs, pad=None, what=""):
    """the verdict of one guarded call: status, findings, bits (``refs``: {output: the ordinary call's tensor, or None})"""
    torch.cuda.synchronize()
    assert st == 0, (what, st, lib.anyloc_last_error())
    findings = ar.check(refs, pad)
    assert findings == [], (what, findings)
    for name, want in refs.items():
        if want is not None:
            got = ar.region(name).view
            assert same_bits(got, want.reshape(got.shape)), (what, name, "differs from the ordinary call")
    COUNTS[family] = COUNTS.get(family, 0) + 1


def test_the_planted_faults_are_found_on_the_device_too(monkeypatch):
    """the five planted faults of tests/test_guard_arena_cpu.py (plain torch stores inside the arena) with the arena on the
    GPU: check() reports each once, with region and offset, from device memory as well"""
    import test_guard_arena_cpu as G
    monkeypatch.setattr(G, "DEVICE", DEV)
    for fn in (G.test_layout_alignment_sizes_and_fill, G.test_a_correct_op_has_no_findings, G.test_store_past_an_output_is_found,
               G.test_store_before_an_output_is_found, G.test_store_into_a_stride_gap_is_found,
               G.test_an_unwritten_output_element_is_found, G.test_a_changed_input_is_found_unless_declared_in_place):
        fn()


# ================================================================ rows ====

@covers("anyloc_l2norm_rows")
@pytest.mark.parametrize("rows,dim", [(1, 1), (5, 10), (7, 384), (3, 49152)])
def test_l2norm_rows(lib, rows, dim):
    from anyloc_amd import ops
    x = torch.randn(rows, dim, generator=_gen(rows + dim), device=DEV) * 3
    want = ops.l2norm_rows(x)
    ar = _arena(4 * dim, 8 << 20)
    xin, out = ar.input("x", x), ar.output("out", torch.float32, (rows, dim))
    st = lib.anyloc_l2norm_rows(P(xin), P(out), rows, dim, 1e-12, S())
    _finish("rows", ar, st, lib, {"out": want}, what=("l2norm", rows, dim))
    # x == out, the documented aliasing
    ar = _arena(4 * dim, 8 << 20)
    xio = ar.input("x", x, in_place=True)
    st = lib.anyloc_l2norm_rows(P(xio), P(xio), rows, dim, 1e-12, S())
    _finish("rows", ar, st, lib, {}, what=("l2norm in place", rows, dim))
    assert same_bits(xio, want)


@covers("anyloc_layernorm")
@pytest.mark.parametrize("rows,dim", [(11, 384), (9, 1024), (3, 1536)])
def test_layernorm(lib, rows, dim):
    from anyloc_amd import ops
    g = _gen(rows * dim)
    x = torch.randn(rows, dim, generator=g, device=DEV) * 2 + 0.5
    w, b = torch.randn(dim, generator=g, device=DEV), torch.randn(dim, generator=g, device=DEV)
    want = ops.layernorm(x, w, b, 1e-6)
    ar = _arena(4 * dim, 8 << 20)
    xin, win, bin_ = ar.input("x", x), ar.input("w", w), ar.input("b", b)
    out = ar.output("y", torch.float32, (rows, dim))
    st = lib.anyloc_layernorm(P(xin), P(out), P(win), P(bin_), rows, dim, 1e-6, S())
    _finish("rows", ar, st, lib, {"y": want}, what=("layernorm", rows, dim))


@covers("anyloc_rope_rows")
def test_rope_rows_in_place(lib):
    """two images of 5 + 6 rows (one prefix row each), 2 heads, the ragged table: q and k of the patch rows are rotated in
    place, the v columns and the prefix rows keep their bits"""
    from anyloc_amd import ops
    heads, D, prefix = 2, 128, 1
    g = _gen(3)
    qkv = torch.randn(11, 3 * D, generator=g, device=DEV)
    table = torch.randn(9, 64, generator=g, device=DEV)
    meta = torch.zeros(5, 3, dtype=torch.int64)
    meta[0] = torch.tensor([0, 5, 11])
    meta[2, :2] = torch.tensor([0, 4])
    want = ops.rope_rows(qkv, heads, table, prefix=prefix, meta=meta)
    ar = _arena(4 * 3 * D, 8 << 20)
    q = ar.input("qkv", qkv, in_place=True)
    t, m = ar.input("table", table), ar.input("meta", meta.to(DEV))
    st = lib.anyloc_rope_rows(P(q), 11, heads, P(t), 0, prefix, P(m), 2, S())
    _finish("rows", ar, st, lib, {}, what="rope_rows")
    assert same_bits(q, want)
    assert torch.equal(q[:, 2 * D:], qkv[:, 2 * D:]) and torch.equal(q[0], qkv[0]) and torch.equal(q[5], qkv[5])
    assert not torch.equal(q[1:5, :2 * D], qkv[1:5, :2 * D])


@covers("anyloc_preprocess_u8")
@pytest.mark.parametrize("B,H,W", [(2, 126, 155), (2, 30, 45)])
def test_preprocess_u8(lib, B, H, W):
    from anyloc_amd import preprocess, synth
    u8 = torch.randint(0, 256, (B, H, W, 3), generator=torch.Generator().manual_seed(H + W), dtype=torch.uint8).to(DEV)
    want = preprocess.images_to_input(u8)
    ch, cw = H // 14 * 14, W // 14 * 14
    assert tuple(want.shape) == (B, 3, ch, cw)
    ar = _arena(4 * cw, 8 << 20)
    img, out = ar.input("img", u8), ar.output("out", torch.float32, (B, 3, ch, cw))
    mean, std = (C.c_float * 3)(*synth.IMAGENET_MEAN), (C.c_float * 3)(*synth.IMAGENET_STD)
    st = lib.anyloc_preprocess_u8(P(img), B, H, W, ch, cw, mean, std, P(out), S())
    _finish("rows", ar, st, lib, {"out": want}, what=("preprocess_u8", B, H, W))


@covers("anyloc_resize_bicubic")
def test_resize_bicubic_off_centre_window(lib):
    """3 planes of 61 x 47 -> 90 x 61, of which only the window 84 x 56 at (5, 1) is written: the same pixels as that window
    of the whole resized image (every output pixel is computed on its own)"""
    from anyloc_amd import preprocess
    x = torch.randn(1, 3, 61, 47, generator=_gen(5), device=DEV)
    want = preprocess.resize_bicubic(x, (90, 61))[0, :, 5:89, 1:57].contiguous()
    ar = _arena(4 * 56, 8 << 20)
    xin, out = ar.input("in", x[0]), ar.output("out", torch.float32, (3, 84, 56))
    st = lib.anyloc_resize_bicubic(P(xin), 3, 61, 47, 90, 61, 5, 1, 84, 56, P(out), S())
    _finish("rows", ar, st, lib, {"out": want}, what="resize_bicubic")


def _pool_cases():
    g = torch.Generator().manual_seed(8)
    uniform = [torch.randn(2, 7, 3, generator=g), torch.randn(4, 37, 100, generator=g)]
    ragged = [[torch.randn(n, 100, generator=g) for n in (5, 0, 37)], [torch.randn(n, 3, generator=g) for n in (7, 1, 2)]]
    return uniform, ragged


@covers("anyloc_pool_tokens")
@pytest.mark.parametrize("mode", ["average", "max", "gem", "gem_abs"])
def test_pool_tokens(lib, mode):
    """uniform batches and ragged ones, one of them with an empty image in the middle (torch.max has no answer for an empty
    image and the wrapper refuses it: that batch runs the three other modes)"""
    from anyloc_amd import ops
    uniform, ragged = _pool_cases()
    for t in uniform:
        n_img, n_tok, D = t.shape
        want = ops.pool(t.to(DEV), mode)
        ar = _arena(4 * D, 8 << 20)
        tin, out = ar.input("tokens", t), ar.output("out", torch.float32, (n_img, D))
        st = lib.anyloc_pool_tokens(P(tin), None, n_img, n_tok, D, ops.POOL_MODES[mode], 3.0, P(out), S())
        _finish("rows", ar, st, lib, {"out": want}, what=("pool", mode, tuple(t.shape)))
    for parts in ragged:
        if mode == "max" and any(len(p) == 0 for p in parts):
            continue
        want = ops.pool([p.to(DEV) for p in parts], mode)
        off = torch.tensor([0] + list(itertools.accumulate(len(p) for p in parts)), dtype=torch.int64)
        D = parts[0].shape[1]
        ar = _arena(4 * D, 8 << 20)
        tin, oin = ar.input("tokens", torch.cat(parts)), ar.input("offsets", off)
        out = ar.output("out", torch.float32, (len(parts), D))
        st = lib.anyloc_pool_tokens(P(tin), P(oin), len(parts), -1, D, ops.POOL_MODES[mode], 3.0, P(out), S())
        _finish("rows", ar, st, lib, {"out": want}, what=("pool ragged", mode, [len(p) for p in parts]))


# ================================================== splits and images ====

SPLIT_X3 = [(1, 5), (77, 48), (130, 100), (333, 200)]        # odd K16 (1, 3, 7, 13), K % 16 != 0, rows % 128 != 0
SPLIT_H2 = [(33, 16), (77, 48), (130, 112), (300, 4096)]


@covers("anyloc_split_x3")
@pytest.mark.parametrize("pad", [0, 4], ids=["ldx=K", "ldx=K+4"])
@pytest.mark.parametrize("rows,K", SPLIT_X3)
def test_split_x3(lib, rows, K, pad):
    """the whole anyloc_x3_bytes extent is written, the planes are the exact split of tests/test_gpu_x6.py::test_split_is_exact
    (its generator, its assertions), and the padded columns hold what anyloc_gemm_nt_x6 needs: that GEMM on the guarded
    image gives the bits of the GEMM on the ordinary one"""
    import test_gpu_x6 as X6
    from anyloc_amd import ops
    g = _gen(1)
    x = torch.randn(rows, K, generator=g, device=DEV) * torch.exp(4 * torch.randn(rows, 1, generator=g, device=DEV))
    x[0, 0] = 0.0
    x[-1, -1] = 1.0 + 2.0 ** -23
    want = ops.split_x3(x)
    nbytes = lib.anyloc_x3_bytes(rows, K)
    assert nbytes == want.numel() and nbytes % 2 == 0
    ar = _arena(6 * 16 * ((K + 15) // 16), 8 << 20)
    xin = ar.input("x", x, strides=(K + pad, 1))
    img = ar.output("x3", torch.int16, (nbytes // 2,))
    st = lib.anyloc_split_x3(P(xin), K + pad, rows, K, P(img), S())
    _finish("splits", ar, st, lib, {"x3": want.view(torch.int16)}, what=("split_x3", rows, K, pad))
    p = X6.planes_from_image(img.view(torch.uint8), rows, K)
    assert p.shape[2] % 16 == 0
    back = (p[0].double() + p[1].double() + p[2].double())[:, :K]
    assert torch.equal(back, x.double())
    assert float(p[:, :, K:].abs().max() if p.shape[2] > K else 0.0) == 0.0
    assert float((p[1].abs() > p[0].abs() * 2.0 ** -7 + 1e-38).float().max()) == 0.0
    assert torch.equal(p[0][:, :K], x.to(torch.bfloat16).float())
    w = torch.randn(17, K, generator=g, device=DEV)
    w3 = ops.split_x3(w)
    assert torch.equal(ops.gemm_nt_x6(img.view(torch.uint8), w3, rows, 17, K), ops.gemm_nt_x6(want, w3, rows, 17, K))
    assert torch.equal(ops.gemm_nt_x6(w3, img.view(torch.uint8), 17, rows, K), ops.gemm_nt_x6(w3, want, 17, rows, K))


@covers("anyloc_split_h2")
@pytest.mark.parametrize("pad", [0, 4], ids=["ldx=K", "ldx=K+4"])
@pytest.mark.parametrize("rows,K", SPLIT_H2)
def test_split_h2(lib, rows, K, pad):
    """image of anyloc_h2_bytes and inv_scale[rows], both guarded; generator and assertions of
    tests/test_gpu_x6.py::test_split_h2_row_scaling_and_precision"""
    import test_gpu_x6 as X6
    from anyloc_amd import ops
    g = _gen(2)
    x = torch.randn(rows, K, generator=g, device=DEV) * torch.exp(3 * torch.randn(rows, 1, generator=g, device=DEV))
    x[:, ::7] *= 40.0
    x[5] = 0.0
    want_img, want_inv = ops.split_h2(x)
    nbytes = lib.anyloc_h2_bytes(rows, K)
    assert nbytes == want_img.numel()
    ar = _arena(4 * K, 16 << 20)
    xin = ar.input("x", x, strides=(K + pad, 1))
    img, inv = ar.output("h2", torch.int16, (nbytes // 2,)), ar.output("inv", torch.float32, (rows,))
    st = lib.anyloc_split_h2(P(xin), K + pad, rows, K, P(img), P(inv), S())
    _finish("splits", ar, st, lib, {"h2": want_img.view(torch.int16), "inv": want_inv}, what=("split_h2", rows, K, pad))
    p = X6.h2_planes_from_image(img.view(torch.uint8), rows, K)
    amax = x.abs().amax(dim=1)
    scaled = amax / inv
    ok = amax > 0
    assert bool(((scaled[ok] >= 2.0 ** 14) & (scaled[ok] < 2.0 ** 15)).all())
    assert bool((torch.log2(inv) == torch.log2(inv).round()).all())
    assert float(p.abs().max()) < 65504.0
    back = (p[0].double() + p[1].double()) * inv.double()[:, None]
    err = (back - x.double()).abs().amax(dim=1)
    assert float((err / amax.clamp_min(1e-30)).max()) < 2.0 ** -22
    assert float(back[5].abs().max()) == 0.0


# =============================================================== GEMMs ====

def _ldcs(N):
    return [N, N + 4, N + 1]


def _gemm_verdict(family, ar, st, lib, C_view, want, what):
    """ldc = N + 1 may be refused: then ANYLOC_ERR_INVALID_ARG comes before any launch -- nothing in the arena moved.
    -> True when the call ran."""
    if st == ERR_INVALID_ARG and C_view.stride(0) % 4 != 0:
        torch.cuda.synchronize()
        assert ar.check() == [] and bool(torch.isnan(C_view).all()), (what, "refused, but something was written")
        print(f"GUARD {what}: refused with ANYLOC_ERR_INVALID_ARG ({lib.anyloc_last_error().decode()})")
        COUNTS[family] = COUNTS.get(family, 0) + 1
        return False
    _finish(family, ar, st, lib, {"C": want}, what=what)
    return True


@covers("anyloc_gemm_nt")
@pytest.mark.parametrize("M,N,K", [(64, 17, 40), (129, 384, 588), (300, 256, 64)])
def test_gemm_nt_strided(lib, M, N, K):
    """lda = ldw = K + 4 and ldc in {N, N + 4, N + 1}; float64 bound of tests/test_gpu_kernels.py::test_gemm_nt"""
    from anyloc_amd import ops
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    a, w, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    ref = a.double() @ w.double().T + bias.double()
    bound = 1.5e-6 * (a.abs().double() @ w.abs().double().T) + 1e-6
    for with_bias, ldc in itertools.product((True, False), _ldcs(N)):
        want = ops.gemm_nt(a.to(DEV), w.to(DEV), bias.to(DEV) if with_bias else None)
        ar = Arena(DEV, 8 << 20, guard=_guard_for(ldc))
        ain, win = ar.input("A", a, strides=(K + 4, 1)), ar.input("W", w, strides=(K + 4, 1))
        bin_ = ar.input("bias", bias) if with_bias else None
        out = ar.output("C", torch.float32, (M, N), (ldc, 1))
        st = lib.anyloc_gemm_nt(P(ain), K + 4, P(win), K + 4, P(bin_), P(out), ldc, M, N, K, S())
        if _gemm_verdict("gemm", ar, st, lib, out, want, ("gemm_nt", M, N, K, ldc, with_bias)):
            r = ref if with_bias else ref - bias.double()
            assert bool(((out.cpu().double() - r).abs() <= bound).all())


def _x6_operands(M, N, K):
    g = _gen(M + N + K)
    a = torch.randn(M, K, generator=g, device=DEV) * (0.25 + torch.rand(M, 1, generator=g, device=DEV))
    w = torch.randn(N, K, generator=g, device=DEV) * 0.05
    bias = torch.randn(N, generator=g, device=DEV)
    return a, w, bias


@covers("anyloc_gemm_nt_x6")
@pytest.mark.parametrize("M,N,K", [(130, 515, 100), (300, 200, 48)])
def test_gemm_nt_x6_strided(lib, M, N, K):
    """with and without bias, ldc in {N, N + 4, N + 1}; error measure and bounds of
    tests/test_gpu_x6.py::test_gemm_x6_as_accurate_as_fp32"""
    from anyloc_amd import ops
    a, w, bias = _x6_operands(M, N, K)
    a3, w3 = ops.split_x3(a), ops.split_x3(w)
    for with_bias, ldc in itertools.product((True, False), _ldcs(N)):
        b = bias if with_bias else None
        want = ops.gemm_nt_x6(a3, w3, M, N, K, b)
        ar = Arena(DEV, 8 << 20, guard=_guard_for(ldc))
        ain, win = ar.input("a3", a3), ar.input("w3", w3)
        bin_ = ar.input("bias", bias) if with_bias else None
        out = ar.output("C", torch.float32, (M, N), (ldc, 1))
        st = lib.anyloc_gemm_nt_x6(P(ain), P(win), P(bin_), P(out), ldc, M, N, K, S())
        if _gemm_verdict("gemm", ar, st, lib, out, want, ("gemm_nt_x6", M, N, K, ldc, with_bias)):
            ref = a.double() @ w.double().t() + (bias.double() if with_bias else 0.0)
            mag = a.double().abs() @ w.double().abs().t() + (bias.double().abs() if with_bias else 0.0)
            err = float(((out.double() - ref).abs() / mag).max())
            assert err < 6e-7, err
            if K % 4 == 0:
                e32 = float(((ops.gemm_nt(a, w, b).double() - ref).abs() / mag).max())
                assert err < 1.5 * e32 + 1e-7, (err, e32)


def _h3_operands(M, N, K):
    a, w, bias = _x6_operands(M, N, K)
    a[:, ::53] *= 30.0
    return a, w, bias


def _h3_guarded(lib, M, N, K, ldcs, biases, what, accuracy=True):
    from anyloc_amd import ops
    a, w, bias = _h3_operands(M, N, K)
    a2, w2 = ops.split_h2(a), ops.split_h2(w)
    cap = (M * (N + 4) * 4) + (M + N) * K * 4 + (16 << 20)
    for with_bias, ldc in itertools.product(biases, ldcs):
        b = bias if with_bias else None
        want = ops.gemm_nt_h3(a2, w2, M, N, K, b)
        ar = Arena(DEV, cap + 8 * _guard_for(ldc), guard=_guard_for(ldc))
        ain, ainv = ar.input("a2", a2[0]), ar.input("a_inv", a2[1])
        win, winv = ar.input("w2", w2[0]), ar.input("w_inv", w2[1])
        bin_ = ar.input("bias", bias) if with_bias else None
        out = ar.output("C", torch.float32, (M, N), (ldc, 1))
        st = lib.anyloc_gemm_nt_h3(P(ain), P(ainv), P(win), P(winv), P(bin_), P(out), ldc, M, N, K, S())
        if _gemm_verdict("gemm", ar, st, lib, out, want, what + (M, N, K, ldc, with_bias)) and accuracy:
            ref = a.double() @ w.double().t() + (bias.double() if with_bias else 0.0)
            mag = a.double().abs() @ w.double().abs().t() + (bias.double().abs() if with_bias else 0.0)
            err = float(((out.double() - ref).abs() / mag).max())
            e32 = float(((ops.gemm_nt(a, w, b).double() - ref).abs() / mag).max())
            assert err < 1.5 * e32 + 1e-7, (err, e32)


@covers("anyloc_gemm_nt_h3")
@pytest.mark.parametrize("M,N,K", [(130, 515, 112), (300, 200, 48)])
def test_gemm_nt_h3_strided(lib, M, N, K):
    """with and without bias, ldc in {N, N + 4, N + 1}; error measure and bound of
    tests/test_gpu_x6.py::test_gemm_h3_as_accurate_as_fp32"""
    _h3_guarded(lib, M, N, K, _ldcs(N), (True, False), ("gemm_nt_h3",))


H3_WIDTHS = ((200, 48), (515, 112), (1536, 384), (4608, 384))          # (N, K) the plain-store plans are enumerated over
H3_MAX_M = 2051


def h3_tile_shapes(lib):
    """-> {(route, tile, tile_rows, tile_cols): (M, N, K)}: every distinct (route, tile) the plan function gives a
    plain-store GEMM (anyloc_h3_plan_describe(M, N, K, "store", 0, 0)) at M <= 2051 over H3_WIDTHS, each with the smallest
    M * N that reaches it"""
    seen = {}
    for (N, K), M in itertools.product(H3_WIDTHS, range(1, H3_MAX_M + 1)):
        d = PE.describe(lib, M, N, K, "store", 0, 0)
        key = (d["route"], d["tile"], d["tile_rows"], d["tile_cols"])
        if key not in seen or M * N < seen[key][0] * seen[key][1]:
            seen[key] = (M, N, K)
    return seen


@covers("anyloc_gemm_nt_h3")
def test_gemm_nt_h3_every_tile_shape(lib):
    shapes = h3_tile_shapes(lib)
    assert len(shapes) >= 2, shapes
    for key, (M, N, K) in sorted(shapes.items()):
        print(f"GUARD gemm_nt_h3 plan (route, tile, rows, cols) {key}: M {M} N {N} K {K}")
        _h3_guarded(lib, M, N, K, (N, N + 4), (True,), ("gemm_nt_h3 tile", key))


def h3m_smallest(lib):
    """the smallest square-ish shape option h3_mfma16 = 1 sends to gemm_h3m_kernel at K = 16 (host-only plan calls)"""
    for tiles in range(1, 40):
        M = N = 256 * (tiles - 1) + 1
        if PE.describe(lib, M, N, 16, "store", 0, 0)["mfma16"]:
            return M, N
    raise AssertionError("no shape up to 39 x 39 tiles takes the 16 x 16 x 32 MFMA kernel")


@covers("anyloc_gemm_nt_h3")
def test_gemm_nt_h3_mfma16_kernel(lib):
    from anyloc_amd import ops
    ops.set_option("h3_mfma16", 1)
    M, N = h3m_smallest(lib)
    assert not PE.describe(lib, M - 256, N, 16, "store", 0, 0)["mfma16"]
    print(f"GUARD gemm_nt_h3 mfma16: M {M} N {N} K 16")
    _h3_guarded(lib, M, N, 16, (N, N + 4), (True,), ("gemm_nt_h3 mfma16",))


@covers("anyloc_gemm_nt_f64", "anyloc_pca_gram_f64", "anyloc_pca_axes_f64")
def test_f64_products(lib):
    """n = 37 samples (odd: single fetches), f = 50 features (even: pair fetches), k = 5; both sides, both storage orders"""
    from anyloc_amd import ops
    n, f, k = 37, 50, 5
    g = _gen(9)
    X = torch.randn(n, f, generator=g, device=DEV)
    mean = X.double().mean(dim=0)
    X64 = X.double()
    U = torch.randn(n, k, generator=g, device=DEV, dtype=torch.float64)
    # anyloc_gemm_nt_f64: operands as stored and as .t() views of the other storage order, plain and symmetric
    Xt = X64.t().contiguous()                                      # [f, n] storage: X64 again through strides (1, n)
    for a_store, a_view, b_store, b_view, sym in (
            (X64, lambda t: t, X64[:k].contiguous(), lambda t: t, False),          # [37, 50] x [5, 50]: pairs along c
            (Xt, lambda t: t.t(), X64[:k].contiguous(), lambda t: t, False),       # A with rs = 1 over 37 rows: singles
            (Xt, lambda t: t, Xt[:k].contiguous(), lambda t: t, False),            # contraction over n = 37 (odd)
            (X64, lambda t: t.t(), X64, lambda t: t.t(), True),                    # scatter X^T X, symmetric, rs = 1 even
            (X64, lambda t: t, X64, lambda t: t, True)):                           # Gram X X^T, symmetric
        A = a_view(a_store)
        B = A if sym else b_view(b_store)
        want = ops.gemm_nt_f64(A, B, symmetric=sym)
        ar = _arena(8 * B.shape[0], 8 << 20)
        ain = a_view(ar.input("A", a_store))
        bin_ = ain if sym else b_view(ar.input("B", b_store))
        (M, K), Nn = A.shape, B.shape[0]
        out = ar.output("C", torch.float64, (M, Nn))
        st = lib.anyloc_gemm_nt_f64(P(ain), ain.stride(0), ain.stride(1), P(bin_), bin_.stride(0), bin_.stride(1), M, Nn, K,
                                    int(sym), P(out), S())
        _finish("f64", ar, st, lib, {"C": want}, what=("gemm_nt_f64", tuple(A.shape), A.stride(), sym))
    for side in (0, 1):
        want = ops.pca_gram_f64(X, mean, side)
        m = n if side == 0 else f
        ar = _arena(8 * m, 8 << 20)
        xin, min_ = ar.input("X", X), ar.input("mean", mean)
        out = ar.output("G", torch.float64, (m, m))
        st = lib.anyloc_pca_gram_f64(P(xin), n, f, P(min_), side, P(out), S())
        _finish("f64", ar, st, lib, {"G": want}, what=("pca_gram_f64", side))
    for store in (U, U.t().contiguous()):                          # [n, k] row-major; [k, n] = the column-major order
        vec = store if store.shape == (n, k) else store.t()
        want = ops.pca_axes_f64(vec, k, X, mean)
        ar = _arena(8 * f, 8 << 20)
        vin = ar.input("vec", store)
        vin = vin if store.shape == (n, k) else vin.t()
        xin, min_ = ar.input("X", X), ar.input("mean", mean)
        out = ar.output("axes", torch.float64, (k, f))
        st = lib.anyloc_pca_axes_f64(P(vin), vin.stride(0), vin.stride(1), k, P(xin), n, f, P(min_), P(out), S())
        _finish("f64", ar, st, lib, {"axes": want}, what=("pca_axes_f64", vin.stride()))


# =========================================================== attention ====

ATTN_SHAPES = [(3, 33, 2), (1, 128, 1), (1, 20, 3), (2, 257, 6)]
RAGGED_TOKENS = (20, 257, 33)


def _qkv(B, T, heads):
    D = heads * 64
    qkv = torch.randn(B, T, 3 * D, generator=_gen(B * T + heads), device=DEV) * 1.5
    qkv[0, 3, :D] *= 6.0
    qkv[0, T - 2, D:2 * D] *= 6.0
    return qkv


@covers("anyloc_attention")
@pytest.mark.parametrize("x6", [0, 1], ids=["fp32-mfma", "split-bf16"])
@pytest.mark.parametrize("B,T,heads", ATTN_SHAPES)
def test_attention(lib, B, T, heads, x6):
    from anyloc_amd import ops
    ops.set_option("attn_x6", x6)
    D = heads * 64
    qkv = _qkv(B, T, heads)
    want = ops.attention(qkv, heads)
    ar = _arena(4 * D, 16 << 20)
    qin, out = ar.input("qkv", qkv), ar.output("out", torch.float32, (B * T, D))
    st = lib.anyloc_attention(P(qin), P(out), B, T, D, heads, S())
    _finish("attention", ar, st, lib, {"out": want}, what=("attention", B, T, heads, x6))


@covers("anyloc_attention_h3")
@pytest.mark.parametrize("qg,ks", [(1, 1), (2, 1), (1, 2)], ids=["4x32q", "2x64q", "2x32q-x-2keys"])
@pytest.mark.parametrize("B,T,heads", ATTN_SHAPES)
def test_attention_h3(lib, B, T, heads, qg, ks):
    from anyloc_amd import ops
    ops.set_option("attn_h3_qg", qg)
    ops.set_option("attn_h3_ks", ks)
    D = heads * 64
    qkv = _qkv(B, T, heads)
    want_img, want_inv = ops.attention_h3(qkv, heads)
    nbytes, ws_bytes = lib.anyloc_h2_bytes(B * T, D), lib.anyloc_attention_h3_workspace_bytes(B, T, heads)
    for scale in (1, 2):
        ar = _arena(4 * D, 16 << 20)
        qin = ar.input("qkv", qkv)
        img, inv = ar.output("img", torch.int16, (nbytes // 2,)), ar.output("inv", torch.float32, (B * T,))
        ws = ar.workspace(ws_bytes * scale)
        st = lib.anyloc_attention_h3(P(qin), P(img), P(inv), B, T, D, heads, P(ws), ws.numel(), S())
        _finish("attention", ar, st, lib, {"img": want_img.view(torch.int16), "inv": want_inv},
                what=("attention_h3", B, T, heads, qg, ks, scale))


@covers("anyloc_attention_ragged", "anyloc_attention_h3_ragged")
@pytest.mark.parametrize("xcd", [0, 1])
def test_attention_ragged(lib, xcd):
    """token counts (20, 257, 33), 2 heads: the fp32-MFMA and split-bf16 kernels and the two-term fp16 one, the latter under
    both workgroup orders; the ordinary call is the same entry on plain torch.empty tensors"""
    from anyloc_amd import ops
    ops.set_option("attn_h3_ragged_xcd", xcd)
    heads, D, n_img = 2, 128, len(RAGGED_TOKENS)
    total = sum(RAGGED_TOKENS)
    qkv = _qkv(1, total, heads)[0]
    tokens = (C.c_int32 * n_img)(*RAGGED_TOKENS)
    off = torch.tensor([0] + list(itertools.accumulate(RAGGED_TOKENS)), dtype=torch.int64, device=DEV)
    for x6 in (0, 1):
        ops.set_option("attn_x6", x6)
        want = torch.empty(total, D, device=DEV)
        assert lib.anyloc_attention_ragged(P(qkv), P(want), n_img, tokens, P(off), D, heads, S()) == 0
        ar = _arena(4 * D, 16 << 20)
        qin, oin = ar.input("qkv", qkv), ar.input("tok_off", off)
        out = ar.output("out", torch.float32, (total, D))
        st = lib.anyloc_attention_ragged(P(qin), P(out), n_img, tokens, P(oin), D, heads, S())
        _finish("attention", ar, st, lib, {"out": want}, what=("attention_ragged", x6, xcd))
    nbytes, ws_bytes = lib.anyloc_h2_bytes(total, D), lib.anyloc_attention_h3_workspace_bytes(1, total, heads)
    want_img = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    want_inv = torch.empty(total, device=DEV)
    plain_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    assert lib.anyloc_attention_h3_ragged(P(qkv), P(want_img), P(want_inv), n_img, tokens, P(off), D, heads, P(plain_ws),
                                          ws_bytes, S()) == 0
    for scale in (1, 2):
        ar = _arena(4 * D, 16 << 20)
        qin, oin = ar.input("qkv", qkv), ar.input("tok_off", off)
        img, inv = ar.output("img", torch.int16, (nbytes // 2,)), ar.output("inv", torch.float32, (total,))
        ws = ar.workspace(ws_bytes * scale)
        st = lib.anyloc_attention_h3_ragged(P(qin), P(img), P(inv), n_img, tokens, P(oin), D, heads, P(ws), ws.numel(), S())
        _finish("attention", ar, st, lib, {"img": want_img.view(torch.int16), "inv": want_inv},
                what=("attention_h3_ragged", xcd, scale))


# ==================================================== VLAD and k-means ====

VLAD_HARD = [(8, 384, 256), (32, 1536, 529), (5, 64, 77), (200, 256, 700)]              # (K, D, N)
VLAD_OPTIONS = [{}, {"vlad_parts": 1}, {"vlad_parts": 3}, {"vlad_parts": 8}, {"vlad_two_pass": 1}]


def _tokens_centers(K, D, N, seed):
    g = _gen(seed)
    tokens = torch.randn(N, D, generator=g, device=DEV)
    centers = 0.8 * tokens[torch.randperm(N, generator=g, device=DEV)[:K]] + 0.05 * torch.randn(K, D, generator=g, device=DEV)
    return tokens, centers


@covers("anyloc_vlad_hard")
@pytest.mark.parametrize("options", VLAD_OPTIONS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "defaults")
@pytest.mark.parametrize("K,D,N", VLAD_HARD)
def test_vlad_hard(lib, K, D, N, options):
    """three images, the middle one empty; descriptors [3, K * D] and labels [N] guarded, the workspace of exactly
    anyloc_vlad_workspace_bytes_parts under the options of the run"""
    from anyloc_amd import ops
    for name, value in options.items():
        ops.set_option(name, value)
    tokens, centers = _tokens_centers(K, D, N, K + D + N)
    cut = N // 3
    parts = [tokens[:cut], tokens[cut:cut], tokens[cut:]]
    want, want_labels = ops.vlad(parts, centers, return_labels=True)
    off = torch.tensor([0, cut, cut, N], dtype=torch.int64)
    flags = ops.VLAD_NORM_DESCS | ops.VLAD_INTRA_NORM
    ws_bytes = lib.anyloc_vlad_workspace_bytes_parts(N, 3, D, K, 0)
    for scale in (1, 2):
        ar = _arena(4 * K * D, 2 * ws_bytes + (32 << 20))
        tin, oin, cin = ar.input("tokens", tokens), ar.input("offsets", off), ar.input("centers", centers)
        out, labels = ar.output("out", torch.float32, (3, K * D)), ar.output("labels", torch.int64, (N,))
        ws = ar.workspace(ws_bytes * scale)
        st = lib.anyloc_vlad_hard(P(tin), P(oin), 3, N, D, P(cin), K, flags, P(out), P(labels), P(ws), ws.numel(), S())
        _finish("vlad", ar, st, lib, {"out": want, "labels": want_labels}, what=("vlad_hard", K, D, N, options, scale))


@covers("anyloc_vlad_soft", "anyloc_vlad_soft_weights", "anyloc_vlad_residuals", "anyloc_vlad_assigned")
@pytest.mark.parametrize("K,D,N", [(8, 384, 256), (33, 64, 77)])
def test_vlad_soft_family(lib, K, D, N):
    from anyloc_amd import ops
    tokens, centers = _tokens_centers(K, D, N, K * D + N)
    cut = N // 3
    off = torch.tensor([0, cut, cut, N], dtype=torch.int64)
    flags = ops.VLAD_NORM_DESCS | ops.VLAD_INTRA_NORM

    def arena(ws_bytes):
        ar = _arena(4 * K * D, 2 * ws_bytes + (32 << 20))
        return ar, ar.input("tokens", tokens), ar.input("centers", centers)

    want = ops.vlad([tokens[:cut], tokens[cut:cut], tokens[cut:]], centers, mode="soft", soft_temp=1.5)
    ws_bytes = lib.anyloc_vlad_workspace_bytes_parts(N, 3, D, K, 0)
    for scale in (1, 2):
        ar, tin, cin = arena(ws_bytes)
        oin, out = ar.input("offsets", off), ar.output("out", torch.float32, (3, K * D))
        ws = ar.workspace(ws_bytes * scale)
        st = lib.anyloc_vlad_soft(P(tin), P(oin), 3, N, D, P(cin), K, 1.5, flags, P(out), P(ws), ws.numel(), S())
        _finish("vlad", ar, st, lib, {"out": want}, what=("vlad_soft", K, D, N, scale))

    one_bytes = lib.anyloc_vlad_workspace_bytes(N, 1, D, K)
    weights = ops.vlad_soft_weights(tokens, centers, 1.5)
    for scale in (1, 2):
        ar, tin, cin = arena(one_bytes)
        out, ws = ar.output("weights", torch.float32, (N, K)), ar.workspace(one_bytes * scale)
        st = lib.anyloc_vlad_soft_weights(P(tin), N, D, P(cin), K, 1.5, P(out), P(ws), ws.numel(), S())
        _finish("vlad", ar, st, lib, {"weights": weights}, what=("vlad_soft_weights", K, D, N, scale))

    want = ops.vlad_residuals(tokens, centers)
    ar, tin, cin = arena(0)
    out = ar.output("residuals", torch.float32, (N, K, D))
    st = lib.anyloc_vlad_residuals(P(tin), N, D, P(cin), K, ops.VLAD_NORM_DESCS, P(out), S())
    _finish("vlad", ar, st, lib, {"residuals": want}, what=("vlad_residuals", K, D, N))

    labels = torch.randint(0, K, (N,), generator=_gen(N), device=DEV)
    for given in ("labels", "soft"):
        want = ops.vlad_assigned(tokens, centers, labels=labels) if given == "labels" else \
            ops.vlad_assigned(tokens, centers, soft=weights)
        for scale in (1, 2):
            ar, tin, cin = arena(one_bytes)
            lin = ar.input("labels", labels) if given == "labels" else None
            sin = ar.input("soft", weights) if given == "soft" else None
            out, ws = ar.output("out", torch.float32, (K * D,)), ar.workspace(one_bytes * scale)
            st = lib.anyloc_vlad_assigned(P(tin), N, D, P(cin), K, P(lin), P(sin), flags, P(out), P(ws), ws.numel(), S())
            _finish("vlad", ar, st, lib, {"out": want}, what=("vlad_assigned", given, K, D, N, scale))


@covers("anyloc_kmeans_step")
@pytest.mark.parametrize("mode", ["cosine", "euclidean"])
@pytest.mark.parametrize("n,D,K", [(5003, 384, 16), (700, 64, 40)], ids=["fused", "two-pass"])
def test_kmeans_step(lib, n, D, K, mode):
    from anyloc_amd import ops
    x, centers = _tokens_centers(K, D, n, n + D + K)
    want = ops.kmeans_step(x, centers, mode, want_labels=True)
    ws_bytes = lib.anyloc_kmeans_workspace_bytes(n, D, K)
    for scale in (1, 2):
        ar = _arena(4 * D, 2 * ws_bytes + (32 << 20))
        xin, cin = ar.input("x", x), ar.input("centers", centers)
        sums, counts = ar.output("sums", torch.float32, (K, D)), ar.output("counts", torch.float32, (K,))
        labels, ws = ar.output("labels", torch.int64, (n,)), ar.workspace(ws_bytes * scale)
        st = lib.anyloc_kmeans_step(P(xin), n, D, P(cin), K, 0 if mode == "cosine" else 1, P(sums), P(counts), P(labels),
                                    P(ws), ws.numel(), S())
        _finish("kmeans", ar, st, lib, {"sums": want[0], "counts": want[1], "labels": want[2]},
                what=("kmeans_step", n, D, K, mode, scale))


@covers("anyloc_kmeans_update")
def test_kmeans_update_with_an_empty_cluster(lib):
    from anyloc_amd import ops
    K, D = 16, 384
    g = _gen(6)
    sums, old = torch.randn(K, D, generator=g, device=DEV), torch.randn(K, D, generator=g, device=DEV)
    counts = torch.arange(1, K + 1, device=DEV, dtype=torch.float32)
    counts[7] = 0.0
    sums[7] = 0.0
    want_new, want_err = ops.kmeans_update(sums, counts, old)
    assert float(want_new[7].abs().max()) == 0.0
    ar = _arena(4 * D, 8 << 20)
    sin, cin, oin = ar.input("sums", sums), ar.input("counts", counts), ar.input("old", old)
    new, err = ar.output("new", torch.float32, (K, D)), ar.output("err", torch.float64, (1,))
    st = lib.anyloc_kmeans_update(P(sin), P(cin), P(oin), K, D, P(new), P(err), S())
    _finish("kmeans", ar, st, lib, {"new": want_new, "err": want_err}, what="kmeans_update")


# =========================================================== retrieval ====

TOPK_KS = (1, 10, 129)


def topk_option_sets(lib, nq, ndb, dim):
    """the option sets of tests/test_topk_workspace_cpu.py that change what serves (nq, ndb, dim): one per distinct
    (scoring path, workspace bytes at each k) and, on the few-query path, per value of the two options that choose its
    kernel without moving the carve (topk_fewq_x6: fp32 MFMA / three bf16 planes / two fp16 planes; topk_fewq_qdma: the
    queries split once or per slab) -- host-only calls; the defaults always first"""
    import test_topk_workspace_cpu as TW
    chosen, seen = [], set()
    for options in TW.OPTION_SETS:
        lib.anyloc_reset_options()
        for name, value in options.items():
            assert lib.anyloc_set_option(name.encode(), value) == 0
        path = lib.anyloc_topk_path(nq, ndb, dim)
        key = (path,) + tuple(lib.anyloc_topk_workspace_bytes(nq, ndb, dim, k) for k in TOPK_KS)
        if path == 1:
            key += (options.get("topk_fewq_x6", 2), options.get("topk_fewq_qdma", 1))       # (the defaults of the header)
        if key not in seen:
            seen.add(key)
            chosen.append(options)
    lib.anyloc_reset_options()
    return chosen


def _topk_shapes():
    import test_topk_workspace_cpu as TW
    return [s for s in TW.SHAPES if s[1] > 0]


def _retrieval_data(nq, ndb, dim):
    g = _gen(nq + ndb + dim)
    db = torch.randn(ndb, dim, generator=g, device=DEV)
    qu = db[torch.randperm(ndb, generator=g, device=DEV)[:nq] % ndb] if ndb >= nq else torch.randn(nq, dim, generator=g, device=DEV)
    qu = torch.nn.functional.normalize(qu + 0.3 * torch.randn(nq, dim, generator=g, device=DEV), dim=-1)
    return qu, db


@covers("anyloc_topk")
@pytest.mark.parametrize("nq,ndb,dim", _topk_shapes(), ids=lambda v: str(v))
def test_topk(lib, nq, ndb, dim):
    """dist [nq, k] and idx [nq, k] guarded, the workspace of exactly anyloc_topk_workspace_bytes: every k, both metrics, every
    option set that changes the path of the shape.  Queries and database lie in the arena too (inputs: compared with their
    copies by every check) while they hold at most 16 MiB together; the larger ones, read-only operands of up to 0.5 GB,
    stay ordinary tensors and are compared with their copies after the last call.  idx -1 remains only in the tail of a
    list longer than the database."""
    from anyloc_amd import ops
    qu, db = _retrieval_data(nq, ndb, dim)
    qu0, db0 = qu.clone(), db.clone()
    small = (qu.numel() + db.numel()) * 4 <= (16 << 20)
    for options in topk_option_sets(lib, nq, ndb, dim):
        lib.anyloc_reset_options()
        for name, value in options.items():
            ops.set_option(name, value)
        for k, metric in itertools.product(TOPK_KS, ("ip", "l2")):
            want_d, want_i = ops.topk(qu, db, k, metric, normalize_db=True)
            tail = torch.arange(k, device=DEV)[None, :].expand(nq, k) >= ndb
            assert torch.equal(want_i == -1, tail), (nq, ndb, dim, k, metric, options)
            ws_bytes = lib.anyloc_topk_workspace_bytes(nq, ndb, dim, k)
            for scale in (1, 2):
                ar = _arena(8 * k, 2 * ws_bytes + (8 << 20) + (32 << 20 if small else 0))
                qin, din = (ar.input("queries", qu), ar.input("db", db)) if small else (qu, db)
                dist, idx = ar.output("dist", torch.float32, (nq, k)), ar.output("idx", torch.int64, (nq, k))
                ws = ar.workspace(ws_bytes * scale)
                st = lib.anyloc_topk(P(qin), nq, P(din), ndb, dim, k, 0 if metric == "ip" else 1, ops.TOPK_NORMALIZE_DB, 0,
                                     P(dist), P(idx), P(ws), ws.numel(), S())
                _finish("topk", ar, st, lib, {"dist": want_d, "idx": want_i}, pad={"idx": -1},
                        what=("topk", nq, ndb, dim, k, metric, options, scale))
    assert torch.equal(qu, qu0) and torch.equal(db, db0)


def _index_live_parts(lib, index, plain, ndb, dim):
    """The live parts of a guarded index (csrc/topk.hip, index_view: per panel the two-plane image of the panel's own row
    count at a 256-byte aligned slot sized for a whole panel, then 2^-e, sums of squares and residual norms as three float
    arrays of ndb entries at multiples of 64, then 256 bytes of slack) are all written and have the bits of the ordinary build; the padding between
    them is not compared (the ordinary buffer is a torch.empty)."""
    panel = lib.anyloc_topk_index_panel(dim)
    n_panels = (ndb + panel - 1) // panel
    slot = (lib.anyloc_h2_bytes(panel, dim) + 255) // 256 * 256
    pad64 = (ndb + 63) // 64 * 64
    assert n_panels * slot + 3 * pad64 * 4 + 256 == index.numel() == plain.numel()
    for p in range(n_panels):
        rows = min(panel, ndb - p * panel)
        lo, hi = p * slot, p * slot + lib.anyloc_h2_bytes(rows, dim)
        got = index[lo:hi].view(torch.int16)
        assert torch.equal(got, plain[lo:hi].view(torch.int16)), ("index image", p)
        assert not bool((got == -1).any()), ("index image", p, "an fp16 element left unwritten")      # 0xFFFF is a NaN
    for j, what in enumerate(("2^-e", "sums of squares", "residual norms")):
        lo = n_panels * slot + j * pad64 * 4
        got = index[lo:lo + 4 * ndb].view(torch.int32)
        assert torch.equal(got, plain[lo:lo + 4 * ndb].view(torch.int32)), what
        assert not bool((got == -1).any()), (what, "an entry left unwritten")


@covers("anyloc_topk_index_build", "anyloc_topk_index_build_range", "anyloc_topk_search_index",
        "anyloc_topk_search_index_rows")
@pytest.mark.parametrize("screen", [0, 1])
def test_topk_index(lib, screen):
    """(70, 8492, 256): the index built into a buffer of exactly anyloc_topk_index_bytes, at once and in two ranges (one
    whole panel, then the rest) -- both leave the same bytes --, then both searches on the guarded index with the exact
    anyloc_topk_index_workspace_bytes (which holds the screened search's read-back flag and candidate buffers)"""
    from anyloc_amd import ops
    ops.set_option("topk_screen", screen)
    nq, ndb, dim, k = 70, 8492, 256, 10
    qu, db = _retrieval_data(nq, ndb, dim)
    nbytes = lib.anyloc_topk_index_bytes(ndb, dim)
    panel = lib.anyloc_topk_index_panel(dim)
    assert nbytes > 0 and 0 < panel < ndb
    plain_index = ops.topk_index_build(db)
    cap = 3 * nbytes + 16 * lib.anyloc_topk_index_workspace_bytes(nq, ndb, dim, k) + (64 << 20)

    ar = Arena(DEV, cap)
    din, qin = ar.input("db", db), ar.input("queries", qu)
    index = ar.output("index", torch.uint8, (nbytes,))
    st = lib.anyloc_topk_index_build(P(din), ndb, dim, P(index), nbytes, S())
    _finish("index", ar, st, lib, {}, what="topk_index_build")
    _index_live_parts(lib, index, plain_index, ndb, dim)
    pieces = ar.output("index_by_ranges", torch.uint8, (nbytes,))
    for row0, n in ((panel, ndb - panel), (0, panel)):
        rows = db[row0:row0 + n].contiguous()
        st = lib.anyloc_topk_index_build_range(P(rows), row0, n, ndb, dim, P(pieces), nbytes, S())
        _finish("index", ar, st, lib, {}, what=("topk_index_build_range", row0, n))
    assert torch.equal(index, pieces)
    _index_live_parts(lib, pieces, plain_index, ndb, dim)

    ws_bytes = lib.anyloc_topk_index_workspace_bytes(nq, ndb, dim, k)
    for metric, with_rows, scale in itertools.product(("ip", "l2"), (False, True), (1, 2)):
        m = 0 if metric == "ip" else 1
        if with_rows:
            want_d, want_i = ops.topk_indexed(qu, plain_index, ndb, k, metric, normalize_db=True, db=db)
        else:
            want_d = torch.empty(nq, k, device=DEV)
            want_i = torch.empty(nq, k, dtype=torch.int64, device=DEV)
            plain_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
            assert lib.anyloc_topk_search_index(P(qu), nq, P(plain_index), ndb, dim, k, m, ops.TOPK_NORMALIZE_DB, 0, P(want_d),
                                                P(want_i), P(plain_ws), ws_bytes, S()) == 0
        dist, idx = ar.output(f"dist{metric}{with_rows}{scale}", torch.float32, (nq, k)), \
            ar.output(f"idx{metric}{with_rows}{scale}", torch.int64, (nq, k))
        ws = ar.workspace(ws_bytes * scale, name=f"ws{metric}{with_rows}{scale}")
        if with_rows:
            st = lib.anyloc_topk_search_index_rows(P(qin), nq, P(din), P(index), ndb, dim, k, m, ops.TOPK_NORMALIZE_DB, 0,
                                                   P(dist), P(idx), P(ws), ws.numel(), S())
        else:
            st = lib.anyloc_topk_search_index(P(qin), nq, P(index), ndb, dim, k, m, ops.TOPK_NORMALIZE_DB, 0, P(dist), P(idx),
                                              P(ws), ws.numel(), S())
        _finish("index", ar, st, lib, {f"dist{metric}{with_rows}{scale}": want_d, f"idx{metric}{with_rows}{scale}": want_i},
                what=("topk_search_index" + ("_rows" if with_rows else ""), metric, screen, scale))
    # the searches read the index: after all of them it still holds what the build left
    assert torch.equal(index, pieces)


# ================================================================= ViT ====

VIT_MODES = ("f32", "x6", "h3")
_MODELS = {}


def _model(name, mode, depth=2, ffn_check=False):
    from anyloc_amd import synth
    from anyloc_amd.extractor import HipDinoV2
    key = (name, mode, depth, ffn_check)
    if key not in _MODELS:
        sd = synth.synthetic_state_dict(name, 7, depth=depth)
        m = HipDinoV2(name, {k: v.to(DEV) for k, v in sd.items()}, torch.device(DEV), gemm=mode)
        # False: one call per forward and no telemetry; True (the extractor's default): every h3 forward runs with the
        # FFN-bound telemetry on and reads it back
        m.ffn_check = ffn_check
        _MODELS[key] = m
    return _MODELS[key]


def _images(B, hw, seed):
    return torch.randn(B, 3, hw[0], hw[1], generator=_gen(seed + hw[0] + hw[1]), device=DEV)


class _Telemetry:
    """The FFN-bound telemetry of the default two-term fp16 forward, as HipDinoV2._telemetry_call sets it around EVERY such
    forward: the memset over the rows' maxima inside the workspace carve widens, the fc1 / w12 epilogues leave one maximum
    per token row there, and one launch writes the caller's device array -- one figure per executed block (per_image = 0)
    or per (executed block, image).  ``want``: the figures of the same call on plain torch.empty tensors; ``worst``: the
    per-block figures the extractor's own ``ffn_check = True`` call reports (the largest over the images)."""

    def __init__(self, lib, model, per_image, n_blocks, n_img):
        self.lib, self.model, self.per_image = lib, model, per_image
        self.shape = (n_blocks, n_img if per_image else 1)
        self.want = torch.empty(self.shape, device=DEV)
        self.worst = None

    def extractor(self, run):
        """``run()`` (a forward_taps call) with the extractor's own check on: no image may have needed a re-run"""
        self.model.ffn_check = True
        before = self.model.ffn_reruns
        try:
            res = run()
        finally:
            self.model.ffn_check = False
        assert self.model.ffn_reruns == before
        self.worst = torch.from_numpy(np.asarray(self.model.ffn_looseness, dtype=np.float32).copy())
        assert self.worst.shape == (self.shape[0],)
        return res

    def around(self, target, call):
        """``call()`` with ``target`` as the telemetry array of the handle"""
        from anyloc_amd import _lib
        _lib.check(self.lib.anyloc_vit_set_telemetry(self.model._handle, P(target), self.per_image), "anyloc_vit_set_telemetry")
        try:
            return call()
        finally:
            _lib.check(self.lib.anyloc_vit_set_telemetry(self.model._handle, None, 0), "anyloc_vit_set_telemetry")

    def verdict(self, got, ffn_of_last_block):
        """``ffn_of_last_block``: the forward ends at a token tap -- at a q / k / v tap it leaves its last block before the
        FFN, and that block reports the 0 of a block that did not run fused"""
        assert same_bits(got, self.want)
        assert torch.equal(got.cpu().amax(dim=1), self.worst), (got, self.worst)
        fused = got if ffn_of_last_block else got[:-1]
        assert bool((fused > 0).all()) and (ffn_of_last_block or bool((got[-1] == 0).all())), got


def _vit_uniform(lib, model, B, hw, facet="value", use_cls=False, telemetry=None, layer=None):
    """anyloc_vit_forward with the model's handle, as HipDinoV2._forward_uniform calls it: guarded img, out and workspace
    (``telemetry``: per_image of a guarded telemetry array, None = telemetry off)"""
    H, W = hw
    imgs = _images(B, hw, B)
    layer = model.depth - 1 if layer is None else layer
    taps = [(layer, facet)]
    tel = None if telemetry is None else _Telemetry(lib, model, telemetry, layer + 1, B)
    if tel is None:
        want = model.forward_taps(imgs, taps, use_cls=use_cls)
    else:
        want = tel.extractor(lambda: model.forward_taps(imgs, taps, use_cls=use_cls))
    n_taps, layers, facets, flags = model._tap_args(taps, use_cls, True, False)
    pos = model.pos_table(H, W)
    ws_bytes = lib.anyloc_vit_workspace_bytes(model._handle, B, H, W)
    assert ws_bytes > 0
    if tel is not None:
        plain_out, plain_ws = torch.empty_like(want), torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        assert tel.around(tel.want, lambda: lib.anyloc_vit_forward(
            model._handle, P(imgs), B, H, W, P(pos), n_taps, layers, facets, flags, P(plain_out), P(plain_ws), ws_bytes, S())) == 0
        assert same_bits(plain_out, want)
    for scale in (1, 2):
        ar = Arena(DEV, 2 * ws_bytes + imgs.numel() * 4 + want.numel() * 4 + (16 << 20), guard=_guard_for(want.shape[-1]))
        iin, pin = ar.input("img", imgs), ar.input("pos", pos)
        out, ws = ar.output("out", torch.float32, tuple(want.shape)), ar.workspace(ws_bytes * scale)
        refs = {"out": want}

        def call():
            return lib.anyloc_vit_forward(model._handle, P(iin), B, H, W, P(pin), n_taps, layers, facets, flags, P(out), P(ws),
                                          ws.numel(), S())
        if tel is None:
            st = call()
        else:
            figures = ar.output("telemetry", torch.float32, tel.shape)
            refs["telemetry"] = tel.want
            st = tel.around(figures, call)
        _finish("vit", ar, st, lib, refs,
                what=("vit_forward", model.name, model.gemm, B, hw, facet, use_cls, scale, telemetry, layer))
        if tel is not None:
            tel.verdict(figures, facet == "token")


def _vit_ragged(lib, model, sizes, facet="value", use_cls=False, telemetry=None):
    """anyloc_vit_forward_ragged with the model's handle, as HipDinoV2._forward_ragged calls it"""
    from anyloc_amd.extractor import ragged_offsets
    imgs = [_images(1, hw, i)[0] for i, hw in enumerate(sizes)]
    taps = [(model.depth - 1, facet)]
    n_img = len(sizes)
    tel = None if telemetry is None else _Telemetry(lib, model, telemetry, model.depth, n_img)
    if tel is None:
        want, _ = model.forward_taps_ragged(imgs, taps, use_cls=use_cls)
    else:
        want, _ = tel.extractor(lambda: model.forward_taps_ragged(imgs, taps, use_cls=use_cls))
    tok, out_off, pix = ragged_offsets(sizes, use_cls, patch=model.patch, registers=model.n_reg)
    tables = [model.pos_table(*hw) for hw in sizes]
    meta = np.zeros((5, n_img + 1), dtype=np.int64)
    meta[0], meta[1] = tok, pix
    meta[2, :n_img] = np.cumsum([0] + [t.shape[0] for t in tables])[:-1]
    meta[3, :n_img] = [h for h, _ in sizes]
    meta[4, :n_img] = [w for _, w in sizes]
    hw_host = (C.c_int32 * (2 * n_img))(*[v for hw in sizes for v in hw])
    n_taps, layers, facets, flags = model._tap_args(taps, use_cls, True, False)
    ws_bytes = lib.anyloc_vit_workspace_bytes_ragged(model._handle, n_img, hw_host)
    assert ws_bytes > 0
    flat = torch.cat([im.reshape(-1) for im in imgs])
    pos, dev_meta = torch.cat(tables), torch.from_numpy(meta).to(DEV)
    if tel is not None:
        plain_out, plain_ws = torch.empty_like(want), torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        assert tel.around(tel.want, lambda: lib.anyloc_vit_forward_ragged(
            model._handle, P(flat), n_img, hw_host, P(dev_meta), P(pos), n_taps, layers, facets, flags, P(plain_out), P(plain_ws),
            ws_bytes, S())) == 0
        assert same_bits(plain_out, want)
    for scale in (1, 2):
        ar = Arena(DEV, 2 * ws_bytes + flat.numel() * 4 + want.numel() * 4 + (16 << 20), guard=_guard_for(want.shape[-1]))
        iin, pin = ar.input("img", flat), ar.input("pos", pos)
        min_ = ar.input("meta", dev_meta)
        out, ws = ar.output("out", torch.float32, tuple(want.shape)), ar.workspace(ws_bytes * scale)
        refs = {"out": want}

        def call():
            return lib.anyloc_vit_forward_ragged(model._handle, P(iin), n_img, hw_host, P(min_), P(pin), n_taps, layers, facets,
                                                 flags, P(out), P(ws), ws.numel(), S())
        if tel is None:
            st = call()
        else:
            figures = ar.output("telemetry", torch.float32, tel.shape)
            refs["telemetry"] = tel.want
            st = tel.around(figures, call)
        _finish("vit", ar, st, lib, refs, what=("vit_forward_ragged", model.name, model.gemm, sizes, facet, scale, telemetry))
        if tel is not None:
            tel.verdict(figures, facet == "token")


@covers("anyloc_vit_forward")
@pytest.mark.parametrize("mode", VIT_MODES)
@pytest.mark.parametrize("B,hw", [(2, (28, 42)), (1, (224, 308))])
def test_vit_forward(lib, B, hw, mode):
    """synthetic dinov2_vits14 of depth 2 in the three arithmetic modes (option x6_min_rows = 0: the split-bf16 kernels at
    these row counts too)"""
    from anyloc_amd import ops
    ops.set_option("x6_min_rows", 0)
    _vit_uniform(lib, _model("dinov2_vits14", mode), B, hw)


@covers("anyloc_vit_forward_ragged")
@pytest.mark.parametrize("mode", VIT_MODES)
def test_vit_forward_ragged(lib, mode):
    from anyloc_amd import ops
    ops.set_option("x6_min_rows", 0)
    _vit_ragged(lib, _model("dinov2_vits14", mode), [(28, 42), (126, 154)])


@covers("anyloc_vit_set_telemetry", "anyloc_vit_forward", "anyloc_vit_forward_ragged")
@pytest.mark.parametrize("per_image", [1, 0], ids=["per-image", "per-call"])
def test_vit_forward_with_the_ffn_telemetry(lib, per_image):
    """The default two-term fp16 forward as the extractor runs it (``ffn_check``): the telemetry array is a guarded output of
    exactly [executed blocks] or [executed blocks][images] floats, every figure written, the workspace the exact
    anyloc_vit_workspace_bytes(_ragged); tokens and figures have the bits of the extractor's own checked call.  A tap at
    layer 0 of the two blocks: one block executes, so one row of figures is the whole documented extent.  A value tap:
    the forward leaves its last block before the FFN, whose figures are the documented 0."""
    model = _model("dinov2_vits14", "h3")
    _vit_uniform(lib, model, 2, (28, 42), facet="token", telemetry=per_image)
    _vit_uniform(lib, model, 1, (224, 308), facet="token", telemetry=per_image)
    _vit_uniform(lib, model, 2, (28, 42), facet="token", telemetry=per_image, layer=0)
    _vit_uniform(lib, model, 2, (28, 42), facet="value", telemetry=per_image)
    _vit_ragged(lib, model, [(28, 42), (126, 154)], facet="token", telemetry=per_image)
    _vit_ragged(lib, model, [(28, 42), (126, 154)], facet="value", telemetry=per_image)


@covers("anyloc_vit_forward", "anyloc_vit_forward_ragged")
@pytest.mark.parametrize("name,B,hw", [("dinov3_vits16", 2, (48, 80)), ("dinov2_vits14_reg", 2, (210, 238))])
def test_vit_rotary_and_register_models(lib, name, B, hw):
    """one DINOv3 and one register model (two-term fp16, the default arithmetic) at the smallest size of their own tests:
    the token tap with the CLS row, uniform and ragged"""
    model = _model(name, "h3")
    _vit_uniform(lib, model, B, hw, facet="token", use_cls=True)
    small = (model.patch * 1, model.patch * 1)
    _vit_ragged(lib, model, [hw, small], facet="query")


def test_guarded_workspace_serves_the_host_modules_at_256_and_16_byte_alignment(lib, monkeypatch):
    """``guarded_workspace`` under the unmodified call sequences of ops.*, kmeans.py, vlad.py, retrieval.py and
    extractor.py: every workspace they ask for is a fresh 0xFF region of exactly the bytes they asked for, and the
    results keep the bits of the run on the growing per-stream buffer -- with the workspace on a 256-byte boundary (what
    ``torch.empty`` gives) and 16 bytes behind one (the alignment include/anyloc_hip.h asks for: the carve keeps the
    base's alignment and the kernels access 16 bytes at a time)."""
    from _stream_harness import flat
    from anyloc_amd import ops
    tokens, centers = _tokens_centers(8, 384, 256, 77)
    small, small_centers = _tokens_centers(40, 64, 700, 78)
    qu, db = _retrieval_data(70, 8492, 256)
    few, wide = _retrieval_data(5, 300, 4096)
    # (the two-term fp16 model with ffn_check = True, the extractor's default: its forwards run with the telemetry on)
    models = [_model("dinov2_vits14", mode, ffn_check=(mode == "h3")) for mode in VIT_MODES]
    imgs = _images(2, (28, 42), 1)
    ragged = [_images(1, hw, 2)[0] for hw in ((28, 42), (126, 154))]
    index = ops.topk_index_build(db)

    def run():
        ops.set_option("x6_min_rows", 0)
        res = [ops.vlad(tokens.reshape(2, 128, 384), centers), ops.vlad(tokens.reshape(2, 128, 384), centers, mode="soft"),
               ops.kmeans_step(tokens, centers, want_labels=True), ops.kmeans_step(small, small_centers, "euclidean", True),
               ops.topk(qu, db, 10), ops.topk(few, wide, 10, "l2"), ops.attention_h3(_qkv(1, 20, 3), 3),
               ops.vlad_assigned(tokens, centers, labels=torch.arange(256, device=DEV) % 8)]
        with ops.options(vlad_two_pass=1):
            res.append(ops.vlad(tokens.reshape(2, 128, 384), centers))
        with ops.options(topk_h3=1, topk_screen=1):
            res += [ops.topk(qu, db, 10, normalize_db=True), ops.topk_indexed(qu, index, 8492, 10, db=db)]
        for m in models:
            res += [m.forward_taps(imgs, [(1, "value")]), m.forward_taps_ragged(ragged, [(1, "token")])[0]]
        return flat(res)

    want = run()
    for skew in (0, 16):
        ar = Arena(DEV, 512 << 20)
        handed = guarded_workspace(monkeypatch, ar, skew=skew)
        got = run()
        torch.cuda.synchronize()
        assert {tag for tag, _ in handed} == {"vlad", "kmeans", "topk", "vit", "attn_h3"}, handed
        assert ar.check() == [], skew
        assert len(got) == len(want) and all(same_bits(g, w) for g, w in zip(got, want)), skew
        COUNTS[f"host modules, workspace base % 256 == {skew}"] = len(handed)


# ============================================================ coverage ====

# Entry points of _lib.SIGNATURES with neither a device output nor a workspace:
EXEMPT = {
    # library state and diagnostics
    "anyloc_version", "anyloc_last_error",
    # options
    "anyloc_set_option", "anyloc_get_option", "anyloc_reset_options",
    # profiling (host buffers only)
    "anyloc_profile_enable", "anyloc_profile_filter", "anyloc_profile_reset", "anyloc_profile_dump",
    # host-only plan and size calls: no device is touched
    "anyloc_h3_lead_plan_check", "anyloc_h3_plan_describe", "anyloc_gemm_plan_describe", "anyloc_topk_path", "anyloc_topk_index_panel",
    "anyloc_vlad_auto_parts", "anyloc_x3_bytes", "anyloc_h2_bytes", "anyloc_topk_index_bytes",
    # construction and per-handle switches: they store pointers or host state (anyloc_vit_attach_h2 writes memory the
    # library allocated itself)
    "anyloc_vit_create", "anyloc_vit_destroy", "anyloc_vit_attach_x3", "anyloc_vit_attach_h2", "anyloc_vit_set_registers",
    "anyloc_vit_set_rope", "anyloc_vit_set_ln_eps", "anyloc_vit_block_ffn_exact",
}


def test_every_entry_point_with_a_device_output_has_a_guarded_case():
    from anyloc_amd import _lib
    names = [n for n in _lib.SIGNATURES if not n.endswith("_workspace_bytes") and not n.endswith("_workspace_bytes_parts")
             and not n.endswith("_workspace_bytes_ragged")]
    assert EXEMPT <= set(names), EXEMPT - set(names)
    uncovered = [n for n in names if n not in EXEMPT and n not in COVERS]
    assert uncovered == [], uncovered
    assert not (EXEMPT & set(COVERS)), EXEMPT & set(COVERS)
    src = open(__file__).read()
    for n in COVERS:
        assert f"lib.{n}(" in src, n
    # every workspace size function is used by the case of its entry
    for n in _lib.SIGNATURES:
        if "_workspace_bytes" in n:
            assert f"lib.{n}(" in src, n
    print("GUARD cases per family:", dict(sorted(COUNTS.items())), "total", sum(COUNTS.values()))
