"""The far side of every addressing limit (profiles/addressing_audit.md), no GPU needed: a call with the smallest shape
beyond a limit returns ANYLOC_ERR_INVALID_ARG from its argument checks, in front of the first HIP call, and
``anyloc_last_error()`` names the limit.  Small host buffers stand in for the pointers (tests/test_limits_cpu.py).

HARD RULE of this file: no call here may PASS its argument checks -- with made-up pointers it would launch a kernel on a
machine that has a GPU.  The last served shape of every limit runs in tests/test_gpu_addressing.py, or is read here from
the host-only functions (``*_bytes``, ``*_workspace_bytes``, ``anyloc_gemm_plan_describe``).

The limit formulas are restated in tests/_big_cases.py from the header's wording, and that module's case table is held
here to what the GPU module relies on: every case's sample holds the rows on both sides of every boundary it claims,
and the token inputs put no label on a near-tie."""
import ctypes as C
import os

import pytest
import torch

import _big_cases as BC
from anyloc_amd import _lib

ERR_INVALID_ARG = -1
WS = 1 << 40               # workspace bytes claimed (never touched: the argument checks come first)
B31 = 1 << 31


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.fail("libanyloc_hip.so not built (python -m anyloc_amd.build)")
    return _lib.load()


@pytest.fixture(scope="module")
def host():
    """small 16-byte-aligned host buffers for the pointers a call checks; none is read before the argument checks"""
    raw = (C.c_char * 1024)()
    base = (C.addressof(raw) + 15) // 16 * 16
    i32 = (C.c_int32 * 4)()
    return dict(f=base, i=base + 256, f3=C.cast(base, C.POINTER(C.c_float)), i32=i32, keep=(raw, i32))


@pytest.fixture()
def options(lib):
    """options set through lib.anyloc_set_option in a test are gone after it"""
    yield lambda name, value: lib.anyloc_set_option(name.encode(), value)
    assert lib.anyloc_reset_options() == 0


def _refused(lib, status, *words):
    msg = lib.anyloc_last_error().decode()
    assert status == ERR_INVALID_ARG, (status, msg)
    for w in words:
        assert w in msg, (w, msg)


def _clear(lib):
    """leave a message of another call behind, so that a stale one cannot pass for the refusal under test"""
    assert lib.anyloc_set_option(b"no_such_option", 0) == ERR_INVALID_ARG
    assert b"2^31" not in lib.anyloc_last_error() and b"2 GiB" not in lib.anyloc_last_error()


def _plan(lib, M, N, K):
    d = _lib.GemmPlanDesc()
    assert lib.anyloc_gemm_plan_describe(M, N, K, b"store", 0, C.byref(d)) == 0, lib.anyloc_last_error()
    return [(d.part[i].rows, d.part[i].tile_rows, d.part[i].tile_cols) for i in range(d.parts)]


# ------------------------------------------------------------------------------------------------------------ fp32 GEMM
@pytest.mark.parametrize("cfg,M,N,K,tall", [(0, 128, 128, 36, 128), (0, 1000, 128, 64, 64), (0, 128, 16, 64, 128), (1, 256, 128, 64, 256),
                                            (0, 128, 128, 8192, 128), (0, 3, 128, 64, 3), (0, 70000, 128, 64, 128)])
def test_gemm_nt_first_leading_dimension_past_a_tile_s_2gib(lib, host, options, cfg, M, N, K, tall):
    """The plan's tile height decides how far apart two rows of one tile may lie: lda (and ldw) one step of 4 past the last
    value that keeps (min(tile rows, rows) - 1) * ld * 4 + K * 4 below 2^31 is refused, for every tile height a plan picks
    here -- 128 (a K tail, the narrow tile, the chunked summation, the 128-row part of a row split), 64 (the half tile),
    256 (gemm_f32_cfg = 1) -- and for a matrix shorter than its tile."""
    f = host["f"]
    options("gemm_f32_cfg", cfg)
    parts = _plan(lib, M, N, K)
    a_rows = max(min(tr, rows) for rows, tr, _ in parts)
    w_rows = min(parts[0][2], N)
    assert a_rows == tall, parts
    for which, rows in (("lda", a_rows), ("ldw", w_rows)):
        last = BC.gemm_last_ld(rows, K)
        assert BC.gemm_tile_span_ok(rows, rows, last, K) and not BC.gemm_tile_span_ok(rows, rows, last + 4, K)
        lda, ldw = (last + 4, K) if which == "lda" else (K, last + 4)
        _clear(lib)
        _refused(lib, lib.anyloc_gemm_nt(f, lda, f, ldw, None, f, N, M, N, K, None), "2 GiB", "2^31", f"{which}={last + 4}")


def test_gemm_nt_leading_dimension_below_the_row_length(lib, host):
    f = host["f"]
    _clear(lib)
    _refused(lib, lib.anyloc_gemm_nt(f, 60, f, 64, None, f, 128, 128, 128, 64, None), "at least K")
    _clear(lib)
    _refused(lib, lib.anyloc_gemm_nt(f, 64, f, -64, None, f, 128, 128, 128, 64, None), "at least K")


# ------------------------------------------------------------------------------------------------------------ attention
def test_attention_one_image_of_2gib(lib, host):
    """tokens * 3 * dim * 4 >= 2^31 for ONE image: refused in the uniform entry and in the ragged one, whatever the batch."""
    f, c = host["f"], BC.CASES["attn_one_image"]
    T, dim, heads = c["rows"] + 1, c["cols"] // 3, c["heads"]
    assert BC.attention_image_ok(T - 1, dim) and not BC.attention_image_ok(T, dim)
    for batch in (1, 3):
        _clear(lib)
        _refused(lib, lib.anyloc_attention(f, f, batch, T, dim, heads, None), "2 GiB", "tokens * 3 * dim * 4 < 2^31", f"tokens={T}")
    toks = (C.c_int32 * 2)(5, T)
    _clear(lib)
    _refused(lib, lib.anyloc_attention_ragged(f, f, 2, toks, host["i"], dim, heads, None), "2 GiB", f"tokens={T}")
    # one head, the longest rows the formula allows and one more
    T1 = (B31 - 1) // (3 * 64 * 4) + 1
    _clear(lib)
    _refused(lib, lib.anyloc_attention(f, f, 1, T1, 64, 1, None), "2 GiB", f"tokens={T1}")


@pytest.mark.parametrize("tokens,dim,heads", [(1 << 31, 64, 1), (16, (1 << 32) + 64, 1), (16, 64, (1 << 32) + 1)])
def test_attention_sizes_that_do_not_fit_32_bits(lib, host, tokens, dim, heads):
    """the kernels take tokens, dim and heads as int: a value that would be cut to its low 32 bits is refused by name"""
    f = host["f"]
    _clear(lib)
    _refused(lib, lib.anyloc_attention(f, f, 1, tokens, dim, heads, None), "below 2^31")


def test_attention_h3_operand_tiles_of_2gib(lib, host):
    """heads * ceil(rows / 32) * 8192 >= 2^31: refused IN FRONT of the launch that builds the tiles"""
    f = host["f"]
    B, T = 65535, 129
    assert BC.attention_h3_rows_ok(65535 * 128, 1) and not BC.attention_h3_rows_ok(B * T, 1)
    _clear(lib)
    _refused(lib, lib.anyloc_attention_h3(f, f, f, B, T, 64, 1, f, WS, None), "2 GiB", f"rows={B * T}")
    _clear(lib)
    _refused(lib, lib.anyloc_attention_h3(f, f, f, 1, 1 << 31, 64, 1, f, WS, None), "2^31")


# ------------------------------------------------------------------------------------------------------- VLAD / k-means
def test_vlad_hard_one_pass_unit_of_2gib(lib, host):
    """One image (the host knows its length) of 2^31 / (4 D) tokens per part and more; and a batch whose total cannot be
    shown to fit one unit.  Refused in front of the workspace check and the first launch."""
    f, i = host["f"], host["i"]
    for D in (384, 1536):
        limit = BC.fused_unit_rows(D)
        assert limit * D * 4 < B31 <= (limit + 16) * D * 4
        for parts in (1, 2, 64):
            n = limit * parts + 1
            assert BC.vlad_rows_per_part(n - 1, parts) == limit and BC.vlad_rows_per_part(n, parts) == limit + 16
            _clear(lib)
            _refused(lib, lib.anyloc_vlad_hard(f, i, 1, n, D, f, 8, 3 | (parts << 8), f, None, f, WS, None),
                     "2^31 / (4 D)", f"= {limit} tokens", f"{parts} part(s)")
    c = BC.CASES["tokens_8g"]
    n_img = -(-c["rows"] // c["n_tok"])
    assert lib.anyloc_vlad_auto_parts(c["rows"], n_img, 384, 8) == 1
    _clear(lib)
    _refused(lib, lib.anyloc_vlad_hard(f, i, n_img, c["rows"], 384, f, 8, 3, f, None, f, WS, None), "2^31 / (4 D)", f"{n_img} image(s)")


def test_ops_vlad_hands_a_long_batch_over_in_pieces_that_fit():
    """The Python surface reads the offsets once: ordinary images whose total passes the limit go over in pieces of whole images,
    every piece inside the limit at the whole batch's parts count; one image that cannot fit is a ValueError naming the limit."""
    from anyloc_amd import ops
    c = BC.CASES["tokens_8g"]
    D, K, n_tok, total = 384, 8, c["n_tok"], c["rows"]
    n_img = -(-total // n_tok)
    offsets = torch.clamp(torch.arange(n_img + 1, dtype=torch.int64) * n_tok, max=total)
    parts, pieces = ops._vlad_hard_pieces(offsets, n_img, total, D, K, 0)
    limit = ops.vlad_fused_unit_rows(D)
    assert limit == BC.fused_unit_rows(D) and parts == 1 and len(pieces) == -(-total // (limit // n_tok * n_tok))
    assert pieces[0][:1] == (0,) and pieces[-1][1] == n_img and pieces[-1][3] == total
    for (a0, a1, r0, r1), nxt in zip(pieces, pieces[1:] + [None]):
        assert a0 < a1 and (r0, r1) == (int(offsets[a0]), int(offsets[a1]))
        assert ops.vlad_rows_per_part(r1 - r0, parts) <= limit
        assert nxt is None or (nxt[0], nxt[2]) == (a1, r1)
    # an ordinary batch is one piece with the caller's parts untouched (its bits depend on them)
    assert ops._vlad_hard_pieces(offsets[:62], 61, 61 * n_tok, D, K, 0) == (0, [(0, 61, 0, 61 * n_tok)])
    assert ops._vlad_hard_pieces(offsets[:62], 61, 61 * n_tok, D, K, 5) == (5, [(0, 61, 0, 61 * n_tok)])
    # K = 33 or D = 128: the two-pass path, 64-bit throughout -- one piece
    assert ops._vlad_hard_pieces(offsets, n_img, total, D, 33, 0)[1] == [(0, n_img, 0, total)]
    one = torch.tensor([0, limit + 1], dtype=torch.int64)
    with pytest.raises(ValueError, match=rf"2\^31 / \(4 D\) = {limit}"):
        ops._vlad_hard_pieces(one, 1, limit + 1, D, K, 1)
    assert ops._vlad_hard_pieces(one, 1, limit + 1, D, K, 2) == (2, [(0, 1, 0, limit + 1)])


def _kmeans_ws(lib, n, D, K):
    return lib.anyloc_kmeans_workspace_bytes(n, D, K)


def test_kmeans_chunks_never_reach_2gib(lib, options):
    """kmeans_max_chunks = 1 on rows of 2 GiB and more gives MORE chunks, never a chunk the fused kernel cannot address; the
    workspace size function shows the chunk count (one [K, D] partial sum and K counters per chunk)."""
    n, D, K = BC.CASES["tokens_2g"]["rows"], 384, 32
    per_chunk = K * D * 4                                         # (a multiple of 256: no padding between the partial sums)
    sizes = {}
    for mc in (1, 2, 4, 8):
        options("kmeans_max_chunks", mc)
        sizes[mc] = _kmeans_ws(lib, n, D, K)
    chunks = {mc: BC.kmeans_chunks(n, D, mc) for mc in sizes}
    assert chunks == {1: 2, 2: 2, 4: 4, 8: 8}
    align = lambda b: -(-b // 256) * 256
    for mc in (2, 4, 8):
        want = (chunks[mc] - chunks[1]) * per_chunk + align(chunks[mc] * K * 4) - align(chunks[1] * K * 4)
        assert sizes[mc] - sizes[1] == want, (mc, sizes)
    # a row count one chunk serves: one chunk, and below it the option is obeyed as before
    n1 = BC.fused_unit_rows(D)
    options("kmeans_max_chunks", 1)
    assert _kmeans_ws(lib, n1 + 1, D, K) - _kmeans_ws(lib, n1, D, K) >= per_chunk
    assert BC.kmeans_chunks(n1, D, 1) == 1 and BC.kmeans_chunks(n1 + 1, D, 1) == 2


def test_row_counts_and_widths_that_do_not_fit_32_bits(lib, host):
    """the documented 32-bit sizes: one step past each, by name"""
    f, i = host["f"], host["i"]
    big = 1 << 31
    _clear(lib)
    _refused(lib, lib.anyloc_l2norm_rows(f, f, big, 4, 1e-12, None), "too many rows")
    _clear(lib)
    _refused(lib, lib.anyloc_layernorm(f, f, f, f, big, 4, 1e-6, None), "below 2^31")
    _clear(lib)
    _refused(lib, lib.anyloc_layernorm(f, f, f, f, 4, (1 << 32) + 4, 1e-6, None), "below 2^31")
    _clear(lib)
    _refused(lib, lib.anyloc_preprocess_u8(f, 1, 14, (1 << 32) + 14, 14, 14, host["f3"], host["f3"], f, None), "below 2^31")
    _clear(lib)
    _refused(lib, lib.anyloc_resize_bicubic(f, 1, 14, (1 << 32) + 14, 7, 7, 0, 0, 7, 7, f, None), "below 2^31")
    _clear(lib)
    _refused(lib, lib.anyloc_resize_bicubic(f, 1, 14, 14, 7, (1 << 32) + 7, 0, 0, 7, 7, f, None), "below 2^31")
    _clear(lib)
    _refused(lib, lib.anyloc_pool_tokens(f, None, 1, 2, 1 << 30, 0, 3.0, f, None), f"bad D={1 << 30}")
    _clear(lib)
    _refused(lib, lib.anyloc_vlad_residuals(f, big, 64, f, 4, 1, f, None), "bad shape")
    _clear(lib)
    _refused(lib, lib.anyloc_vlad_residuals(f, 4, (1 << 32) + 64, f, 4, 1, f, None), "below 2^31")
    _clear(lib)
    _refused(lib, lib.anyloc_vlad_hard(f, i, 1, big, 64, f, 4, 3, f, None, f, WS, None), "tokens < 2^31")
    _clear(lib)
    _refused(lib, lib.anyloc_vlad_hard(f, i, 1, 4, 1 << 21, f, 256, 3, f, None, f, WS, None), "desc_dim < 2^21")
    _clear(lib)
    _refused(lib, lib.anyloc_kmeans_step(f, 8, 1 << 21, f, 4, 0, f, f, i, f, WS, None), "below 2^21")
    _clear(lib)
    _refused(lib, lib.anyloc_kmeans_step(f, big, 64, f, 4, 0, f, f, i, f, WS, None), "fewer than 2^31")
    _clear(lib)
    _refused(lib, lib.anyloc_vlad_assigned(f, big, 64, f, 4, i, None, 3, f, f, WS, None), "n_tok < 2^31")
    _clear(lib)
    _refused(lib, lib.anyloc_vlad_soft(f, i, 1, big, 64, f, 4, 1.0, 3, f, f, WS, None), f"{big} tokens")
    _clear(lib)
    _refused(lib, lib.anyloc_kmeans_update(f, f, f, 256, 1 << 23, f, f, None), "bad shape")
    _clear(lib)
    _refused(lib, lib.anyloc_topk(f, big, f, 100, 64, 5, 0, 0, 0, f, i, f, WS, None), "too many queries")
    _clear(lib)
    _refused(lib, lib.anyloc_topk(f, 5, f, 300, 1 << 21, 5, 0, 0, 0, f, i, f, WS, None), "below 2^21")
    _clear(lib)
    _refused(lib, lib.anyloc_vlad_soft_weights(f, 4, 1 << 21, f, 4, 1.0, f, f, WS, None), "below 2^21")
    _clear(lib)
    _refused(lib, lib.anyloc_vlad_assigned(f, 4, 1 << 21, f, 4, i, None, 3, f, f, WS, None), "below 2^21")
    # the widest row these entry points take still fits the tallest tile of the GEMM they call
    assert BC.gemm_tile_span_ok(256, 256, (1 << 21) - 4, (1 << 21) - 4) and not BC.gemm_tile_span_ok(256, 256, 1 << 21, 1 << 21)
    _clear(lib)
    _refused(lib, lib.anyloc_split_h2(f, 64, big, 64, f, f, None), "split_h2", "below 2^31")
    _clear(lib)
    _refused(lib, lib.anyloc_split_x3(f, 64, big, 64, f, None), "split_x3", "below 2^31")
    _clear(lib)
    _refused(lib, lib.anyloc_split_x3(f, 1 << 22, 16, 1 << 22, f, None), "split_x3", "at most")


@pytest.mark.parametrize("K", [64, 1536, 4096])
def test_plane_images_on_both_sides_of_2gib(lib, host, K):
    """anyloc_h2_bytes = 4 bytes and anyloc_x3_bytes = 6 bytes per element of [rows, K padded to 16]; the GEMMs that read an
    image through a 32-bit descriptor refuse the first row count whose image reaches 2^31 bytes."""
    f = host["f"]
    for name, fn, gemm, planes in (("h2", lib.anyloc_h2_bytes, lib.anyloc_gemm_nt_h3, 2), ("x3", lib.anyloc_x3_bytes, lib.anyloc_gemm_nt_x6, 3)):
        per_row = K // 16 * planes * 32
        last = (B31 - 1) // per_row
        assert fn(last, K) == last * per_row < B31 <= fn(last + 1, K) == (last + 1) * per_row
        _clear(lib)
        if name == "h2":       # (as the A operand, then as W)
            _refused(lib, gemm(f, f, f, f, None, f, 16, last + 1, 16, K, None), "2 GiB")
            _clear(lib)
            _refused(lib, gemm(f, f, f, f, None, f, last + 1, 16, last + 1, K, None), "2 GiB")
        else:
            _refused(lib, gemm(f, f, None, f, 16, last + 1, 16, K, None), "2 GiB")
            _clear(lib)
            _refused(lib, gemm(f, f, None, f, last + 1, 16, last + 1, K, None), "2 GiB")


def test_extractor_max_rows_keeps_every_activation_image_below_2gib(lib):
    """HipDinoV2.max_rows for every model configuration the package knows: the plane image of that many rows, padded to the
    tallest row tile (256) as a forward's last tile pads them, at the wider of dim and ffn_hidden."""
    from anyloc_amd import extractor, synth
    archs = dict(synth.ARCH)
    assert len(archs) >= 8
    for name, (dim, depth, heads, ffn, hidden) in archs.items():
        rows = extractor.max_rows_for(dim, hidden)
        padded = -(-rows // 256) * 256
        width = max(dim, hidden)
        assert rows > 4096, name
        assert lib.anyloc_x3_bytes(padded, width) < B31 and lib.anyloc_h2_bytes(padded, width) < B31, name
        assert lib.anyloc_x3_bytes(rows + 513, width) >= B31 - 6 * width, name        # (and not needlessly small)


# ------------------------------------------------------------------------------------------------------- the case table
@pytest.mark.parametrize("case", sorted(BC.CASES))
def test_case_samples_hold_both_sides_of_every_boundary(case):
    c = BC.CASES[case]
    sample = set(BC.case_sample(case))
    assert len(sample) <= 1024 and max(sample) == c["rows"] - 1 and min(sample) == 0
    claimed = dict(c["crosses"])
    for name, stride, eb in c["operands"]:
        found = BC.crossings(c["rows"], stride, eb)
        assert sorted(found) == sorted(claimed.pop(name, [])), (case, name, found)
        for what, row in found.items():
            assert 0 < row < c["rows"] - 1 and {row - 1, row, row + 1} <= sample, (case, name, what, row)
            # the boundary lies inside the operand, with rows on both sides of it
            assert row * stride * eb <= {"2^31 B": B31, "2^32 B": 1 << 32, "2^31 el": B31 * eb}[what] < (row + 1) * stride * eb
    assert not claimed, claimed
    assert c["device_bytes"] <= 40 << 30
    assert c["rows"] * sum(s * e for _, s, e in c["operands"]) <= c["device_bytes"]


def test_generated_rows_do_not_depend_on_the_slab(lib):
    """a row regenerated alone is the row of the whole tensor (here: a small tensor filled in slabs of 1000 elements)"""
    for gen in BC.GENERATORS:
        whole = BC.fill(300, 384, gen, 5, "cpu", scale=4.0, slab_elems=1000)
        idx = [0, 1, 77, 299]
        assert torch.equal(whole[idx].double(), BC.rows_f64(idx, 384, gen, 5, 4.0))
        assert float(whole.abs().max()) <= {"scaled": 256.0, "bytes": 1020.0}.get(gen, 4.0) and whole.unique().numel() > 20


@pytest.mark.parametrize("case", ["tokens_2g", "tokens_8g"])
def test_token_cases_have_no_near_tie_and_exact_sums(case):
    """In the sampled rows the float64 reference's best centre leads the second by > 0.1 in both metrics (the kernels' fp32
    scores err by ~1e-6), the label is the row's own base direction, and the values lie on the 1 / 32 lattice with |x| <= 1
    (per-cluster sums of < 2^18 rows are then exact in fp32)."""
    c = BC.CASES[case]
    idx = BC.case_sample(case)
    x = BC.case_rows_f64(case, idx)
    cen = BC.token_centers(c["cols"], c["seed"]).double()
    assert bool((x * 32 == (x * 32).round()).all()) and float(x.abs().max()) <= 1.0
    assert bool((cen * 32 == (cen * 32).round()).all())
    own = BC.mode_of(torch.tensor(idx))
    cos = torch.nn.functional.normalize(x, dim=-1) @ torch.nn.functional.normalize(cen, dim=-1).T
    euc = 2 * x @ cen.T - (x * x).sum(-1, keepdim=True) - (cen * cen).sum(-1)[None]
    for sim in (cos, euc):
        top2 = sim.topk(2, dim=-1)
        assert torch.equal(top2.indices[:, 0], own)
        assert float((top2.values[:, 0] - top2.values[:, 1]).min()) > 0.1
    # every cluster gets its share, and no cluster more than 2^18 rows
    counts = torch.bincount(BC.mode_of(torch.arange(c["rows"])), minlength=BC.MODES)
    assert int(counts.min()) > c["rows"] // BC.MODES // 2 and int(counts.max()) < (1 << 18)
