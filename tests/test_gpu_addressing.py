"""Past 2 GiB every call is right or refused (profiles/addressing_audit.md): the entry points of include/anyloc_hip.h at the
thinnest shapes whose tensors, leading dimensions or units of work cross 2^31 bytes, 2^32 bytes or 2^31 elements, and
the last served shape next to every refusal that tests/test_addressing_limits_cpu.py makes from the other side.

Inputs come from the closed formula of tests/_big_cases.py, generated on the device in slabs; any row is regenerated
alone on the CPU for its float64 reference.  Outputs start as 0xFF bytes (NaN as fp32, -1 as int64: the fresh pattern of
tests/_guard_arena.py), so an element nobody wrote cannot pass.  Compared: the first and last 64 rows, 64 rows around
every row where an operand crosses a boundary, 256 seeded random rows; reductions over all rows (k-means sums and
counts, an image's VLAD, a pooled image) in full against float64 on the device.  Bars: those of each family's own test,
imported; no label is excused (the inputs have no near-tie, which the CPU module checks).

Every test states its device bytes in the case table, skips only when the device has less free memory than that, and
frees what it held before the next one starts."""
import ctypes as C
import gc
import time

import pytest
import torch

import _big_cases as BC
import _vlad_refs as VR
import test_gpu_kernels as TK
import test_gpu_long_sequences as TL
import test_gpu_pca as TPCA
import test_gpu_pooling as TP
import test_gpu_vlad_soft as VS
import test_gpu_vlad_topk as VT
import test_gpu_x6 as X6
from oracle import vlad_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_INVALID_ARG = -1


@pytest.fixture(autouse=True)
def _isolated(request):
    """each test's wall time; its tensors, the library's workspaces and the allocator's cache are gone when it ends; so are
    the options it set and the CPU thread count it ran under"""
    from anyloc_amd import _lib
    t0 = time.time()
    # (the sampled rows are regenerated, and the oracles run, on the CPU: at most 16 threads, whatever a module imported before
    # this one asked for -- hundreds of threads on a few cores make every small tensor operation slow)
    threads = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, threads)))
    yield
    torch.set_num_threads(threads)
    torch.cuda.synchronize()
    _lib.release_workspaces()
    assert _lib.load().anyloc_reset_options() == 0
    gc.collect()
    torch.cuda.empty_cache()
    print(f"\n[addressing] {request.node.name}: {time.time() - t0:.2f} s")


def _room(case):
    """skip only when the device cannot hold the case"""
    need = BC.CASES[case]["device_bytes"]
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"{case} needs {need >> 30} GiB of device memory, {free >> 30} GiB are free")


def fresh(shape, dtype=torch.float32):
    """an output nobody has written: every byte 0xFF"""
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(-1).view(torch.uint8).fill_(0xFF)
    return t


def untouched(t):
    return bool((t.view(-1).view(torch.uint8) == 0xFF).all())


def written(t):
    """no element of a float output is still NaN"""
    return not bool(torch.isnan(t).any())


def _lib_and_ptrs():
    from anyloc_amd import _lib
    return _lib.load(), _lib.ptr, _lib.stream_ptr()


def _ok(lib, status, what):
    assert status == 0, (what, status, lib.anyloc_last_error().decode())


def _refused(lib, status, *words):
    msg = lib.anyloc_last_error().decode()
    assert status == ERR_INVALID_ARG, (status, msg)
    for w in words:
        assert w in msg, (w, msg)


def _idx(rows):
    return torch.tensor(rows, dtype=torch.int64, device=DEV)


# ----------------------------------------------------------------------------------------- rows: l2norm, layernorm, pool
def test_l2norm_rows_past_4_gib():
    """262 500 x 4092: the input and the output cross 2^31 and 2^32 bytes inside a row; out of place, then in place."""
    _room("rows_4g")
    lib, ptr, stream = _lib_and_ptrs()
    c = BC.CASES["rows_4g"]
    x = BC.case_fill("rows_4g", DEV)
    out = fresh(x.shape)
    sample = BC.case_sample("rows_4g")
    ref = torch.nn.functional.normalize(BC.case_rows_f64("rows_4g", sample), dim=-1)
    _ok(lib, lib.anyloc_l2norm_rows(ptr(x), ptr(out), c["rows"], c["cols"], 1e-12, stream), "l2norm_rows")
    assert written(out)
    err = TK._rel(out[_idx(sample)].cpu(), ref)
    _ok(lib, lib.anyloc_l2norm_rows(ptr(x), ptr(x), c["rows"], c["cols"], 1e-12, stream), "l2norm_rows in place")
    err_in = TK._rel(x[_idx(sample)].cpu(), ref)
    print(f"[l2norm 4 GiB] rel error {err:.3e} out of place, {err_in:.3e} in place (bar {TK.L2NORM_REL:.0e})")
    assert err < TK.L2NORM_REL and err_in < TK.L2NORM_REL
    assert torch.equal(out, x)            # every row of the two, not only the sampled ones


def test_layernorm_past_4_gib():
    _room("rows_4g")
    lib, ptr, stream = _lib_and_ptrs()
    c = BC.CASES["rows_4g"]
    x = BC.case_fill("rows_4g", DEV)
    out = fresh(x.shape)
    dim = c["cols"]
    w = BC.rows_f64([0], dim, "unit", 101)[0] + 1.5
    b = BC.rows_f64([0], dim, "unit", 102)[0]
    sample = BC.case_sample("rows_4g")
    ref = torch.nn.functional.layer_norm(BC.case_rows_f64("rows_4g", sample), (dim,), w, b, 1e-6)
    w_d, b_d = w.float().to(DEV), b.float().to(DEV)
    _ok(lib, lib.anyloc_layernorm(ptr(x), ptr(out), ptr(w_d), ptr(b_d), c["rows"], dim, 1e-6, stream), "layernorm")
    assert written(out)
    err = float((out[_idx(sample)].cpu().double() - ref).abs().max())
    print(f"[layernorm 4 GiB] largest error {err:.3e} (bar {TK.LAYERNORM_ATOL:.0e})")
    assert err < TK.LAYERNORM_ATOL
    # the rows nobody sampled: mean b-weighted statistics of every row against float64 on the device, in slabs
    worst = 0.0
    for r0 in range(0, c["rows"], 16384):
        xs = x[r0:r0 + 16384].double()
        want = torch.nn.functional.layer_norm(xs, (dim,), w_d.double(), b_d.double(), 1e-6)
        worst = max(worst, float((out[r0:r0 + 16384].double() - want).abs().max()))
    assert worst < TK.LAYERNORM_ATOL, worst


def _pool_f64(x, mode, p):
    x = x.double()
    if mode == "average":
        return x.mean(0)
    if mode == "max":
        return x.max(0).values
    if mode == "gem":
        m = x.pow(p).mean(0)
        return m.abs().pow(1.0 / p) * torch.sign(m)
    return x.abs().pow(p).mean(0).pow(1.0 / p)


def test_pool_tokens_images_across_2_and_4_gib():
    """191 images of 1369 tokens and one of 1021, 4092 columns: one image straddles 2^31 bytes, one 2^32 bytes.  Every image
    of every mode against float64 on the device; ragged (offsets) and uniform (n_tok) addressing."""
    from anyloc_amd import ops
    _room("pool_4g")
    lib, ptr, stream = _lib_and_ptrs()
    c = BC.CASES["pool_4g"]
    rows, D, n_tok = c["rows"], c["cols"], c["n_tok"]
    x = BC.case_fill("pool_4g", DEV)
    n_full = rows // n_tok
    off_h = [i * n_tok for i in range(n_full + 1)] + [rows]
    offsets = torch.tensor(off_h, dtype=torch.int64, device=DEV)
    straddled = {b // n_tok for b in BC.case_boundary_rows("pool_4g")}
    assert len(straddled) == 2 and all(b % n_tok not in (0, n_tok - 1) for b in BC.case_boundary_rows("pool_4g"))
    for mode in ("average", "max", "gem", "gem_abs"):
        code = ops.POOL_MODES[mode]
        p = 3.0
        want = torch.stack([_pool_f64(x[off_h[i]:off_h[i + 1]], mode, p) for i in range(n_full + 1)])
        out = fresh((n_full + 1, D))
        _ok(lib, lib.anyloc_pool_tokens(ptr(x), ptr(offsets), n_full + 1, -1, D, code, p, ptr(out), stream), f"pool {mode}")
        out_u = fresh((n_full, D))
        _ok(lib, lib.anyloc_pool_tokens(ptr(x), None, n_full, n_tok, D, code, p, ptr(out_u), stream), f"pool {mode} uniform")
        assert written(out) and written(out_u)
        err = TP.rel_err(out, want.cpu())
        print(f"[pool {mode} 4 GiB] worst image {err:.3e} (bar {TP.REL:.0e})")
        assert err < TP.REL, (mode, err)
        assert torch.equal(out_u, out[:n_full]), mode


# ---------------------------------------------------------------------------------------------------------- k-means
def _labels_f64(x, centers, mode, slab=1 << 18):
    """float64 arg-max of the fast-pytorch-kmeans similarity of every row, on the device"""
    cd = centers.double()
    out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    for r0 in range(0, x.shape[0], slab):
        xs = x[r0:r0 + slab].double()
        if mode == "cosine":
            sim = (xs / (xs.norm(dim=-1, keepdim=True) + 1e-8)) @ (cd / (cd.norm(dim=-1, keepdim=True) + 1e-8)).T
        else:
            sim = 2 * xs @ cd.T - (xs * xs).sum(-1, keepdim=True) - (cd * cd).sum(-1)[None]
        out[r0:r0 + slab] = sim.argmax(-1)
    return out


def _sums_f64(x, labels, K, slab=1 << 18):
    sums = torch.zeros(K, x.shape[1], dtype=torch.float64, device=x.device)
    for r0 in range(0, x.shape[0], slab):
        sums.index_add_(0, labels[r0:r0 + slab], x[r0:r0 + slab].double())
    return sums


def _kmeans_step(x, centers, mode):
    """anyloc_kmeans_step into fresh outputs -> (sums, counts, labels)"""
    from anyloc_amd import _lib
    lib, ptr, stream = _lib_and_ptrs()
    n, D = x.shape
    K = centers.shape[0]
    sums, counts, labels = fresh((K, D)), fresh((K,)), fresh((n,), torch.int64)
    ws = _lib.workspace(lib.anyloc_kmeans_workspace_bytes(n, D, K), x.device, "kmeans")
    _ok(lib, lib.anyloc_kmeans_step(ptr(x), n, D, ptr(centers), K, 0 if mode == "cosine" else 1, ptr(sums), ptr(counts), ptr(labels),
                                    ptr(ws), ws.numel(), stream), "kmeans_step")
    return sums, counts, labels


def _check_kmeans(case, x, centers, mode, got, tag):
    sums, counts, labels = got
    c = BC.CASES[case]
    K = centers.shape[0]
    sample = BC.case_sample(case)
    own = BC.mode_of(torch.tensor(sample))
    assert torch.equal(labels[_idx(sample)].cpu(), own), tag                # the rows regenerated on the CPU: no label excused
    want_lab = _labels_f64(x, centers, mode)
    differ = int((labels != want_lab).sum())
    assert differ == 0, (tag, differ)
    assert torch.equal(counts.double(), torch.bincount(want_lab, minlength=K).double()), tag
    assert float(counts.sum()) == c["rows"]
    err = VR.l2rel(sums, _sums_f64(x, want_lab, K))
    print(f"[kmeans {tag}] sums l2rel {err:.3e} (bar {VT.KMEANS_SUMS_RTOL:.0e}), 0 labels differ")
    assert err < VT.KMEANS_SUMS_RTOL, (tag, err)


@pytest.mark.parametrize("mode", ["cosine", "euclidean"])
def test_kmeans_step_one_chunk_of_2_gib(mode):
    """1 398 400 rows of 384 floats, 304 rows past 2 GiB: with kmeans_max_chunks = 1 (and 2: the same two chunks) no chunk may
    reach 2 GiB -- a chunk that does reads its tail as zero rows (label 0, nothing added).  Default chunking next to them."""
    from anyloc_amd import ops
    _room("tokens_2g")
    c = BC.CASES["tokens_2g"]
    x = BC.case_fill("tokens_2g", DEV)
    centers = BC.token_centers(c["cols"], c["seed"]).to(DEV)
    for max_chunks in (1, 2, 0):
        with ops.options(kmeans_max_chunks=max_chunks):
            got = _kmeans_step(x, centers, mode)
        _check_kmeans("tokens_2g", x, centers, mode, got, f"2 GiB, {mode}, kmeans_max_chunks={max_chunks}")


@pytest.mark.parametrize("mode", ["cosine", "euclidean"])
def test_kmeans_step_past_2g_elements(mode):
    """5 592 500 x 384 = 2^31 + 36 352 elements under default chunking"""
    _room("tokens_8g")
    c = BC.CASES["tokens_8g"]
    x = BC.case_fill("tokens_8g", DEV)
    centers = BC.token_centers(c["cols"], c["seed"]).to(DEV)
    _check_kmeans("tokens_8g", x, centers, mode, _kmeans_step(x, centers, mode), f"8 GiB, {mode}")


# ------------------------------------------------------------------------------------------------------------- VLAD
def _vlad_hard(x, offsets, n_img, centers, flags, labels=True):
    """anyloc_vlad_hard into fresh outputs -> (status, out, labels)"""
    from anyloc_amd import _lib
    lib, ptr, stream = _lib_and_ptrs()
    total, D = x.shape
    K = centers.shape[0]
    out, lab = fresh((n_img, K * D)), fresh((total,), torch.int64) if labels else None
    ws = _lib.workspace(lib.anyloc_vlad_workspace_bytes_parts(total, n_img, D, K, (flags >> 8) & 0x7f), x.device, "vlad")
    st = lib.anyloc_vlad_hard(ptr(x), ptr(offsets), n_img, total, D, ptr(centers), K, flags, ptr(out), ptr(lab), ptr(ws), ws.numel(), stream)
    return st, out, lab


def test_vlad_hard_one_image_of_2_gib():
    """ONE image of 1 398 400 tokens at D = 384.  One-pass kernel: at one part the image is 2 GiB and more -- refused, nothing
    written, and ops.vlad says so before any call; at two parts each unit is 1 GiB -- served (the second part starts past
    2^30 bytes).  Two-pass path (option vlad_two_pass): served, 64-bit throughout.  Raw tokens (no NORM_DESCS): residuals on
    the 1 / 32 lattice, sums exact in fp32."""
    from anyloc_amd import ops
    _room("tokens_2g")
    lib, ptr, stream = _lib_and_ptrs()
    c = BC.CASES["tokens_2g"]
    n, D = c["rows"], c["cols"]
    x = BC.case_fill("tokens_2g", DEV)
    centers = BC.token_centers(D, c["seed"]).to(DEV)
    offsets = torch.tensor([0, n], dtype=torch.int64, device=DEV)
    assert BC.vlad_rows_per_part(n, 1) > BC.fused_unit_rows(D) >= BC.vlad_rows_per_part(n, 2)
    st, out, lab = _vlad_hard(x, offsets, 1, centers, ops.VLAD_INTRA_NORM | (1 << 8))
    _refused(lib, st, "2^31 / (4 D)", "1 part(s)")
    torch.cuda.synchronize()
    assert untouched(out) and untouched(lab)
    with pytest.raises(ValueError, match=r"2\^31 / \(4 D\)"):
        ops.vlad((x, offsets), centers, norm_descs=False, parts=1)
    want_lab = _labels_f64(x, centers, "cosine")
    sample = BC.case_sample("tokens_2g")
    assert torch.equal(want_lab[_idx(sample)].cpu(), BC.mode_of(torch.tensor(sample)))
    want = VR.hard_vlad_f64(x, centers, want_lab, False, slab=1 << 18)
    for tag, opts, flags in (("one-pass, 2 parts", {}, ops.VLAD_INTRA_NORM | (2 << 8)), ("two-pass", dict(vlad_two_pass=1), ops.VLAD_INTRA_NORM)):
        with ops.options(**opts):
            st, out, lab = _vlad_hard(x, offsets, 1, centers, flags)
        _ok(lib, st, tag)
        assert int((lab != want_lab).sum()) == 0, tag
        err = VR.l2rel(out[0], want)
        print(f"[vlad hard, one image of 2 GiB, {tag}] l2rel {err:.3e} (bar {VT.VLAD_RTOL:.0e})")
        assert err < VT.VLAD_RTOL, (tag, err)


def test_vlad_hard_batch_past_2g_elements():
    """4085 images of 1369 tokens and one of 135, 2^31 + 36 352 elements in all.  The C entry point cannot read the offsets and
    refuses the one-pass kernel a batch whose total might be one image; ops.vlad hands it over in pieces that fit, and the
    two-pass path takes it in one call.  Images around every boundary, the first, the last: each against float64."""
    from anyloc_amd import ops
    _room("tokens_8g")
    lib, ptr, stream = _lib_and_ptrs()
    c = BC.CASES["tokens_8g"]
    total, D, n_tok = c["rows"], c["cols"], c["n_tok"]
    x = BC.case_fill("tokens_8g", DEV)
    centers = BC.token_centers(D, c["seed"]).to(DEV)
    n_img = -(-total // n_tok)
    off_h = [min(i * n_tok, total) for i in range(n_img + 1)]
    offsets = torch.tensor(off_h, dtype=torch.int64, device=DEV)
    st, out, _ = _vlad_hard(x, offsets, n_img, centers, 3, labels=False)
    _refused(lib, st, "2^31 / (4 D)", f"{n_img} image(s)")
    torch.cuda.synchronize()
    assert untouched(out)
    del out
    images = {0, 1, n_img - 2, n_img - 1}
    for b in BC.case_boundary_rows("tokens_8g"):
        images |= {b // n_tok + d for d in (-2, -1, 0, 1, 2)}
    pieces = ops._vlad_hard_pieces(offsets, n_img, total, D, centers.shape[0], 0)[1]
    images |= {p[0] + d for p in pieces[1:] for d in (-1, 0)}               # both sides of every seam between two pieces
    images = {i for i in images if 0 <= i < n_img}
    for norm_descs in (True, False):
        results = {"one-pass in pieces": ops.vlad((x, offsets), centers, norm_descs=norm_descs, return_labels=True)}
        with ops.options(vlad_two_pass=1):
            results["two-pass"] = ops.vlad((x, offsets), centers, norm_descs=norm_descs, return_labels=True)
        for tag, (out, lab) in results.items():
            assert written(out) and abs(float(out.norm(dim=1).min()) - 1.0) < 1e-5 and abs(float(out.norm(dim=1).max()) - 1.0) < 1e-5
            worst = 0.0
            for i in sorted(images):
                xi = x[off_h[i]:off_h[i + 1]]
                want_lab = _labels_f64(xi, centers, "cosine")
                assert torch.equal(lab[off_h[i]:off_h[i + 1]], want_lab), (tag, i)
                err = VR.l2rel(out[i], VR.hard_vlad_f64(xi, centers, want_lab, norm_descs, slab=1 << 18))
                assert err < VT.VLAD_RTOL, (tag, i, err)
                worst = max(worst, err)
            print(f"[vlad hard, 8 GiB batch, {tag}, norm_descs={norm_descs}] worst of {len(images)} images {worst:.3e} (bar {VT.VLAD_RTOL:.0e})")
        assert torch.equal(results["one-pass in pieces"][1], results["two-pass"][1])


# ----------------------------------------------------------------------------------------------------------- fp32 GEMM
def _gemm_nt(a, lda, w, ldw, out, ldc, M, N, K):
    lib, ptr, stream = _lib_and_ptrs()
    return lib.anyloc_gemm_nt(ptr(a), lda, ptr(w), ldw, None, ptr(out), ldc, M, N, K, stream)


def _check_gemm_rows(out_rows, a_rows, w):
    """rows of C (CPU) against float64 under the bound of tests/test_gpu_kernels.py::test_gemm_nt"""
    ref = a_rows @ w.T
    bound = TK.gemm_nt_bound(a_rows.abs() @ w.abs().T)
    diff = (out_rows.double() - ref).abs()
    assert bool((diff <= bound).all()), float((diff / bound).max())
    return float((diff / bound).max())


@pytest.mark.parametrize("case", ["gemm_c_8g", "gemm_a_8g"])
def test_gemm_nt_operand_past_2g_elements(case):
    """C [2 097 400, 1024] from K = 4, and A [2 097 400, 1024] into 64 columns: M * ld past 2^31 elements"""
    _room(case)
    lib, ptr, stream = _lib_and_ptrs()
    c = BC.CASES[case]
    M, K, N = c["rows"], c["cols"], c["N"]
    a = BC.case_fill(case, DEV)
    w64 = BC.rows_f64(list(range(N)), K, "unit", c["seed"] + 50)
    w = w64.float().to(DEV)
    out = fresh((M, N))
    _ok(lib, _gemm_nt(a, K, w, K, out, N, M, N, K), case)
    assert written(out)
    sample = BC.case_sample(case)
    worst = _check_gemm_rows(out[_idx(sample)].cpu(), BC.case_rows_f64(case, sample), w64)
    print(f"[{case}] largest error / bound {worst:.3f}")


@pytest.mark.parametrize("cfg,M,N,K,side", [(0, 128, 128, 36, "A"), (1, 256, 128, 64, "A"), (0, 64, 128, 64, "A"), (0, 128, 128, 36, "W")])
def test_gemm_nt_widest_row_stride_a_tile_is_served_with(cfg, M, N, K, side):
    """A row-strided view of a very wide matrix: the last leading dimension whose tile rows stay inside 2 GiB is served -- every
    row right, the last rows of the tile above all -- and the next multiple of 4 is refused with nothing written.  Tile
    heights 128, 256 (gemm_f32_cfg = 1) and 64, as the plan says; the W operand likewise."""
    from anyloc_amd import _lib, ops
    _room("gemm_view_2g")
    lib, ptr, stream = _lib_and_ptrs()
    with ops.options(gemm_f32_cfg=cfg):
        d = _lib.GemmPlanDesc()
        assert lib.anyloc_gemm_plan_describe(M, N, K, b"store", 0, C.byref(d)) == 0
        tall = max(min(d.part[i].tile_rows, d.part[i].rows) for i in range(d.parts)) if side == "A" else min(d.part[0].tile_cols, N)
        assert tall == {(0, 128): 128, (1, 256): 256, (0, 64): 64}[(cfg, M)] if side == "A" else tall == 128
        ld = BC.gemm_last_ld(tall, K)
        rows = M if side == "A" else N
        assert (rows - 1) * ld * 4 + K * 4 + (1 << 30) <= BC.CASES["gemm_view_2g"]["device_bytes"]
        buf = torch.zeros((rows - 1) * ld + K, dtype=torch.float32, device=DEV)       # the rows of the view; zeros between them
        vals = BC.rows_f64(list(range(rows)), K, "unit", 60 + cfg)
        torch.as_strided(buf, (rows, K), (ld, 1)).copy_(vals.float())
        other64 = BC.rows_f64(list(range(N if side == "A" else M)), K, "unit", 70)
        other = other64.float().to(DEV)
        out = fresh((M, N))
        a, lda, w, ldw = (buf, ld, other, K) if side == "A" else (other, K, buf, ld)
        _ok(lib, _gemm_nt(a, lda, w, ldw, out, N, M, N, K), f"ld={ld}")
        a64, w64 = (vals, other64) if side == "A" else (other64, vals)
        worst = _check_gemm_rows(out.cpu(), a64, w64)
        print(f"[gemm_nt {side} view, tile of {tall} rows, ld={ld}] largest error / bound {worst:.3f}")
        out = fresh((M, N))
        lda, ldw = (ld + 4, K) if side == "A" else (K, ld + 4)
        _refused(lib, _gemm_nt(a, lda, w, ldw, out, N, M, N, K), "2 GiB", f"ld{'a' if side == 'A' else 'w'}={ld + 4}")
        torch.cuda.synchronize()
        assert untouched(out)


# ------------------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("kernel", ["fp32-mfma", "split-bf16"])
def test_attention_many_images_past_2g_elements(kernel):
    """65 535 images of 171 tokens, one head: qkv crosses 2^31 bytes, 2^32 bytes and 2^31 elements, the output 2^31 bytes.  The
    images around every boundary, the first and last, and 32 seeded ones against float64 (tests/test_gpu_kernels.py)."""
    from anyloc_amd import ops
    _room("attn_8g")
    lib, ptr, stream = _lib_and_ptrs()
    c = BC.CASES["attn_8g"]
    T, B = c["n_tok"], c["rows"] // c["n_tok"]
    qkv = BC.case_fill("attn_8g", DEV)
    out = fresh((c["rows"], 64))
    with ops.options(attn_x6=TK.ATTN_KERNELS[kernel][0]):
        _ok(lib, lib.anyloc_attention(ptr(qkv), ptr(out), B, T, 64, 1, stream), "attention")
    assert written(out)
    images = {0, 1, B - 2, B - 1} | {b // T + d for b in BC.case_boundary_rows("attn_8g") for d in (-1, 0, 1)}
    images |= set(torch.randint(0, B, (32,), generator=torch.Generator().manual_seed(c["seed"])).tolist())
    images = sorted(i for i in images if 0 <= i < B)
    rows = [i * T + t for i in images for t in range(T)]
    got = out[_idx(rows)].cpu().reshape(len(images), T, 64)
    worst = TK.check_attention(got, BC.case_rows_f64("attn_8g", rows).float().reshape(len(images), T, 192), 1)
    print(f"[attention {kernel}, 8 GiB] largest error over {len(images)} images {worst:.3e} (bar {TK.ATTN_ATOL:.0e})")


@pytest.mark.parametrize("kernel", ["fp32-mfma", "split-bf16"])
def test_attention_longest_image_and_the_first_refused(kernel):
    """ONE image of 21 845 tokens x 128 heads: tokens * 3 * dim * 4 = 2^31 - 32 768, the last the descriptor of an image's rows
    holds; the first and the last head (the last bytes of every row) in full against float64 on the device, under the bar
    of the family's long-sequence test (tests/test_gpu_long_sequences.py: 5330 tokens there).  One token more is refused with
    nothing written."""
    from anyloc_amd import ops
    _room("attn_one_image")
    lib, ptr, stream = _lib_and_ptrs()
    c = BC.CASES["attn_one_image"]
    T, heads = c["rows"], c["heads"]
    D = heads * 64
    assert BC.attention_image_ok(T, D) and not BC.attention_image_ok(T + 1, D)
    qkv = BC.case_fill("attn_one_image", DEV)
    out = fresh((T, D))
    with ops.options(attn_x6=TK.ATTN_KERNELS[kernel][0]):
        _ok(lib, lib.anyloc_attention(ptr(qkv), ptr(out), 1, T, D, heads, stream), "attention")
        assert written(out)
        for h in (0, heads - 1):
            q, k, v = (qkv[:, j * D + h * 64:j * D + (h + 1) * 64].double() for j in range(3))
            ref = torch.zeros(T, 64, dtype=torch.float64, device=DEV)
            smax = torch.zeros(T, dtype=torch.float64, device=DEV)
            for r0 in range(0, T, 4096):
                s = (q[r0:r0 + 4096] * 0.125) @ k.T
                smax[r0:r0 + 4096] = s.abs().amax(dim=1)
                ref[r0:r0 + 4096] = torch.softmax(s, dim=-1) @ v
            err = (out[:, h * 64:(h + 1) * 64].double() - ref).abs().amax(dim=1)
            worst = TL.check_attention_long(err, smax, float(v.abs().max()), ref.abs().max())
            print(f"[attention {kernel}, one image of 2 GiB, head {h}] largest error {float(err.max()):.3e}, {worst:.3f} of the row's bar; "
                  f"relative to the largest output {float(err.max() / ref.abs().max()):.3e} (bar 1e-05)")
        out = fresh((64, D))
        _refused(lib, lib.anyloc_attention(ptr(qkv), ptr(out), 1, T + 1, D, heads, stream), "2 GiB", f"tokens={T + 1}")
    torch.cuda.synchronize()
    assert untouched(out)


def test_attention_h3_most_rows_its_tiles_hold_and_the_first_refused():
    """65 535 images of 128 tokens, one head: 262 140 groups of 32 rows, the q | k | v tile images 4 groups short of 2 GiB each;
    qkv crosses 2^31 and 2^32 bytes.  The images around the boundaries, both ends and 32 seeded ones against float64 under the
    bars of tests/test_gpu_kernels.py.  One token more per image is refused in front of the launch that builds the tiles."""
    from anyloc_amd import _lib
    _room("attn_h3_6g")
    lib, ptr, stream = _lib_and_ptrs()
    c = BC.CASES["attn_h3_6g"]
    T, B = c["n_tok"], c["rows"] // c["n_tok"]
    assert BC.attention_h3_rows_ok(B * T, 1) and not BC.attention_h3_rows_ok(B * (T + 1), 1)
    qkv = BC.case_fill("attn_h3_6g", DEV)
    img = fresh((lib.anyloc_h2_bytes(B * T, 64),), torch.uint8)
    inv = fresh((B * T,))
    ws = _lib.workspace(lib.anyloc_attention_h3_workspace_bytes(B, T, 1), qkv.device, "attn_h3")
    _refused(lib, lib.anyloc_attention_h3(ptr(qkv), ptr(img), ptr(inv), B, T + 1, 64, 1, ptr(ws), 1 << 40, stream), "2 GiB", f"rows={B * (T + 1)}")
    torch.cuda.synchronize()
    assert untouched(inv) and untouched(img[:1 << 20]) and untouched(img[-(1 << 20):])
    _ok(lib, lib.anyloc_attention_h3(ptr(qkv), ptr(img), ptr(inv), B, T, 64, 1, ptr(ws), ws.numel(), stream), "attention_h3")
    assert written(inv)
    images = {0, 1, B - 2, B - 1} | {b // T + d for b in BC.case_boundary_rows("attn_h3_6g") for d in (-1, 0, 1)}
    images |= set(torch.randint(0, B, (32,), generator=torch.Generator().manual_seed(c["seed"])).tolist())
    images = sorted(i for i in images if 0 <= i < B)
    rows = [i * T + t for i in images for t in range(T)]
    planes = _plane_rows(img, torch.float16, 2, B * T, 64, rows)
    inv_s = inv[_idx(rows)]
    out = ((planes[0] + planes[1]) * inv_s.double()[:, None]).cpu().reshape(len(images), T, 64)
    worst = TK.check_attention_h3_decoded(out, inv_s, BC.case_rows_f64("attn_h3_6g", rows).float().reshape(len(images), T, 192), 1)
    print(f"[attention_h3, 6 GiB] largest error over {len(images)} images {worst:.3e}")


# ------------------------------------------------------------------------------------------- residuals, plane splitters
def test_vlad_residuals_output_past_2g_elements():
    """174 800 tokens x 32 centres x 384: out crosses 2^31 bytes, 2^32 bytes and 2^31 elements.  Raw tokens: x - c on the 1 / 32
    lattice, bit-exact in every element; normalised tokens: the sampled rows within the l2norm bar plus the one rounding of the
    subtraction (2^-23 for values below 2)."""
    from anyloc_amd import ops
    _room("resid_8g")
    lib, ptr, stream = _lib_and_ptrs()
    c = BC.CASES["resid_8g"]
    n, D, K = c["rows"], c["cols"], BC.MODES
    x = BC.case_fill("resid_8g", DEV)
    centers = BC.token_centers(D, c["seed"]).to(DEV)
    out = fresh((n, K, D))
    _ok(lib, lib.anyloc_vlad_residuals(ptr(x), n, D, ptr(centers), K, 0, ptr(out), stream), "vlad_residuals")
    for r0 in range(0, n, 8192):
        assert torch.equal(out[r0:r0 + 8192], x[r0:r0 + 8192, None, :] - centers[None]), r0
    out.view(-1).view(torch.uint8).fill_(0xFF)
    _ok(lib, lib.anyloc_vlad_residuals(ptr(x), n, D, ptr(centers), K, ops.VLAD_NORM_DESCS, ptr(out), stream), "vlad_residuals, normalised")
    assert written(out)
    sample = BC.case_sample("resid_8g")
    ref = torch.nn.functional.normalize(BC.case_rows_f64("resid_8g", sample), dim=-1)[:, None, :] - centers.cpu().double()[None]
    err = float((out[_idx(sample)].cpu().double() - ref).abs().max())
    print(f"[vlad_residuals 8 GiB] largest error {err:.3e} (bar {TK.L2NORM_REL + 2.0 ** -23:.2e})")
    assert err < TK.L2NORM_REL + 2.0 ** -23


def _plane_rows(img, dtype, planes, rows, K, idx):
    """the rows ``idx`` of a plane image [K / 16][plane][row][16] (16-byte halves of a row swapped when (row >> 3) & 1: the
    layout tests/test_gpu_x6.py decodes whole) -> float64 [planes, len(idx), K] on the device"""
    k16 = K // 16
    i = _idx(idx)
    t = img.view(dtype)[:k16 * planes * rows * 16].reshape(k16, planes, rows, 2, 8)[:, :, i].clone()
    odd = ((i >> 3) & 1).bool()
    t[:, :, odd] = t[:, :, odd].flip(3)
    return t.permute(1, 2, 0, 3, 4).reshape(planes, len(idx), K).double()


def _image_boundary_rows(nbytes, rows):
    """rows of a plane image [kb][plane][row][32 bytes] whose 32 bytes hold byte 2^31, 2^32 or 2^33 of the image"""
    return sorted({(b // 32) % rows for b in (1 << 31, 1 << 32, 1 << 33) if b < nbytes})


@pytest.mark.parametrize("name", ["h2", "x3"])
def test_split_h2_and_x3_past_2g_elements(name):
    """524 400 rows of 4096 columns (2^31 + 458 752 elements), row magnitudes 2^-6 .. 2^6: the plane images are 8 and 12 GiB.
    Sampled rows -- those where the INPUT crosses a boundary and those whose 32 image bytes hold byte 2^31, 2^32, 2^33 of the
    image -- are rebuilt from the planes: two fp16 planes within 2^-22 of the row maximum (tests/test_gpu_x6.py), three bf16
    planes exactly."""
    _room("split_8g")
    lib, ptr, stream = _lib_and_ptrs()
    c = BC.CASES["split_8g"]
    rows, K = c["rows"], c["cols"]
    x = BC.case_fill("split_8g", DEV)
    for planes, dtype, nbytes in {"h2": [(2, torch.float16, lib.anyloc_h2_bytes(rows, K))], "x3": [(3, torch.bfloat16, lib.anyloc_x3_bytes(rows, K))]}[name]:
        img = fresh((nbytes,), torch.uint8)
        sample = sorted(set(BC.case_sample("split_8g")) | {r + d for r in _image_boundary_rows(nbytes, rows) for d in range(-8, 9) if 0 <= r + d < rows})
        want = BC.case_rows_f64("split_8g", sample)
        if name == "h2":
            inv = fresh((rows,))
            _ok(lib, lib.anyloc_split_h2(ptr(x), K, rows, K, ptr(img), ptr(inv), stream), "split_h2")
            assert written(inv)
            p = _plane_rows(img, dtype, planes, rows, K, sample)
            back = ((p[0] + p[1]) * inv[_idx(sample)].double()[:, None]).cpu()
            amax = want.abs().amax(dim=1)
            err = float(((back - want).abs().amax(dim=1) / amax).max())
            print(f"[split_h2 8 GiB] worst row error / row maximum {err:.3e} (bar 2^-22 = {2.0 ** -22:.3e})")
            assert err < 2.0 ** -22
            scaled = amax / inv[_idx(sample)].cpu().double()
            assert bool(((scaled >= 2.0 ** 14) & (scaled < 2.0 ** 15)).all())
            del inv
        else:
            _ok(lib, lib.anyloc_split_x3(ptr(x), K, rows, K, ptr(img), stream), "split_x3")
            p = _plane_rows(img, dtype, planes, rows, K, sample)
            assert torch.equal((p[0] + p[1] + p[2]).cpu(), want)
            print("[split_x3 8 GiB] sampled rows rebuilt exactly")
        # every 32-byte piece of the image was written: no fp16 / bf16 NaN pattern (0xFFFF) is left in it
        for b0 in range(0, nbytes, 1 << 31):
            assert not bool((img[b0:b0 + (1 << 31)].view(torch.int16) == -1).any()), (name, b0)
        del img, p
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- top-k
def _topk(q, db, k, index_base):
    from anyloc_amd import _lib
    lib, ptr, stream = _lib_and_ptrs()
    nq, dim = q.shape
    ndb = db.shape[0]
    dist, idx = fresh((nq, k)), fresh((nq, k), torch.int64)
    ws = _lib.workspace(lib.anyloc_topk_workspace_bytes(nq, ndb, dim, k), q.device, "topk")
    _ok(lib, lib.anyloc_topk(ptr(q), nq, ptr(db), ndb, dim, k, 0, 0, index_base, ptr(dist), ptr(idx), ptr(ws), ws.numel(), stream), "topk")
    return dist, idx


@pytest.mark.parametrize("path,nq,opts", [(1, 5, dict(topk_fewq_x6=2)), (1, 5, dict(topk_fewq_x6=1)), (1, 5, dict(topk_fewq_x6=0)),
                                          (0, 70, dict(topk_h3=0, topk_screen=0))],
                         ids=["few-queries-fp16", "few-queries-bf16", "few-queries-fp32", "fp32-panels"])
def test_topk_database_past_4_gib_with_a_64_bit_index_base(path, nq, opts):
    """262 400 rows of 4096 columns: rows 131 072 and 262 144 start exactly on byte 2^31 and 2^32.  Every query's best rows are
    planted there, one row behind, and at both ends of the database; the rest scores ~1e-3.  Lists against float64 scores of
    the whole database on the device: the planted rows lead every list in order, a differing index elsewhere only inside
    the swap gap, every distance the true score of the row it names.  index_base = 2^33 + 5: the indices are int64 sums."""
    from anyloc_amd import ops
    _room("topk_4g")
    lib, ptr, stream = _lib_and_ptrs()
    c = BC.CASES["topk_4g"]
    ndb, dim, planted, k, base = c["rows"], c["cols"], c["planted"], 16, (1 << 33) + 5
    db = BC.case_fill("topk_4g", DEV)
    q = torch.nn.functional.normalize(BC.rows_f64(list(range(nq)), dim, "unit", c["seed"] + 1), dim=-1).float().to(DEV)
    for j, row in enumerate(planted):                      # planted row j copies query j % nq, scaled 1, 0.97, 0.94, ...
        db[row] = q[j % nq] * (1.0 - 0.03 * j)
    with ops.options(**opts):
        assert lib.anyloc_topk_path(nq, ndb, dim) == path
        dist, idx = _topk(q, db, k, base)
    scores = torch.empty(nq, ndb, dtype=torch.float64, device=DEV)
    for r0 in range(0, ndb, 32768):
        scores[:, r0:r0 + 32768] = q.double() @ db[r0:r0 + 32768].double().T
    d_ref, i_ref = scores.topk(k, dim=1)
    assert bool((idx >= base).all()) and bool((idx < base + ndb).all())
    got = idx - base
    for qi in range(nq):
        own = [row for j, row in enumerate(planted) if j % nq == qi]
        assert got[qi, :len(own)].tolist() == own == i_ref[qi, :len(own)].tolist(), (qi, got[qi].tolist())
    true = scores.gather(1, got)
    assert float((dist.double() - true).abs().max()) < VT.TOPK_DIST_ATOL
    differ = got != i_ref
    assert not bool(differ.any()) or float((d_ref - true)[differ].abs().max()) < VT.TOPK_SWAP_GAP
    print(f"[topk 4 GiB, path {path}, {opts}] largest distance error {float((dist.double() - true).abs().max()):.3e} (bar {VT.TOPK_DIST_ATOL:.0e}), "
          f"{int(differ.sum())} indices inside the swap gap")


# --------------------------------------------------------------------------------------------------------------- ingest
def _sampled_units(case, rows_per_unit, n_units):
    """images / planes to compare: both ends, those around every boundary of the output, 16 seeded ones"""
    c = BC.CASES[case]
    units = {0, 1, n_units - 2, n_units - 1} | {b // rows_per_unit + d for b in BC.case_boundary_rows(case) for d in (-1, 0, 1)}
    units |= set(torch.randint(0, n_units, (16,), generator=torch.Generator().manual_seed(c["seed"])).tolist())
    return sorted(u for u in units if 0 <= u < n_units)


def test_preprocess_u8_output_past_2g_elements():
    """2731 images of 520 x 520 -> [2731, 3, 518, 518]: the output crosses 2^31 bytes, 2^32 bytes and 2^31 elements, the uint8
    input 2^31 bytes.  Sampled images bit-exact against ToTensor + Normalize + CenterCrop (tests/test_gpu_kernels.py)."""
    from anyloc_amd import synth
    _room("ingest_8g")
    lib, ptr, stream = _lib_and_ptrs()
    c = BC.CASES["ingest_8g"]
    B, hw, crop = c["batch"], c["hw"], c["crop"]
    u8 = BC.fill(B * hw, hw * 3, "bytes", c["seed"], DEV, dtype=torch.uint8)
    assert u8.numel() > BC.B31
    out = fresh((B, 3, crop, crop))
    mean, std = (C.c_float * 3)(*synth.IMAGENET_MEAN), (C.c_float * 3)(*synth.IMAGENET_STD)
    _ok(lib, lib.anyloc_preprocess_u8(ptr(u8), B, hw, hw, crop, crop, mean, std, ptr(out), stream), "preprocess_u8")
    assert written(out)
    images = _sampled_units("ingest_8g", 3 * crop, B) + [BC.B31 // (hw * hw * 3)]      # (and the image holding input byte 2^31)
    for i in sorted(set(images)):
        rows = list(range(i * hw, (i + 1) * hw))
        img = BC.rows_f64(rows, hw * 3, "bytes", c["seed"]).to(torch.uint8).reshape(1, hw, hw, 3)
        assert torch.equal(out[i].cpu(), TK.totensor_normalize_centercrop(img)[0]), i
    print(f"[preprocess_u8 8 GiB] {len(set(images))} images bit-exact")


def test_resize_bicubic_output_past_2g_elements():
    """8300 planes of 64 x 64 upscaled to 512 x 508: the output crosses 2^31 bytes, 2^32 bytes and 2^31 elements"""
    _room("resize_8g")
    lib, ptr, stream = _lib_and_ptrs()
    c = BC.CASES["resize_8g"]
    P, hw, (oh, ow) = c["planes"], c["hw"], c["out_hw"]
    x = BC.fill(P * hw, hw, "unit", c["seed"], DEV)
    out = fresh((P, oh, ow))
    _ok(lib, lib.anyloc_resize_bicubic(ptr(x), P, hw, hw, oh, ow, 0, 0, oh, ow, ptr(out), stream), "resize_bicubic")
    assert written(out)
    planes = _sampled_units("resize_8g", oh, P)
    src = torch.stack([BC.rows_f64(list(range(p * hw, (p + 1) * hw)), hw, "unit", c["seed"]).float() for p in planes])
    ref = torch.nn.functional.interpolate(src[None], size=(oh, ow), mode="bicubic", align_corners=False)[0]
    err = float((out[_idx(planes)].cpu() - ref).abs().max())
    print(f"[resize_bicubic 8 GiB] largest error over {len(planes)} planes {err:.3e} (bar {TK.RESIZE_ATOL:.0e})")
    assert err < TK.RESIZE_ATOL


# -------------------------------------------------------------------------------- soft VLAD, given assignments (8 GiB)
def _batch_of_ordinary_images(case, around=(-2, -1, 0, 1, 2)):
    """the rows of a token case as images of n_tok tokens -> (n_img, host offsets, images to compare: both ends and two on either
    side of every boundary)"""
    c = BC.CASES[case]
    total, n_tok = c["rows"], c["n_tok"]
    n_img = -(-total // n_tok)
    off_h = [min(i * n_tok, total) for i in range(n_img + 1)]
    images = {0, 1, n_img - 2, n_img - 1} | {b // n_tok + d for b in BC.case_boundary_rows(case) for d in around}
    return n_img, off_h, sorted(i for i in images if 0 <= i < n_img)


def test_vlad_soft_batch_past_2g_elements():
    """anyloc_vlad_soft over 4086 ordinary images, 2^31 + 36 352 token elements, against 8 of the 32 base directions as centres
    (the oracle forms [N, K, D] per image): both ends and the images on either side of every boundary against the oracle and
    float64 by the yardstick of tests/test_gpu_vlad_soft.py; every image of unit norm."""
    from anyloc_amd import ops
    _room("tokens_8g")
    c = BC.CASES["tokens_8g"]
    D, K, temp = c["cols"], 8, VS.TEMPS[1]
    x = BC.case_fill("tokens_8g", DEV)
    centers = BC.token_centers(D, c["seed"])[:K].contiguous()
    n_img, off_h, images = _batch_of_ordinary_images("tokens_8g", around=(0, 1))
    offsets = torch.tensor(off_h, dtype=torch.int64, device=DEV)
    out = ops.vlad((x, offsets), centers.to(DEV), mode="soft", soft_temp=temp, out=fresh((n_img, K * D)))
    assert written(out) and float((out.norm(dim=1) - 1.0).abs().max()) < 1e-5
    for i in images:
        xi = BC.case_rows_f64("tokens_8g", list(range(off_h[i], off_h[i + 1]))).float()
        v32 = vlad_ref.vlad_soft(xi, centers, temp)[0]
        v64 = VS._soft_f64(xi, centers, VS._weights_f64(xi, centers, temp))
        VS._judge(out[i], v32, v64, f"soft 8 GiB, image {i}")


def test_vlad_soft_weights_past_2g_elements():
    """anyloc_vlad_soft_weights of 5 592 500 tokens x 384: sampled rows as close to the float64 soft-max as the oracle's"""
    from anyloc_amd import _lib
    _room("tokens_8g")
    lib, ptr, stream = _lib_and_ptrs()
    c = BC.CASES["tokens_8g"]
    n, D, K, temp = c["rows"], c["cols"], BC.MODES, VS.TEMPS[1]
    x = BC.case_fill("tokens_8g", DEV)
    centers = BC.token_centers(D, c["seed"])
    c_d = centers.to(DEV)
    w = fresh((n, K))
    ws = _lib.workspace(lib.anyloc_vlad_workspace_bytes(n, 1, D, K), x.device, "vlad")
    _ok(lib, lib.anyloc_vlad_soft_weights(ptr(x), n, D, ptr(c_d), K, temp, ptr(w), ptr(ws), ws.numel(), stream), "vlad_soft_weights")
    assert written(w) and float((w.double().sum(dim=1) - 1.0).abs().max()) <= 1e-6
    sample = BC.case_sample("tokens_8g")
    xs = BC.case_rows_f64("tokens_8g", sample).float()
    w32 = vlad_ref.vlad_soft(xs, centers, temp)[1]
    w64 = VS._weights_f64(xs, centers, temp)
    e_or, e_k = float((w32.double() - w64).abs().max()), float((w[_idx(sample)].cpu().double() - w64).abs().max())
    print(f"[soft weights 8 GiB] largest error to float64: kernel {e_k:.3e} oracle {e_or:.3e}")
    assert e_k <= 3.0 * e_or + 1e-6


def test_vlad_assigned_one_image_past_2g_elements():
    """anyloc_vlad_assigned: ONE image of 5 592 500 tokens under given labels (each row's own base direction), raw tokens:
    residuals on the 1 / 32 lattice, sums exact in fp32.  Against float64 on the device."""
    from anyloc_amd import _lib, ops
    _room("tokens_8g")
    lib, ptr, stream = _lib_and_ptrs()
    c = BC.CASES["tokens_8g"]
    n, D, K = c["rows"], c["cols"], BC.MODES
    x = BC.case_fill("tokens_8g", DEV)
    centers = BC.token_centers(D, c["seed"]).to(DEV)
    labels = BC.mode_of(torch.arange(n, device=DEV))
    out = fresh((K * D,))
    ws = _lib.workspace(lib.anyloc_vlad_workspace_bytes(n, 1, D, K), x.device, "vlad")
    _ok(lib, lib.anyloc_vlad_assigned(ptr(x), n, D, ptr(centers), K, ptr(labels), None, ops.VLAD_INTRA_NORM, ptr(out), ptr(ws), ws.numel(),
                                      stream), "vlad_assigned")
    err = VR.l2rel(out, VR.hard_vlad_f64(x, centers, labels, False, slab=1 << 18))
    print(f"[vlad_assigned, one image of 8 GiB] l2rel {err:.3e} (bar {VT.VLAD_RTOL:.0e})")
    assert err < VT.VLAD_RTOL


# --------------------------------------------------------------------------------------------- two-term / split GEMMs
def _planes_gemm(kind, a, w, M, N, K):
    """anyloc_gemm_nt_h3 / _x6 from the images of a and w into a fresh C"""
    from anyloc_amd import ops
    lib, ptr, stream = _lib_and_ptrs()
    out = fresh((M, N))
    if kind == "h3":
        (ai, av), (wi, wv) = ops.split_h2(a), ops.split_h2(w)
        assert ai.numel() == lib.anyloc_h2_bytes(M, K)
        _ok(lib, lib.anyloc_gemm_nt_h3(ptr(ai), ptr(av), ptr(wi), ptr(wv), None, ptr(out), N, M, N, K, stream), "gemm_nt_h3")
    else:
        ai, wi = ops.split_x3(a), ops.split_x3(w)
        assert ai.numel() == lib.anyloc_x3_bytes(M, K)
        _ok(lib, lib.anyloc_gemm_nt_x6(ptr(ai), ptr(wi), None, ptr(out), N, M, N, K, stream), "gemm_nt_x6")
    return out, ai.numel()


@pytest.mark.parametrize("kind,case", [("h3", "gemm_h3_image"), ("x6", "gemm_x6_image"), ("h3", "gemm_planes_c_8g"), ("x6", "gemm_planes_c_8g")])
def test_gemm_nt_h3_x6_largest_image_and_c_past_2g_elements(kind, case):
    """The most rows an A image holds below 2 GiB at K = 1024 (524 287 two-plane, 349 525 three-plane rows: one more is refused,
    tests/test_addressing_limits_cpu.py) with its last rows sampled, and C [2 097 400, 1024] past 2^31 elements from K = 64.
    Sampled rows by the yardstick of tests/test_gpu_x6.py: error / (|a| |w|^T), no worse than the fp32-MFMA kernel."""
    from anyloc_amd import ops
    _room(case)
    c = BC.CASES[case]
    M, K, N = c["rows"], c["cols"], c["N"]
    a = BC.case_fill(case, DEV)
    w64 = BC.rows_f64(list(range(N)), K, "unit", c["seed"] + 50, 0.05)
    w = w64.float().to(DEV)
    out, nbytes = _planes_gemm(kind, a, w, M, N, K)
    assert written(out)
    if "image" in case:
        assert nbytes < BC.B31 <= nbytes // M * (M + 1)
    sample = BC.case_sample(case)
    a64 = BC.case_rows_f64(case, sample)
    ref, mag = a64 @ w64.T, a64.abs() @ w64.abs().T
    err = float(((out[_idx(sample)].cpu().double() - ref).abs() / mag).max())
    e32 = float(((ops.gemm_nt(a[_idx(sample)], w).cpu().double() - ref).abs() / mag).max())
    print(f"[gemm_nt_{kind} {case}] error / |a||w| {err:.3e}, the fp32-MFMA kernel on the same rows {e32:.3e}")
    X6.no_worse_than_fp32(err, e32)
    if kind == "x6":
        assert err < X6.GEMM_X6_REL


# ------------------------------------------------------------------------------------------------- float64 products
def _centred_product_f64(x, mean, side, slab=64):
    """Xc Xc^T (side 0) or Xc^T Xc (side 1) in torch float64 on the device, in slabs along the long index"""
    n, f = x.shape
    m = n if side == 0 else f
    out = torch.zeros(m, m, dtype=torch.float64, device=x.device)
    if side == 0:
        for c0 in range(0, f, 1 << 16):
            xs = x[:, c0:c0 + (1 << 16)].double() - mean[c0:c0 + (1 << 16)]
            out += xs @ xs.T
    else:
        for r0 in range(0, n, 1 << 16):
            xs = x[r0:r0 + (1 << 16)].double() - mean
            out += xs.T @ xs
    return out


def test_pca_products_past_2g_elements():
    """X [2056, 1 048 700] fp32 (2^31 + 8.6 M elements) and the same memory as [1 048 700, 2056]: the Gram matrix of the first
    (contraction over the very long rows) and the scatter matrix of the second (contraction over a million samples), and the
    back-projection U^T Xc of both, against torch float64 on the device under the bar of tests/test_gpu_pca.py."""
    from anyloc_amd import ops
    _room("pca_8g")
    c = BC.CASES["pca_8g"]
    n, f = c["rows"], c["cols"]
    x = BC.case_fill("pca_8g", DEV)
    x.mul_(3.0).add_(40.0)                                  # a large common offset: centring must be in float64
    g = torch.Generator().manual_seed(c["seed"])
    for xv, side in ((x, 0), (x.view(f, n), 1)):
        rows, cols = xv.shape
        mean = torch.zeros(cols, dtype=torch.float64, device=DEV)
        for r0 in range(0, rows, 1 << 16):
            mean += xv[r0:r0 + (1 << 16)].sum(dim=0, dtype=torch.float64)
        mean /= rows
        got = ops.pca_gram_f64(xv, mean, side)
        want = _centred_product_f64(xv, mean, side)
        err, bar = float((got - want).abs().max()), TPCA.f64_product_bar(float(want.abs().max()), max(rows, cols))
        print(f"[pca_gram_f64 side {side}, X {rows} x {cols}] largest error {err:.3e} (bar {bar:.3e})")
        assert got.shape == (n, n) and torch.equal(got, got.t()) and err <= bar
        k = 4
        vec = torch.linalg.qr(torch.randn(rows, k, generator=g, dtype=torch.float64))[0].to(DEV)
        got = ops.pca_axes_f64(vec, k, xv, mean)
        want = torch.zeros(k, cols, dtype=torch.float64, device=DEV)
        for r0 in range(0, rows, 1 << 16):
            want += vec[r0:r0 + (1 << 16)].T @ (xv[r0:r0 + (1 << 16)].double() - mean)
        err, bar = float((got - want).abs().max()), TPCA.f64_product_bar(float(want.abs().max() + 1), rows)
        print(f"[pca_axes_f64, X {rows} x {cols}] largest error {err:.3e} (bar {bar:.3e})")
        assert got.shape == (k, cols) and err <= bar


def test_gemm_nt_f64_operand_past_2g_elements():
    """A [2056, 1 048 700] float64 (16 GiB) times B [8, 1 048 700]^T, row-major and as the transpose of the [1 048 700, 2056]
    view of the same memory (strides 1 and 2056)"""
    from anyloc_amd import ops
    _room("f64_16g")
    c = BC.CASES["f64_16g"]
    M, K = c["rows"], c["cols"]
    a = torch.empty(M, K, dtype=torch.float64, device=DEV)
    cols = torch.arange(K, device=DEV)
    for r0 in range(0, M, 16):
        a[r0:r0 + 16] = BC.unit(torch.arange(r0, min(M, r0 + 16), device=DEV), cols, c["seed"])
    b = BC.unit(torch.arange(8, device=DEV), cols, c["seed"] + 1)
    for tag, av, bv in (("row-major", a, b), ("transposed view", a.view(K, M).t(), b)):
        kk = av.shape[1]
        want = torch.zeros(av.shape[0], 8, dtype=torch.float64, device=DEV)
        for c0 in range(0, kk, 1 << 16):
            want += av[:, c0:c0 + (1 << 16)] @ bv[:, c0:c0 + (1 << 16)].T
        got = ops.gemm_nt_f64(av, bv)
        err, bar = float((got - want).abs().max()), TPCA.f64_product_bar(float(want.abs().max()), kk)
        print(f"[gemm_nt_f64 {tag}, A {tuple(av.shape)}] largest error {err:.3e} (bar {bar:.3e})")
        assert err <= bar
