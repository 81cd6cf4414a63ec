"""The ends of the documented argument ranges (include/anyloc_hip.h), where other code runs than in the middle:

* top-k lists of 1022 / 1023 / 1024 entries on every scoring path -- 1023 and 1024 ask for 65 552 bytes of dynamic LDS, 16
  more than a launch gets without hipFuncSetAttribute; rank_entries<4> sorts ~3 300 keys; a list longer than the 256 seed
  columns starts with 768 entries of (-inf, -1) -- the largest k the screened search serves and the next, and databases one
  row short of, at and one row past the panel height of the fp32 and of the fp16 panels;
* k-means and hard VLAD on both sides of K = 128 (accumulate_kernel: full-width | half-width column slices, one | two
  passes of the label histogram) and at K = 255 / 256 (the largest LDS request, knorm[256]), and at the first K the fused
  kernel does not serve;
* 65 538 images in one VLAD call (two launches of the 65 535-image grid) and 65 535 -- the most one call takes -- in
  pooling, both attention entry points and the uint8 ingest.

The references and bars are those of the tests that cover the middle of the same ranges; they are imported from there.
The far side of each limit is tests/test_limits_cpu.py."""
import functools
import time

import pytest
import torch

import _limits_cases as LC
import _retrieval_refs as R
import _vlad_refs as VR
import test_gpu_kernels as TK
import test_gpu_pooling as TP
import test_gpu_vlad_soft as VS
import test_gpu_vlad_topk as VT
from oracle import pool_ref, vlad_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
KS = (1022, 1023, 1024)          # 65 496 bytes of dynamic LDS (under the default limit), then 65 552 twice
METRICS = ("ip", "l2")


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    print(f"\n[limits] wall time of the module: {time.time() - t0:.1f} s")


# ------------------------------------------------------------------------------------------------------------- 1. top-k
@functools.lru_cache(maxsize=2)
def _search_inputs(nq, ndb, dim):
    """the recipe of test_topk_normalize_db_vs_oracle -> (queries, raw rows, F.normalize(rows)), on the CPU"""
    qu, db = VT.normalized_search_data(nq, ndb, dim)
    return qu, db, torch.nn.functional.normalize(db)


def _search(qu, db, dbn, k, metric, normalize_db):
    """the search of F.normalize(db): by the flag on the raw rows, or on the rows normalised beforehand"""
    from anyloc_amd import ops
    d, i = ops.topk(qu.to(DEV), (db if normalize_db else dbn).to(DEV), k, metric, normalize_db=normalize_db)
    return d.cpu(), i.cpu()


@pytest.mark.parametrize("fewq_x6", [2, 1, 0], ids=["fp16-planes", "bf16-planes", "fp32-mfma"])
@pytest.mark.parametrize("normalize_db", [True, False], ids=["raw-rows", "unit-rows"])
def test_topk_longest_lists_few_queries(normalize_db, fewq_x6):
    """5 queries of 4096 columns: the database is the M operand of a split-K launch, in each of its three arithmetics."""
    from anyloc_amd import _lib, ops
    nq, ndb, dim = 5, 3000, 4096
    qu, db, dbn = _search_inputs(nq, ndb, dim)
    with ops.options(topk_fewq_x6=fewq_x6):
        assert _lib.load().anyloc_topk_path(nq, ndb, dim) == 1
        for k in KS:
            for metric in METRICS:
                d, i = _search(qu, db, dbn, k, metric, normalize_db)
                VT.check_normalized_search(d, i, qu, db, k, metric)


@pytest.mark.parametrize("metric", METRICS)
def test_topk_longest_lists_fp16_panels_and_prepared_index(metric):
    """70 queries against 8193 rows under topk_h3 = 1: two fp16 panels, the second one row long.  The prepared index of the
    same rows gives the one-shot call's lists bit for bit (include/anyloc_hip.h, anyloc_topk_search_index)."""
    from anyloc_amd import _lib, ops
    nq, ndb, dim = 70, 8193, 256
    qu, db, _ = _search_inputs(nq, ndb, dim)
    with ops.options(topk_h3=1, topk_screen=0):
        assert _lib.load().anyloc_topk_path(nq, ndb, dim) == 2
        index = ops.topk_index_build(db.to(DEV))
        for k in KS:
            d, i = ops.topk(qu.to(DEV), db.to(DEV), k, metric, normalize_db=True)
            VT.check_normalized_search(d.cpu(), i.cpu(), qu, db, k, metric)
            d_x, i_x = ops.topk_indexed(qu.to(DEV), index, ndb, k, metric, normalize_db=True)
            assert torch.equal(d_x, d) and torch.equal(i_x, i), (k, metric, "prepared index differs from the one-shot call")


@pytest.mark.parametrize("metric", METRICS)
def test_topk_fewer_rows_than_the_longest_list(metric):
    """1000 rows, k = 1024: the 24 entries behind the last row are faiss' padding -- index -1, distance -inf / +inf."""
    from anyloc_amd import ops
    nq, ndb, dim, k = 9, 1000, 64, 1024
    qu, db, dbn = _search_inputs(nq, ndb, dim)
    d, i = _search(qu, db, dbn, k, metric, True)
    VT.check_normalized_search(d, i, qu, db, k, metric)
    d_ref, i_ref = VT.faiss_flat.flat_search(qu, dbn, k, metric)
    assert bool((i[:, ndb:] == -1).all()) and torch.equal(i[:, ndb:], i_ref[:, ndb:])
    assert torch.equal(d[:, ndb:], d_ref[:, ndb:])
    assert bool((i[:, :ndb] >= 0).all()) and all(len(set(r.tolist())) == ndb for r in i[:, :ndb])      # every row exactly once


@pytest.mark.parametrize("k,screens", [(128, True), (129, False)])
def test_topk_screened_search_ends_at_128(k, screens):
    """topk_screen = 1 serves k <= 128: at 128 the leading-plane GEMM runs and the exact one does not, at 129 the reverse;
    both give the float64 lists (the rules of tests/test_gpu_screen.py)."""
    from anyloc_amd import ops
    nq, ndb, dim = 130, 9000, 2048
    qu, db = R.planted_rows(nq, ndb, dim, nq + ndb + dim)
    with ops.options(topk_screen=1, topk_h3=1):
        (d, i), prof = R.profiled(lambda: ops.topk(qu, db, k, "ip", normalize_db=True))
    assert ("topk_screen_gemm" in prof) == screens and ("topk_scores_gemm" in prof) == (not screens), sorted(prof)
    R.check_search(d, i, qu, db, k, "ip", f"k={k}")


@pytest.mark.parametrize("order", ["constant", "ascending"])
@pytest.mark.parametrize("ndb", [32767, 32768, 32769])
def test_topk_fp32_panel_height(order, ndb):
    """One row short of a 32 768-row panel, exactly one panel, one row into the second: the lists of the flat search, ties to
    the lower index ("constant": every list is 0 .. 19; "ascending": the last rows, the candidate buffer full at every step)."""
    VT.check_adversarial_order(order, 20, ndb, 8, (1.0, 2.0, -1.0))


@pytest.mark.parametrize("order", ["constant", "ascending"])
@pytest.mark.parametrize("ndb", [8191, 8192, 8193])
def test_topk_fp16_panel_height(order, ndb):
    """The same at the 8192-row panels of the two-term fp16 GEMM (70 queries, topk_h3 = 1).  The queries are +-2^-j multiples
    of the first axis (exact in the fp16 planes); a database score keeps 22 of its 24 bits there, an error of 2^-22 of a
    score <= 1, against steps of 1 / 8192 between the scores of "ascending": the same lists, within the same 1e-6."""
    from anyloc_amd import _lib, ops
    scales = tuple((-1.0) ** q * 2.0 ** -(q % 4) for q in range(70))
    with ops.options(topk_h3=1):
        assert _lib.load().anyloc_topk_path(70, ndb, 64) == 2
        VT.check_adversarial_order(order, 20, ndb, 64, scales)


# ------------------------------------------------------------------------------------------- 2. K above 32, up to 256
@pytest.mark.parametrize("K,D,n,mode", LC.KMEANS_CASES)
def test_kmeans_step_large_k(K, D, n, mode):
    """One step on the two-pass path (tests/_limits_cases.py) against the fast-pytorch-kmeans rule: labels (at most
    LABEL_TIE_CAP excused as oracle near-ties -- tests/test_limits_cpu.py shows the inputs have none to speak of), counts
    equal to the one-hot counts of those labels, sums within 1e-6 of their float64 sums; some cluster stays empty."""
    from anyloc_amd import ops
    x, c = LC.kmeans_case(K, D, n)
    sums, counts, lab = ops.kmeans_step(x.to(DEV), c.to(DEV), mode, True)
    excused, err = VT.check_kmeans_step(x, c, mode, sums, counts, lab)
    print(f"[kmeans K={K} D={D} {mode}] sums l2rel {err:.3e} (bar 1e-6), {excused} labels excused")
    assert excused <= LC.LABEL_TIE_CAP
    assert bool((counts == 0).any()) and float(sums[counts == 0].abs().max()) == 0.0
    assert float(counts.sum()) == n


def test_kmeans_update_256_clusters():
    """K = 256, D = 1536 (393 216 quotients, 384 per thread of the one workgroup) with three empty clusters."""
    VS.check_kmeans_update(256, 1536, 4000, [0, 129, 255])


@pytest.mark.parametrize("K,D,N", [(K, D, 700) for K in (129, 255, 256) for D in (64, 260)] + [(33, 384, 300)])
def test_vlad_hard_large_k(K, D, N):
    """Three images, the middle one empty, every flag pair of test_vlad_hard_vs_oracle_flags_and_ragged: K = 129 is the
    first on half-width column slices, D = 260 leaves live columns in the last slice at both widths, 255 / 256 fill knorm."""
    from anyloc_amd import ops
    g = torch.Generator().manual_seed(K * D + N)
    x = synth_tokens(3, N, D, K, K + N) * (0.5 + torch.rand(3, N, 1, generator=g))
    centers = 0.7 * synth_tokens(1, K, D, K, K + N)[0] + 0.01 * torch.randn(K, D, generator=g)
    packed = torch.cat([x[0], x[2]]).to(DEV)
    offsets = torch.tensor([0, N, N, 2 * N], dtype=torch.int64, device=DEV)
    worst = 0.0
    for norm_descs, intra in VT.VLAD_FLAG_PAIRS:
        out, lab = ops.vlad((packed, offsets), centers.to(DEV), norm_descs=norm_descs, intra_norm=intra, return_labels=True)
        assert tuple(out.shape) == (3, K * D) and float(out[1].abs().max()) == 0.0
        for row, img in ((0, 0), (2, 2)):
            lab_i = lab[:N] if row == 0 else lab[N:]
            worst = max(worst, VT.check_vlad_hard_image(out[row], lab_i, x[img], centers, norm_descs, intra))
    print(f"[vlad hard K={K} D={D}] worst l2rel {worst:.3e} (bar {VT.VLAD_RTOL:.0e})")


def synth_tokens(n_img, n_tok, dim, n_modes, seed):
    from anyloc_amd import synth
    return synth.clustered_tokens(n_img, n_tok, dim, n_modes=n_modes, seed=seed)


# ------------------------------------------------------------- 3. more images than one 16-bit grid dimension holds
N_IMG = 65538                                          # 65 535 in the first launch of accumulate_kernel, 3 in the second
WINDOWS = ((0, 10), (65530, 65538))                    # the images checked one by one: the second run straddles 65 535


def _ragged_batch(D, seed):
    """image i has i % 3 tokens (empty images on both sides of the group boundary) -> (packed [total, D], offsets), CPU"""
    counts = torch.arange(N_IMG) % 3
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])
    g = torch.Generator().manual_seed(seed)
    packed = torch.randn(int(offsets[-1]), D, generator=g) * (0.5 + torch.rand(int(offsets[-1]), 1, generator=g))
    return packed, offsets, counts


@pytest.mark.parametrize("mode,D,K", [("hard", 8, 3), ("soft", 8, 3), ("hard", 384, 4)], ids=["hard-two-pass", "soft", "hard-fused"])
def test_vlad_65538_images(mode, D, K):
    """A wrong base in the second image group (offsets + i0, out + i0 * K * D) writes a plausible descriptor into the
    wrong row: images 65 530 .. 65 537 have 1, 2, 0, 1, 2, 0, 1, 2 tokens, so the row next door is another image's.
    D = 8 is served by the two-pass path (accumulate_kernel / soft_accumulate_kernel: the 65 535-image groups), D = 384 with
    K = 4 by the fused kernel (a 1-D grid of 65 538 workgroups)."""
    from anyloc_amd import ops
    packed, offsets, counts = _ragged_batch(D, 7 * D + K)
    g = torch.Generator().manual_seed(K)
    centers = 0.5 * torch.randn(K, D, generator=g)
    kw = dict(mode=mode, soft_temp=7.5) if mode == "soft" else dict(mode=mode, return_labels=True)
    packed_d, offsets_d, c_d = packed.to(DEV), offsets.to(DEV), centers.to(DEV)
    res = ops.vlad((packed_d, offsets_d), c_d, **kw)
    out, lab = res if mode == "hard" else (res, None)
    assert tuple(out.shape) == (N_IMG, K * D)
    # the whole output: empty images exactly zero, every other one of unit norm (the bar of tests/test_gpu_fullsize_properties.py)
    norms = out.norm(dim=1).cpu()
    assert float(out[(counts == 0).to(DEV)].abs().max()) == 0.0
    assert float((norms[counts > 0] - 1.0).abs().max()) < 1e-5
    worst = 0.0
    for a, b in WINDOWS:
        r0, r1 = int(offsets[a]), int(offsets[b])
        alone = ops.vlad((packed_d[r0:r1], (offsets_d[a:b + 1] - r0)), c_d, **kw)
        alone = alone[0] if mode == "hard" else alone
        for i in range(a, b):
            t0, t1 = int(offsets[i]), int(offsets[i + 1])
            if t0 == t1:
                assert float(out[i].abs().max()) == 0.0 and float(alone[i - a].abs().max()) == 0.0
                continue
            x_i = packed[t0:t1]
            if mode == "hard":
                err = VT.check_vlad_hard_image(out[i], lab[t0:t1], x_i, centers)
            else:
                err = VR.l2rel(out[i], vlad_ref.vlad_soft(x_i, centers, 7.5)[0])
                assert err < VT.VLAD_RTOL, (i, err)
            assert VR.l2rel(out[i], alone[i - a]) < VT.VLAD_RTOL, i
            worst = max(worst, err)
    print(f"[vlad {mode} D={D} K={K}, {N_IMG} images] worst l2rel to the oracle {worst:.3e} (bar {VT.VLAD_RTOL:.0e})")


def test_pool_65535_images():
    """The most images one anyloc_pool_tokens call takes, two tokens of eight features each.  The two tokens of an image have
    magnitudes in [0.5, 1) and [1.25, 1.5) with random signs: both signs of mean(t^3) occur, and no image has
    t0^3 + t1^3 cancel (the cube root of a cancelled sum would amplify the ulps by which powf and torch.pow differ)."""
    from anyloc_amd import ops
    n = 65535
    g = torch.Generator().manual_seed(n)
    mag = torch.stack([0.5 + 0.5 * torch.rand(n, 8, generator=g), 1.25 + 0.25 * torch.rand(n, 8, generator=g)], dim=1)
    x = mag * (2.0 * torch.randint(0, 2, (n, 2, 8), generator=g) - 1.0)
    x_d = x.to(DEV)
    got = ops.pool(x_d, "average").cpu()
    want = pool_ref.global_pool(x, "average")
    err_avg = TP.rel_err(got, want)
    assert tuple(got.shape) == (n, 8) and err_avg < TP.REL, err_avg
    assert torch.equal(ops.pool(x_d, "max").cpu(), pool_ref.global_pool(x, "max"))
    got = ops.pool(x_d, "gem", 3.0).cpu()
    want = pool_ref.gem_descriptors(x, 3)
    err_gem = TP.rel_err(got, want)
    assert err_gem < TP.REL, err_gem
    assert bool((want < 0).any()) and bool((want > 0).any()) and torch.equal(torch.sign(got), torch.sign(want))
    print(f"[pool {n} images] worst row error: average {err_avg:.3e}, gem {err_gem:.3e} (bar {TP.REL:.0e})")


def _qkv_65535(seed, big_values):
    """[65535, 2, 192], one head.  Sixteen images share a 32-row group of the fp16 kernel's operand tiles, which are scaled per
    group: magnitudes vary from GROUP to group (every seventh is small; with ``big_values`` every 250th has values forty
    times the others -- the fp32 kernel's bar is absolute, so not there), never inside one."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(65535, 2, 192, generator=g) * 1.5
    group = torch.arange(65535) // 16
    qkv[group % 7 == 0] *= 0.05
    if big_values:
        qkv[:, :, 128:] *= torch.where(group % 250 == 5, 40.0, 1.0)[:, None, None]
    qkv[3, 0, :64] *= 6.0                                  # a spiky query
    return qkv


def test_attention_65535_images():
    """65 535 images of two tokens: grid.z of the fp32-MFMA kernel at its largest."""
    from anyloc_amd import ops
    qkv = _qkv_65535(1, False)
    out = ops.attention(qkv.to(DEV), 1).cpu()
    print(f"[attention 65535 images] largest error {TK.check_attention(out, qkv, 1):.3e}")


def test_attention_h3_65535_images():
    from anyloc_amd import ops
    qkv = _qkv_65535(2, True)
    img, inv = ops.attention_h3(qkv.to(DEV), 1)
    print(f"[attention_h3 65535 images] largest error {TK.check_attention_h3(img, inv, qkv, 1):.3e}")


def test_preprocess_65535_images():
    """uint8 [65535, 14, 14, 3] -> one patch per image, bit-exact against ToTensor + Normalize (nothing to crop)."""
    from anyloc_amd import preprocess
    u8 = torch.randint(0, 256, (65535, 14, 14, 3), generator=torch.Generator().manual_seed(14), dtype=torch.uint8)
    out = preprocess.images_to_input(u8).cpu()
    ref = TK.totensor_normalize_centercrop(u8)
    assert out.shape == ref.shape == (65535, 3, 14, 14)
    assert torch.equal(out, ref)
