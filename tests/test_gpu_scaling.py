"""Powers of two are exact (``pytest -m gpu``; rule 4 of include/anyloc_hip.h, Conventions, "Non-finite values").  Every unit of
an input times 2^s, s in {-40, -13, 13, 40}, and -- inside ONE call -- every unit times its own power of two in [-40, 40]
(seeded): the output is the base output times the same power, or unchanged for the normalising ops, BIT FOR BIT; for
split_h2 and attention_h3 the fp16 image is byte-identical and only the row scales move.  2^+-40 keeps every sum of squares
at K <= 4096 inside the normal fp32 range, so nothing overflows or goes subnormal and nothing is measured.  A scale taken
per tile where the design says per row shows in the mixed case, which is therefore also held to float64 per row.

Where an op is NOT exact the reason is in its formula, stated at the case and in profiles/nonfinite_audit.md:
  * k-means / VLAD cosine assignment: the centre norm's + 1e-8 (fast-pytorch-kmeans).  Scaled DOWN, the eps is no longer below
    half an ulp of the norm: labels are held to the float64 scores of the formula instead.
  * attention_h3 with batch neighbours of different magnitude: one scale per (head, 32-row group) is the design; a group at an
    image boundary holds rows of two images.  Measured, printed, and held to 22 bits of the group's maximum."""
import pytest
import torch
import torch.nn.functional as F

import _nonfinite_cases as NF
import _retrieval_refs as R
from _attention_refs import attention_f64
from test_gpu_kernels import gemm_nt_bound
from test_gpu_x6 import GEMM_X6_REL, planes_from_image

pytestmark = pytest.mark.gpu
DEV = "cuda"
POWERS = [-40, -13, 13, 40]
CASES = POWERS + ["mixed"]


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
    """a device error after a test ends the session: nothing more is started on a GPU that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU reported an error ({e}): nothing more runs on it in this session", returncode=3)


def factors(n, case, seed=0, lowest=-40):
    """[n] powers of two (fp32, on the device): 2^case for every unit, or a seeded power in [-40, 40] per unit; no exponent
    below ``lowest`` (a normalising op is exact only while the scaled norm stays above its eps)"""
    if case == "mixed":
        e = torch.randint(-40, 41, (n,), generator=torch.Generator().manual_seed(1000 + seed + n))
    else:
        e = torch.full((n,), int(case))
    return torch.ldexp(torch.ones(n), e.clamp_min(lowest)).to(DEV)


def scaled_bits(got, base, f, tag):
    """``got`` == ``base`` * f (f broadcast; exact products of fp32 values and powers of two), bit for bit"""
    want = base * f
    assert bool(torch.isfinite(want).all()) and NF.same_bits(got, want), \
        f"{tag}: {int((NF.bits(got) != NF.bits(want)).sum())} of {got.numel()} outputs are not the base output times the power of two"


# ================================================================================================ GEMMs, splitters ====
M, N, K = 70, 200, 64


def _operands():
    g = torch.Generator().manual_seed(7)
    return (torch.randn(M, K, generator=g) * (0.5 + torch.rand(M, 1, generator=g))).to(DEV), (torch.randn(N, K, generator=g) * 0.2).to(DEV)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("arith", ["f32", "x6", "h3"])
def test_gemm_rows_scale_exactly(arith, case):
    """C = A W^T with the rows of A scaled: the rows of C scale.  x6 / h3 run through their splitters: the three bf16 planes
    scale with the row; the two fp16 planes do not move at all, the row's 2^-e does."""
    from anyloc_amd import ops
    a, w = _operands()
    f = factors(M, case)[:, None]
    a2 = a * f
    if arith == "f32":
        base, got = ops.gemm_nt(a, w), ops.gemm_nt(a2, w)
    elif arith == "x6":
        w3 = ops.split_x3(w)
        i0, i1 = ops.split_x3(a), ops.split_x3(a2)
        p0, p1 = planes_from_image(i0, M, K), planes_from_image(i1, M, K)
        scaled_bits(p1, p0, f[None], f"split_x3 {case}")
        base, got = ops.gemm_nt_x6(i0, w3, M, N, K), ops.gemm_nt_x6(i1, w3, M, N, K)
    else:
        w2 = ops.split_h2(w)
        (i0, v0), (i1, v1) = ops.split_h2(a), ops.split_h2(a2)
        assert torch.equal(i0, i1), f"split_h2 {case}: the fp16 image moved with a power-of-two row scale"
        scaled_bits(v1, v0, f[:, 0], f"split_h2 {case} row scales")
        base, got = ops.gemm_nt_h3((i0, v0), w2, M, N, K), ops.gemm_nt_h3((i1, v1), w2, M, N, K)
    scaled_bits(got, base, f, f"gemm {arith} {case}")
    # ... and against float64 per row, relative to the row's own scale (bars: tests/test_gpu_kernels.py::test_gemm_nt,
    # tests/test_gpu_x6.py::test_gemm_x6_as_accurate_as_fp32 and ::test_gemm_h3_as_accurate_as_fp32's 1.5 x fp32 + 1e-7)
    ref = a2.double() @ w.double().t()
    mag = a2.double().abs() @ w.double().abs().t()
    err = (got.double() - ref).abs()
    bar = GEMM_X6_REL * mag if arith == "x6" else 1.5e-6 * mag if arith == "f32" else 1.5 * (1.5e-6 * mag) + 1e-7 * mag
    assert gemm_nt_bound(0.0) == 1e-6                      # (the absolute term of the fp32 bar: dropped here, the rows are scaled)
    assert bool((err <= bar).all()), (arith, case, float((err / mag).max()))


# ===================================================================================================== attention ====
B, T, HEADS = 3, 40, 2
ATTN = {"fp32-mfma": dict(attn_x6=0), "split-bf16": dict(attn_x6=1), "h3": dict(attn_h3_ks=1), "h3-keys-split-2": dict(attn_h3_ks=2)}


def _qkv():
    g = torch.Generator().manual_seed(40)
    return (torch.randn(B, T, 3 * HEADS * 64, generator=g) * 1.5).to(DEV)


def _scale_v(qkv, f):
    out = qkv.clone()
    out[:, :, 2 * HEADS * 64:] *= f[:, None, None]
    return out


# (the two-term fp16 kernel with a power of its own per image: test_attention_h3_next_to_a_louder_batch_neighbour)
@pytest.mark.parametrize("kernel,case", [(k, c) for k in ATTN for c in CASES if not (k.startswith("h3") and c == "mixed")])
def test_attention_scales_exactly_with_v(kernel, case):
    """softmax(q k^T / 8) v is linear in v.  fp32-MFMA and split-bf16: every image's output times its own power.  The two-term
    fp16 kernel, all images scaled alike: the output image keeps its bytes and the rows' 2^-e move."""
    from anyloc_amd import ops
    D = HEADS * 64
    qkv = _qkv()
    h3 = kernel.startswith("h3")
    f = factors(B, case)
    with ops.options(**ATTN[kernel]):
        if h3:
            (i0, v0), (i1, v1) = ops.attention_h3(qkv, HEADS), ops.attention_h3(_scale_v(qkv, f), HEADS)
            assert torch.equal(i0, i1), f"attention_h3 {case}: the output image moved with a power-of-two scale of v"
            scaled_bits(v1, v0, f.repeat_interleave(T), f"attention_h3 {case} row scales")
        else:
            scaled_bits(ops.attention(_scale_v(qkv, f), HEADS), ops.attention(qkv, HEADS), f[:, None, None], f"attention {kernel} {case}")


def test_attention_h3_next_to_a_louder_batch_neighbour():
    """Image 1's v is 2^12 larger than its neighbours'.  Images 0 and 2 share a 32-row group with it (T = 40), and a group has
    ONE scale: their rows in the shared groups keep 22 bits of the GROUP's largest |v|, not of their own.  Measured and
    printed; held to the bar of tests/test_gpu_kernels.py::test_attention_h3 with the largest |v| of the groups the image
    reads in place of the image's own (3e-6 gmax + 2e-6).  Image 1 itself keeps its own bar."""
    from anyloc_amd import ops
    D = HEADS * 64
    qkv = _scale_v(_qkv(), torch.tensor([1.0, 4096.0, 1.0], device=DEV))
    img, inv = ops.attention_h3(qkv, HEADS)
    out = ops.h2_image_to_f32(img, inv, B * T, D).reshape(B, T, D)
    ref = attention_f64(qkv, HEADS)
    v = qkv[:, :, 2 * D:].reshape(B * T, D).abs().amax(dim=1)
    for b in range(B):
        g0, g1 = (b * T) // 32, ((b + 1) * T - 1) // 32
        gmax = float(v[g0 * 32:min((g1 + 1) * 32, B * T)].max())
        own = float(v[b * T:(b + 1) * T].max())
        err = float((out[b] - ref[b]).abs().max())
        print(f"attention_h3, neighbour 2^12 louder: image {b} error {err:.3e}; bar on its own |v| {3e-6 * own + 2e-6:.3e}, on its groups' {3e-6 * gmax + 2e-6:.3e}")
        assert err <= 3e-6 * gmax + 2e-6, (b, err, gmax)


# ===================================================================================== l2norm, pooling, VLAD, k-means ====
@pytest.mark.parametrize("case", CASES)
def test_l2norm_rows_and_pooling_scale_exactly(case):
    from anyloc_amd import ops
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(M, K, generator=g) * 2).to(DEV)
    f = factors(M, case)
    assert NF.same_bits(ops.l2norm_rows(x * f[:, None]), ops.l2norm_rows(x)), f"l2norm_rows {case}: a normalised row moved"
    tok = F.normalize(torch.randn(3, 40, 100, generator=g), dim=-1).to(DEV)
    fi = factors(3, case, seed=1)
    for method in ("average", "max"):
        scaled_bits(ops.pool(tok * fi[:, None, None], method), ops.pool(tok, method), fi[:, None], f"pool {method} {case}")


VLAD_PATHS = {"fused": (384, dict(), 0), "fused-parts-2": (384, dict(), 2), "two-pass": (384, dict(vlad_two_pass=1), 0)}


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("path", list(VLAD_PATHS))
def test_vlad_hard_with_norm_descs_ignores_the_tokens_scale(path, case):
    """F.normalize in front of the residuals: a token times a power of two (each token its own in the mixed case) has the same
    label and the same unit row, so the descriptors keep their bits -- through the fp16 screening of the one-pass kernel as
    well (a loud or faint row goes to its exact path; the label is the exact fp32 arg-max either way)."""
    from anyloc_amd import ops
    D, opts, parts = VLAD_PATHS[path]
    g = torch.Generator().manual_seed(D)
    tokens = torch.randn(3, 40, D, generator=g).to(DEV)
    centers = (0.8 * F.normalize(torch.randn(8, D, generator=g), dim=-1)).to(DEV)
    f = factors(120, case).reshape(3, 40, 1)
    with ops.options(**opts):
        base, lab0 = ops.vlad(tokens, centers, "hard", return_labels=True, parts=parts)
        got, lab1 = ops.vlad(tokens * f, centers, "hard", return_labels=True, parts=parts)
    assert torch.equal(lab0, lab1), f"vlad {path} {case}: {int((lab0 != lab1).sum())} labels moved"
    assert NF.same_bits(got, base), f"vlad {path} {case}: {int((NF.bits(got) != NF.bits(base)).sum())} descriptor values moved"


@pytest.mark.parametrize("case", POWERS)
@pytest.mark.parametrize("K_", [5, 200])
@pytest.mark.parametrize("mode", ["cosine", "euclidean"])
def test_kmeans_step_scales_exactly_with_rows_and_centres(mode, K_, case):
    """x and the centres times 2^s: euclidean scores scale by 2^2s, cosine scores by 2^s -- same labels, same counts, sums times
    2^s.  Cosine with s < 0 is the exception: c / (||c|| + 1e-8) -- the eps is below half an ulp of ||c|| ~ 8 and of anything
    larger, but not of 2^-13 ||c||; there the labels are held to the float64 scores of the formula (eps included) and the
    sums to the labels."""
    from anyloc_amd import ops
    n, D = 300, 64
    g = torch.Generator().manual_seed(K_)
    x = torch.randn(n, D, generator=g).to(DEV)
    centers = (x[torch.randperm(n, generator=g)[:K_]] + 0.2 * torch.randn(K_, D, generator=g).to(DEV)).contiguous()
    f = 2.0 ** case
    sums0, counts0, lab0 = ops.kmeans_step(x, centers, mode, want_labels=True)
    sums1, counts1, lab1 = ops.kmeans_step(x * f, centers * f, mode, want_labels=True)
    if mode == "cosine" and case < 0:
        scores = NF.assign_scores64(x * f, centers * f)
        moved = NF.check_labels(lab1, scores, 1e-6 * (x * f).double().norm(dim=1), f"kmeans cosine 2^{case}")
        print(f"kmeans cosine K={K_} 2^{case}: {int((lab0 != lab1).sum())} labels differ from the unscaled call's (the eps of the centre norm), "
              f"{moved} from the float64 arg-max")
        ref = torch.zeros(K_, D, dtype=torch.float64, device=DEV).index_add_(0, lab1, (x * f).double())
        assert float((sums1.double() - ref).norm() / ref.norm()) < 1e-6        # KMEANS_SUMS_RTOL, tests/test_gpu_vlad_topk.py
        return
    assert torch.equal(lab0, lab1) and torch.equal(counts0, counts1)
    scaled_bits(sums1, sums0, torch.tensor(f, device=DEV), f"kmeans {mode} K={K_} 2^{case}")


# ========================================================================================================== top-k ====
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("nq,opts", [(5, dict()), (130, dict(topk_h3=1, topk_screen=0)), (130, dict(topk_h3=1, topk_screen=1))],
                         ids=["few-query fp32", "panels", "screened"])
def test_topk_ip_scales_exactly(nq, opts, case):
    """Inner-product search: a query times a power of two has the same list with its distances times that power (raw rows and
    normalize_db); database rows times powers of two under normalize_db change nothing."""
    from anyloc_amd import ops
    qu, db = R.planted_rows(nq, 300, 2048, nq + 300 + 2048)
    # (the shortest planted row has norm 0.5: times 2^-36 it is still above the 1e-12 of F.normalize's clamp, times 2^-40 not)
    fq, fd = factors(nq, case), factors(300, case, seed=3, lowest=-36)
    with ops.options(**opts):
        for normalize in (False, True):
            d0, i0 = ops.topk(qu, db, 20, "ip", normalize_db=normalize)
            d1, i1 = ops.topk(qu * fq[:, None], db, 20, "ip", normalize_db=normalize)
            assert torch.equal(i0, i1), f"top-k {case} normalize={normalize}: a list moved with its query's scale"
            scaled_bits(d1, d0, fq[:, None], f"top-k distances {case} normalize={normalize}")
        d2, i2 = ops.topk(qu, db * fd[:, None], 20, "ip", normalize_db=True)
        assert torch.equal(i0, i2) and NF.same_bits(d0, d2), f"top-k {case}: normalised rows moved with their scale"
