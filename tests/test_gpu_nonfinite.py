"""Non-finite inputs (``pytest -m gpu``): every op contains the damage.  One unit of the input holds a NaN, a +inf or a -inf;
the call is compared with the same call on the clean twin (bit for bit outside the outputs that depend on the bad unit) and
with the float64 evaluation of the same formula (NaN exactly where float64 has NaN, the rest within the op's existing bar) --
rules 1 - 3 of include/anyloc_hip.h, Conventions, "Non-finite values"; the reading behind every case is
profiles/nonfinite_audit.md.  Generators, references and checkers: tests/_nonfinite_cases.py (tested on the CPU by
tests/test_nonfinite_cpu.py).  Shapes are the smallest that still have the structure where a leak can happen: a tail tile, a
16-row fragment boundary, image boundaries inside a 32-row group, several panels' worth of paths at one small database.

Every tolerance is the one of the parity test of the same op, imported from it or quoted with its name."""
import pytest
import torch
import torch.nn.functional as F

import _nonfinite_cases as NF
import _retrieval_refs as R
from _attention_refs import attention_f64
from _vlad_refs import l2rel
from anyloc_amd import synth
from test_gpu_kernels import ATTN_ATOL, L2NORM_REL, LAYERNORM_ATOL, gemm_nt_bound
from test_gpu_pca import f64_product_bar
from test_gpu_pooling import REL as POOL_REL
from test_gpu_vlad_topk import KMEANS_SUMS_RTOL, VLAD_RTOL
from test_gpu_x6 import GEMM_X6_REL

pytestmark = pytest.mark.gpu
DEV = "cuda"
VALUES = list(NF.VALUES)
WHERE_OF = dict(zip(VALUES, NF.WHERE))                     # nan -> first element, +inf -> last, -inf -> the 16-column boundary


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
    """a device error after a test ends the session: nothing more is started on a GPU that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU reported an error ({e}): nothing more runs on it in this session", returncode=3)


def _rows_mask(n, rows):
    m = torch.zeros(n, 1, dtype=torch.bool, device=DEV)
    m[list(rows)] = True
    return m


# ====================================================================================================== row ops ====
M, N, K = 70, 200, 64                                      # a 6-row tail tile of A, a ragged last tile of W
ARITH = ["f32", "x6", "h3"]


def _gemm_operands():
    g = torch.Generator().manual_seed(70200)
    a = torch.randn(M, K, generator=g) * (0.5 + torch.rand(M, 1, generator=g))
    w = torch.randn(N, K, generator=g) * 0.2
    bias = torch.randn(N, generator=g)
    return a.to(DEV), w.to(DEV), bias.to(DEV)


def _gemm(arith, a, w, bias):
    from anyloc_amd import ops
    if arith == "f32":
        return ops.gemm_nt(a, w, bias), None
    if arith == "x6":
        a3 = ops.split_x3(a)
        return ops.gemm_nt_x6(a3, ops.split_x3(w), M, N, K, bias), (a3.view(K // 16, 3, -1, 32), None)
    img, inv = ops.split_h2(a)
    return ops.gemm_nt_h3((img, inv), ops.split_h2(w), M, N, K, bias), (img.view(K // 16, 2, -1, 32), inv)


def _gemm_tol(arith, a, w, bias):
    """f32: gemm_nt_bound of tests/test_gpu_kernels.py::test_gemm_nt; x6: GEMM_X6_REL of tests/test_gpu_x6.py::
    test_gemm_x6_as_accurate_as_fp32; h3: that file's no_worse_than_fp32 against the same fp32 bound (1.5 x + 1e-7)"""
    mag = a.double().abs().nan_to_num(0.0, 0.0, 0.0) @ w.double().abs().nan_to_num(0.0, 0.0, 0.0).t() + bias.double().abs().nan_to_num(0.0, 0.0, 0.0)
    if arith == "x6":
        return GEMM_X6_REL * mag
    return gemm_nt_bound(mag) * (1.5 if arith == "h3" else 1.0) + (1e-7 * mag if arith == "h3" else 0.0)


@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("target", ["a0", "a15", "a16", "a69", "w0", "w199", "bias16"])
@pytest.mark.parametrize("arith", ARITH)
def test_gemm_contains_a_bad_row_a_bad_weight_row_and_a_bad_bias_element(arith, target, value):
    """gemm_nt, gemm_nt_x6 (through split_x3) and gemm_nt_h3 (through split_h2): a bad row of A spoils that row of C, a bad
    row n of W or bias element n column n; the plane images of the clean rows are byte-identical to the twin's."""
    a, w, bias = _gemm_operands()
    ops_in = {"a": a, "w": w, "bias": bias}
    name, idx = ("bias", int(target[4:])) if target.startswith("bias") else (target[0], int(target[1:]))
    unit = slice(idx, idx + 1) if name == "bias" else idx
    where = "first" if name == "bias" else WHERE_OF[value]
    bad = dict(ops_in, **{name: NF.plant(ops_in[name], unit, where, value)})
    twin = dict(ops_in, **{name: NF.clean_twin(ops_in[name], unit, where)})
    got, planes = _gemm(arith, bad["a"], bad["w"], bad["bias"])
    want, planes_t = _gemm(arith, twin["a"], twin["w"], twin["bias"])
    view = (lambda t: t) if arith == "f32" else NF.split_view          # (the bias is added in fp32 by every epilogue)
    ref = view(bad["a"]).double() @ view(bad["w"]).double().t() + bad["bias"].double()
    spoiled = _rows_mask(M, [idx]) if name == "a" else _rows_mask(N, [idx]).t()
    tol = _gemm_tol(arith, bad["a"], bad["w"], bad["bias"])
    NF.contained(got, want, ref, spoiled, atol=tol, tag=f"gemm {arith} {target} {value}")              # (one bar per output)
    if planes is not None and name == "a":
        keep = torch.arange(planes[0].shape[2], device=DEV) != idx
        assert torch.equal(planes[0][:, :, keep], planes_t[0][:, :, keep]), "the plane image of a clean row changed"
        if planes[1] is not None:
            assert NF.same_bits(planes[1][keep[:M]], planes_t[1][keep[:M]])


@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("row", [0, 15, 16, 69])
def test_layernorm_l2norm_and_rope_rows_contain_a_bad_row(row, value):
    from anyloc_amd import ops
    from test_gpu_dinov3 import _rope_rows_f64
    g = torch.Generator().manual_seed(row)
    x = (torch.randn(M, K, generator=g) * 2 + 0.5).to(DEV)
    w, b = torch.randn(K, generator=g).to(DEV), torch.randn(K, generator=g).to(DEV)
    bad, twin = NF.plant(x, row, WHERE_OF[value], value), NF.clean_twin(x, row, WHERE_OF[value])
    mask = _rows_mask(M, [row])
    # LAYERNORM_ATOL: tests/test_gpu_kernels.py::test_layernorm
    NF.contained(ops.layernorm(bad, w, b, 1e-6), ops.layernorm(twin, w, b, 1e-6),
                 F.layer_norm(bad.double(), (K,), w.double(), b.double(), 1e-6), mask, atol=LAYERNORM_ATOL, tag=f"layernorm row {row} {value}")
    # L2NORM_REL (of the largest entry, < 1 here): tests/test_gpu_kernels.py::test_l2norm_rows
    NF.contained(ops.l2norm_rows(bad), ops.l2norm_rows(twin), F.normalize(bad.double(), dim=-1), mask, atol=L2NORM_REL,
                 tag=f"l2norm_rows row {row} {value}")
    # rope_rows: 2 images of 5 prefix rows + 30 patches, one head; 2e-7 of the row's largest magnitude
    # (tests/test_gpu_dinov3.py::test_rope_rows_alone)
    from anyloc_amd.extractor import rope_table
    table = rope_table(80, 96)                                          # 5 x 6 patches of 16
    qkv = (torch.randn(M, 192, generator=g) * 2).to(DEV)
    qbad, qtwin = NF.plant(qkv, row, WHERE_OF[value], value), NF.clean_twin(qkv, row, WHERE_OF[value])
    ref = _rope_rows_f64(qbad.cpu(), torch.cat([table] * 2), [0, 35, 70], 5, 1)
    NF.contained(ops.rope_rows(qbad, 1, table.to(DEV), tokens=35, prefix=5), ops.rope_rows(qtwin, 1, table.to(DEV), tokens=35, prefix=5),
                 ref.to(DEV), mask, atol=2e-7 * float(qkv.abs().max()), tag=f"rope_rows row {row} {value}")


# ==================================================================================================== attention ====
B, T, HEADS = 3, 40, 2                                     # both image boundaries (rows 40, 80) inside a 32-row group
RAGGED_T = [40, 33, 50]
ATTN = {"fp32-mfma": dict(attn_x6=0), "split-bf16": dict(attn_x6=1), "h3": dict(attn_h3_ks=1), "h3-keys-split-2": dict(attn_h3_ks=2)}


def _attn_batch(tokens):
    g = torch.Generator().manual_seed(sum(tokens))
    return [torch.randn(t, 3 * HEADS * 64, generator=g) * 1.5 for t in tokens]


def _run_attention(kernel, parts, ragged):
    """-> (outputs per image as float64 [T_i, D] on the CPU, bits per image to compare)"""
    from anyloc_amd import ops
    from test_gpu_ragged import _run_ragged_attention
    tokens = [p.shape[0] for p in parts]
    D = HEADS * 64
    with ops.options(**ATTN[kernel]):
        if ragged:
            out, off = _run_ragged_attention("h3" if kernel.startswith("h3") else kernel, torch.cat(parts), tokens, HEADS)
            return [out[off[i]:off[i + 1]] for i in range(len(parts))]
        qkv = torch.stack(parts).to(DEV)
        if kernel.startswith("h3"):
            img, inv = ops.attention_h3(qkv, HEADS)
            out = ops.h2_image_to_f32(img, inv, B * T, D).reshape(B, T, D).cpu()
        else:
            out = ops.attention(qkv, HEADS).cpu().double()
    return list(out)


@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("part", ["q", "k", "v"])
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("kernel", list(ATTN))
def test_attention_contains_a_bad_image(kernel, ragged, part, value):
    """Image 1 of three holds the bad value in q only, k only or v only of one token; images 0 and 2 share a 32-row group with
    it.  Their outputs are the twin's bit for bit; image 1 has NaN where float64 attention has (the two split arithmetics
    see an infinity as a NaN).  Bars: ATTN_ATOL (tests/test_gpu_kernels.py::test_attention), 3e-6 max|v| + 2e-6
    (::test_attention_h3)."""
    parts = _attn_batch(RAGGED_T if ragged else [T] * B)
    D = HEADS * 64
    col0 = "qkv".index(part) * D
    token = {"nan": 0, "+inf": 7, "-inf": parts[1].shape[0] - 1}[value]       # first row, an inner row, the row at the boundary
    unit = (token, slice(col0, col0 + D))
    bad = [NF.plant(p, unit, WHERE_OF[value], value) if i == 1 else p for i, p in enumerate(parts)]
    twin = [NF.clean_twin(p, unit, WHERE_OF[value]) if i == 1 else p for i, p in enumerate(parts)]
    got, want = _run_attention(kernel, bad, ragged), _run_attention(kernel, twin, ragged)
    for i in (0, 2):
        assert NF.same_bits(got[i], want[i]), f"image {i} changed with its batch neighbour"
    view = (lambda t: t) if kernel == "fp32-mfma" else NF.split_view
    ref = attention_f64(view(bad[1]), HEADS)
    vmax = float(twin[1][:, 2 * D:].abs().max())
    atol = 3e-6 * vmax + 2e-6 if kernel.startswith("h3") else ATTN_ATOL
    everything = torch.ones(1, 1, dtype=torch.bool)
    NF.contained(got[1], want[1], ref, everything, atol=atol, tag=f"attention {kernel} ragged={ragged} {part} {value}")
    assert not bool(torch.isfinite(ref).all())


# ================================================================================================== ViT forward ====
VIT_SIZES = {False: [(56, 56)] * 3, True: [(56, 56), (42, 70), (70, 42)]}


def _vit_images(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(3, h, w, generator=g) for h, w in sizes]


@pytest.fixture(scope="module")
def vit_models():
    from anyloc_amd.extractor import HipDinoV2
    cache = {}

    def get(name, mode):
        if (name, mode) not in cache:
            sd = synth.synthetic_state_dict(name, 31, depth=2)
            cache[(name, mode)] = HipDinoV2(name, {k: v.to(DEV) for k, v in sd.items()}, torch.device(DEV), gemm=mode)
        return cache[(name, mode)]
    yield get
    cache.clear()


def _vit_forward(model, imgs, ragged):
    """-> (token rows per image, reruns of the FFN check in this call, blocks it ran exact)"""
    before = model.ffn_reruns
    if ragged:
        packed, off = model.forward_taps_ragged([im.to(DEV) for im in imgs], [(1, "token")], use_cls=True)
        off = off.cpu().tolist()
        out = [packed[off[i]:off[i + 1]] for i in range(len(imgs))]
    else:
        out = list(model.forward_taps(torch.stack(imgs).to(DEV), [(1, "token")], use_cls=True))
    torch.cuda.synchronize()
    return out, model.ffn_reruns - before, set(model.ffn_exact_blocks)


@pytest.mark.parametrize("value", ["nan", "+inf"])
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("name,mode", [("dinov2_vits14", "h3"), ("dinov2_vits14", "x6"), ("dinov2_vits14", "f32"), ("dinov3_vits16", "h3")])
def test_vit_forward_contains_a_bad_image(vit_models, name, mode, ragged, value):
    """One pixel of the middle image is NaN or +inf: that image's tokens are all NaN, the other two images' tokens are the
    twin's bit for bit (their rows share 32-row attention groups and GEMM tiles with the bad image's), and the FFN check
    (h3, on by default) re-runs nothing it does not re-run for the twin."""
    from anyloc_amd import ops
    patch = 16 if "dinov3" in name else 14
    sizes = [(h // 14 * patch, w // 14 * patch) for h, w in VIT_SIZES[ragged]]
    imgs = _vit_images(sizes, 5)
    unit = (0, 5, slice(0, sizes[1][1]))
    bad = [NF.plant(im, unit, "col16", value) if i == 1 else im for i, im in enumerate(imgs)]
    twin = [NF.clean_twin(im, unit, "col16") if i == 1 else im for i, im in enumerate(imgs)]
    with ops.options(x6_min_rows=0):                                      # (small batches: keep the split-bf16 kernels)
        model = vit_models(name, mode)
        assert model.gemm == mode and (mode != "h3" or model.ffn_check)
        want, reruns_t, exact_t = _vit_forward(model, twin, ragged)
        got, reruns, exact = _vit_forward(model, bad, ragged)
    for i in (0, 2):
        assert bool(torch.isfinite(want[i]).all())
        assert NF.same_bits(got[i], want[i]), f"{name} {mode}: image {i} changed with its batch neighbour"
    assert bool(torch.isnan(got[1]).all()), f"{int((~torch.isnan(got[1])).sum())} tokens values of the bad image are numbers"
    assert (reruns, exact) == (reruns_t, exact_t)


# ========================================================================================================== VLAD ====
def _vlad_case(D, K=8):
    g = torch.Generator().manual_seed(D)
    tokens = torch.randn(3, 40, D, generator=g)
    centers = 0.8 * F.normalize(tokens.reshape(-1, D)[torch.randperm(120, generator=g)[:K]] + 0.3 * torch.randn(K, D, generator=g), dim=-1)
    return tokens.to(DEV), centers.to(DEV)


def _tie(x, centers=None):
    """what an fp32 score may be off by, per row: 1e-6 of |x| (cosine; the gap_tol of tests/test_gpu_vlad_topk.py::check_labels on
    unit rows), of 2 |x| max|c| + max|c|^2 (euclidean)"""
    n = x.double().reshape(-1, x.shape[-1]).norm(dim=1).nan_to_num(0.0, 0.0, 0.0)
    if centers is None:
        return 1e-6 * n
    c = float(centers.double().norm(dim=1).nan_to_num(0.0, 0.0, 0.0).max())
    return 1e-6 * (2 * n * c + c * c)


VLAD_PATHS = {"fused": (384, dict(), 0), "fused-parts-2": (384, dict(), 2), "two-pass": (384, dict(vlad_two_pass=1), 0), "two-pass-D100": (100, dict(), 0)}


@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("path", list(VLAD_PATHS))
def test_vlad_hard_contains_a_bad_token_and_never_assigns_to_a_bad_centre(path, value):
    from anyloc_amd import ops
    D, opts, parts = VLAD_PATHS[path]
    tokens, centers = _vlad_case(D)
    unit = (1, 7)
    bad, twin = NF.plant(tokens, unit, WHERE_OF[value], value), NF.clean_twin(tokens, unit, WHERE_OF[value])
    with ops.options(**opts):
        got, lab = ops.vlad(bad, centers, "hard", return_labels=True, parts=parts)
        want, lab_t = ops.vlad(twin, centers, "hard", return_labels=True, parts=parts)
        tag = f"vlad {path} token {value}"
        NF.check_labels(lab, NF.assign_scores64(bad.reshape(-1, D), centers), _tie(bad), tag)
        keep = torch.arange(120, device=DEV) != 47
        assert torch.equal(lab[keep], lab_t[keep]), "a clean token's label changed"
        if value == "nan":
            assert int(lab[47]) == 0
        ref = NF.hard_vlad_nan(bad, centers, lab)
        NF.contained(got, want, ref, _rows_mask(3, [1]), atol=VLAD_RTOL, tag=tag)        # VLAD_RTOL: tests/test_gpu_vlad_topk.py
        assert bool(torch.isnan(ref[1]).all())                             # (the global norm spreads it over the image)
        # a bad centre k: its scores are NaN for every token, no token goes there, the descriptors are the float64 ones
        cbad = NF.plant(centers, 5, WHERE_OF[value], value)
        got_c, lab_c = ops.vlad(twin, cbad, "hard", return_labels=True, parts=parts)
        scores = NF.assign_scores64(twin.reshape(-1, D), cbad)
        assert bool(torch.isnan(scores[:, 5]).all())
        NF.check_labels(lab_c, scores, _tie(twin), f"vlad {path} centre {value}")
        assert not bool((lab_c == 5).any())
        ref_c = NF.hard_vlad_nan(twin, cbad, lab_c)
        assert not bool(torch.isnan(ref_c).any())
        for i in range(3):
            assert l2rel(got_c[i], ref_c[i]) < VLAD_RTOL, (i, l2rel(got_c[i], ref_c[i]))


@pytest.mark.parametrize("value", VALUES)
def test_vlad_soft_assigned_residuals_and_weights_contain_a_bad_token(value):
    """The other VLAD entry points, bad token 7 of image 1 (the single-image ones get image 1 and its twin): soft VLAD of the
    batch, ``vlad_assigned`` with labels and with soft weights, ``vlad_residuals`` and ``vlad_soft_weights`` row by row."""
    from anyloc_amd import ops
    D, K = 384, 8
    tokens, centers = _vlad_case(D)
    bad, twin = NF.plant(tokens, (1, 7), WHERE_OF[value], value), NF.clean_twin(tokens, (1, 7), WHERE_OF[value])
    tag = f"vlad soft {value}"
    got, want = ops.vlad(bad, centers, "soft"), ops.vlad(twin, centers, "soft")
    ref = torch.full((3, K * D), float("nan"), dtype=torch.float64, device=DEV)     # every weight of the token is NaN, the norms spread it
    ref[[0, 2]] = want[[0, 2]].double()
    NF.contained(got, want, ref, _rows_mask(3, [1]), tag=tag)
    row = _rows_mask(40, [7])
    # residuals: normalise(x) - c per token; bar: tests/test_gpu_addressing.py::test_vlad_residuals_output_past_2g_elements
    res_ref = F.normalize(bad[1].double(), dim=-1)[:, None, :] - centers.double()[None]
    NF.contained(ops.vlad_residuals(bad[1], centers), ops.vlad_residuals(twin[1], centers), res_ref, row[:, :, None], atol=L2NORM_REL + 2.0 ** -23, tag=f"residuals {value}")
    cos = F.cosine_similarity(bad[1].double()[:, None, :], centers.double()[None], dim=-1)
    NF.contained(ops.vlad_soft_weights(bad[1], centers), ops.vlad_soft_weights(twin[1], centers), torch.softmax(cos, dim=1), row,
                 tag=f"soft weights {value}")                           # (every weight of the bad token is NaN: no bar needed)
    assert bool(torch.isnan(cos[7]).all())
    lab = NF.hard_assign_nan(NF.assign_scores64(bad[1], centers))
    a_ref = NF.hard_vlad_nan(bad[1:2], centers, lab)[0]
    a_got = ops.vlad_assigned(bad[1], centers, labels=lab)
    assert bool(torch.isnan(a_ref).all()) and bool(torch.isnan(a_got).all())
    w = torch.softmax(F.cosine_similarity(twin[1].double()[:, None, :], centers.double()[None], dim=-1), dim=1).float()
    assert bool(torch.isnan(ops.vlad_assigned(bad[1], centers, soft=w)).all())


# ======================================================================================================= k-means ====
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("K", [5, 200])
@pytest.mark.parametrize("mode", ["cosine", "euclidean"])
def test_kmeans_step_contains_a_bad_row_and_never_chooses_a_bad_centre(mode, K, value):
    """n = 300, D = 64 (the two-pass kernels; K = 200: the half-slice accumulate): a bad row gets label 0 when its scores are
    NaN, every label is in range, the counts add up, and the sums of the clusters neither it nor its twin joins keep their
    bits; a bad centre is never chosen.  KMEANS_SUMS_RTOL: tests/test_gpu_vlad_topk.py."""
    from anyloc_amd import kmeans, ops
    n, D = 300, 64
    g = torch.Generator().manual_seed(K)
    x = torch.randn(n, D, generator=g).to(DEV)
    centers = (x[torch.randperm(n, generator=g)[:K]] + 0.2 * torch.randn(K, D, generator=g).to(DEV)).contiguous()
    eu = mode == "euclidean"
    bad, twin = NF.plant(x, 150, WHERE_OF[value], value), NF.clean_twin(x, 150, WHERE_OF[value])
    sums, counts, lab = ops.kmeans_step(bad, centers, mode, want_labels=True)
    sums_t, counts_t, lab_t = ops.kmeans_step(twin, centers, mode, want_labels=True)
    tag = f"kmeans {mode} K={K} row {value}"
    scores = NF.assign_scores64(bad, centers, eu)
    NF.check_labels(lab, scores, _tie(bad, centers if eu else None), tag)
    if bool(torch.isnan(scores[150]).all()):
        assert int(lab[150]) == 0
    keep = torch.arange(n, device=DEV) != 150
    assert torch.equal(lab[keep], lab_t[keep]) and float(counts.sum()) == n
    assert torch.equal(counts, torch.bincount(lab, minlength=K).float())
    touched = _rows_mask(K, {int(lab[150]), int(lab_t[150])})
    ref = torch.zeros(K, D, dtype=torch.float64, device=DEV).index_add_(0, lab, bad.double())
    NF.contained(sums, sums_t, ref, touched, atol=KMEANS_SUMS_RTOL * float(ref.nan_to_num(0.0, 0.0, 0.0).norm()), tag=tag)
    # a bad centre
    cbad = NF.plant(centers, 3, WHERE_OF[value], value)
    _, counts_c, lab_c = ops.kmeans_step(twin, cbad, mode, want_labels=True)
    scores_c = NF.assign_scores64(twin, cbad, eu)
    NF.check_labels(lab_c, scores_c, _tie(twin, centers if eu else None), f"kmeans {mode} K={K} centre {value}")
    if bool(torch.isnan(scores_c[:, 3]).all()):
        assert not bool((lab_c == 3).any()) and float(counts_c[3]) == 0.0
    km = kmeans.KMeans(K, mode=mode)
    km.centroids = cbad
    assert torch.equal(km.predict(twin), lab_c)
    km.centroids = centers
    assert torch.equal(km.predict(bad), lab)


@pytest.mark.parametrize("value", VALUES)
def test_kmeans_update_turns_a_nan_quotient_into_zero_and_nothing_else(value):
    """fast-pytorch-kmeans' ``c[c != c] = 0`` is part of the formula: a NaN sum gives a zero coordinate (an infinite one stays),
    every other coordinate keeps the twin's bits, the error is the float64 sum of the fp32 squares."""
    from anyloc_amd import ops
    g = torch.Generator().manual_seed(8)
    sums, old = torch.randn(8, 64, generator=g).to(DEV) * 20, torch.randn(8, 64, generator=g).to(DEV)
    counts = torch.tensor([20.0, 3, 0, 7, 11, 1, 40, 9], device=DEV)
    sums[2] = 0.0                                                           # (an empty cluster has summed nothing)
    bad, twin = NF.plant(sums, 4, WHERE_OF[value], value), NF.clean_twin(sums, 4, WHERE_OF[value])
    new, err = ops.kmeans_update(bad, counts, old)
    new_t, _ = ops.kmeans_update(twin, counts, old)
    ref = bad.double() / counts.double()[:, None]
    ref = torch.where(torch.isnan(ref), torch.zeros_like(ref), ref)
    assert bool((new[2] == 0).all())                                        # the empty cluster: 0 / 0 -> 0
    # one fp32 division: 2^-23 of the quotient (tests/test_gpu_vlad_soft.py, the kmeans_update parity)
    NF.contained(new, new_t, ref, _rows_mask(8, [4]), rtol=2.0 ** -23, tag=f"kmeans_update {value}")
    want_err = float((((new - old) ** 2).double()).sum())
    assert float(err) == want_err or abs(float(err) - want_err) <= 1e-12 * abs(want_err)


# ======================================================================================================= pooling ====
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("method", ["average", "max", "gem", "gem_abs"])
def test_pooling_contains_a_bad_token(method, value):
    """POOL_REL (relative to the descriptor's norm): tests/test_gpu_pooling.py"""
    from anyloc_amd import ops
    g = torch.Generator().manual_seed(3)
    x = F.normalize(torch.randn(3, 40, 100, generator=g), dim=-1).to(DEV)
    bad, twin = NF.plant(x, (1, 7), WHERE_OF[value], value), NF.clean_twin(x, (1, 7), WHERE_OF[value])
    got, want = ops.pool(bad, method, 3.0), ops.pool(twin, method, 3.0)
    xd = bad.double()
    if method == "average":
        ref = xd.mean(dim=1)
    elif method == "max":
        ref = xd.max(dim=1)[0]
    elif method == "gem":
        m = (xd ** 3.0).mean(dim=1)
        ref = m.abs() ** (1 / 3.0) * torch.sign(m)
        ref = torch.where(torch.isnan(m), m, ref)
    else:
        ref = (xd.abs() ** 3.0).mean(dim=1) ** (1 / 3.0)
    NF.contained(got, want, ref, _rows_mask(3, [1]), atol=POOL_REL * float(want.double().norm(dim=1).max()), tag=f"pool {method} {value}")


# =========================================================================================================== PCA ====
@pytest.mark.parametrize("value", VALUES)
def test_pca_products_contain_a_bad_sample(value):
    """``pca_gram_f64`` and ``pca_axes_f64`` (float64 matrix cores), 70 samples x 130 features with the mean of the clean data:
    the Gram's row and column of the bad sample are non-finite and nothing else, the scatter's of the bad FEATURE, the
    back-projection's column of it.  f64_product_bar: tests/test_gpu_pca.py::test_pca_f64_products_vs_float64."""
    from anyloc_amd import ops
    n, f, k = 70, 130, 7
    g = torch.Generator().manual_seed(n * 1000 + f)
    x = (torch.randn(n, f, generator=g) * 3 + 40.0).to(DEV)
    col = NF.position(f, WHERE_OF[value])
    bad, twin = NF.plant(x, 33, WHERE_OF[value], value), NF.clean_twin(x, 33, WHERE_OF[value])
    mean = x.mean(dim=0, dtype=torch.float64)
    xw = bad.double() - mean
    for side, ref, unit in ((0, xw @ xw.t(), 33), (1, xw.t() @ xw, col)):
        size = ref.shape[0]
        cross = _rows_mask(size, [unit]) | _rows_mask(size, [unit]).t()
        bar = f64_product_bar(float(ref.nan_to_num(0.0, 0.0, 0.0).abs().max()), max(n, f))
        NF.contained(ops.pca_gram_f64(bad, mean, side), ops.pca_gram_f64(twin, mean, side), ref, cross, atol=bar, tag=f"pca gram side {side} {value}")
    vec = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))[0].to(DEV)
    ref = vec[:, :k].t() @ xw
    NF.contained(ops.pca_axes_f64(vec, k, bad, mean), ops.pca_axes_f64(vec, k, twin, mean), ref, _rows_mask(f, [col]).t(),
                 atol=f64_product_bar(float(ref.nan_to_num(0.0, 0.0, 0.0).abs().max() + 1), n), tag=f"pca axes {value}")


# ========================================================================================================= top-k ====
NDB, KTOP, BAD_Q, BAD_ROW = 300, 20, 3, 150
SCREEN = dict(topk_screen=1, topk_h3=1)
# path -> (queries, columns, options, the arithmetic that scores: "f32" keeps an infinity, the split ones see a NaN)
TOPK_PATHS = {
    "few-query fp32": (5, 2048, dict(), "f32"),
    "few-query fp16 planes": (5, 4096, dict(), "split"),
    "panels": (130, 2048, dict(topk_h3=1, topk_screen=0), "split"),
    "screened one-shot": (130, 2048, SCREEN, "split"),
    "prepared index with rows": (130, 2048, SCREEN, "split"),
    "rows-free": (130, 2048, SCREEN, "split"),
    "no_wait": (130, 2048, SCREEN, "split"),
    "FlatIndex": (130, 2048, SCREEN, "split"),
    "FlatIndex rows-free": (130, 2048, SCREEN, "split"),
}
# (a no_wait call enqueues both remedies behind their gates: its profile names the fallback's kernels whether or not they ran)
SCREENED_PATHS = ("screened one-shot", "prepared index with rows", "rows-free", "FlatIndex", "FlatIndex rows-free")


def _search(path, qu, db, metric, normalize):
    """-> ((distances, indices), profile, the queries the scores are formed with)"""
    from anyloc_amd import ops, retrieval
    if path.startswith("FlatIndex"):
        kw = dict(keep_fp32=False, rescore="planes") if path.endswith("rows-free") else {}
        index = retrieval.FlatIndex(db, "cosine" if metric == "ip" else "l2", normalize, planes=True, **kw)
        res, prof = R.profiled(lambda: index.search(qu, KTOP))
        return res, prof, F.normalize(qu, dim=-1) if normalize else qu     # (torch's, not the op under test)
    if path in ("prepared index with rows", "rows-free"):
        planes = ops.topk_index_build(db)
        kw = dict(rescore_planes=True) if path == "rows-free" else dict(db=db)
        res, prof = R.profiled(lambda: ops.topk_indexed(qu, planes, db.shape[0], KTOP, metric, normalize_db=normalize, **kw))
        return res, prof, qu
    res, prof = R.profiled(lambda: ops.topk(qu, db, KTOP, metric, normalize_db=normalize, no_wait=path == "no_wait"))
    return res, prof, qu


@pytest.mark.parametrize("normalize", [True, False], ids=["normalize_db", "raw rows"])
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("path", list(TOPK_PATHS))
def test_topk_contains_a_bad_query_and_never_lists_a_bad_row(path, metric, normalize):
    """Every top-k path at one small shape (``_retrieval_refs.planted_rows``, near-ties excused under cap="gaps" as everywhere
    that recipe is searched; bars scaled by the largest raw row norm without normalize_db, as
    tests/test_gpu_screen_rowsfree.py::test_rows_free_screened_search_on_raw_rows).
    A bad query: its own list is what rule 3 says (a NaN query: all padding -- the tail rule, the same on every path), every
    other query's list is the twin's bit for bit.  A bad database row: every list passes the float64 check with NaN ranked
    last, the row is never listed while its score is NaN, and a screened path stays screened -- one bad row among the
    database must not send the call into the fallback."""
    from anyloc_amd import ops
    nq, dim, opts, arith = TOPK_PATHS[path]
    qu, db = R.planted_rows(nq, NDB, dim, nq + NDB + dim)
    view = (lambda t: t) if arith == "f32" else NF.split_view
    others = torch.arange(NDB, device=DEV) != BAD_ROW
    scale = 1.0 if normalize else float(db[others].double().norm(dim=1).max()) ** (2 if metric == "l2" else 1)
    with ops.options(**opts):
        (d_t, i_t), prof_t, _ = _search(path, qu, db, metric, normalize)
        if path in SCREENED_PATHS:
            assert R._screened_without_fallback(prof_t), sorted(prof_t)
        for value in VALUES:
            tag = f"{path} {metric} normalize={normalize} {value}"
            # ---- a bad query
            q_bad, q_twin = NF.plant(qu, BAD_Q, WHERE_OF[value], value), NF.clean_twin(qu, BAD_Q, WHERE_OF[value])
            (d, i), _, q_used = _search(path, q_bad, db, metric, normalize)
            (d_c, i_c), _, _ = _search(path, q_twin, db, metric, normalize)
            keep = torch.arange(nq, device=DEV) != BAD_Q
            assert torch.equal(i[keep], i_c[keep]) and NF.same_bits(d[keep], d_c[keep]), f"{tag}: another query's list changed"
            s = R.exact_scores64(view(q_used), db, metric, normalize=normalize)
            NF.check_lists_nan(d, i, s, KTOP, metric, f"{tag}, bad query", scale=scale, cap="gaps")
            # ---- a bad database row
            db_bad = NF.plant(db, BAD_ROW, WHERE_OF[value], value)
            (d, i), prof, q_used = _search(path, qu, db_bad, metric, normalize)
            s = R.exact_scores64(q_used, view(db_bad), metric, normalize=normalize)
            NF.check_lists_nan(d, i, s, KTOP, metric, f"{tag}, bad row", scale=scale, cap="gaps")
            if bool(torch.isnan(s[:, BAD_ROW]).all()):
                assert not bool((i == BAD_ROW).any())
            stayed = R._screened_without_fallback(prof)
            print(f"{tag}: bad row, screened call stayed screened: {stayed}")
            if path in SCREENED_PATHS:
                assert stayed, sorted(prof)


@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("path", ["screened one-shot", "rows-free"])
def test_one_bad_row_does_not_send_the_screened_search_into_the_fallback(path, metric, value):
    """Raw rows (no normalize_db), 700 of them -- more than the 512 candidates a query may have: the bound of every query
    scales with the LARGEST raw row norm of the database.  An infinite element used to make that norm, hence every margin,
    infinite: every column a candidate, every query over the limit, the whole call re-run unscreened.  Now the row's sum of
    squares is NaN (no share in the maximum), its scores are NaN, the call stays screened and the lists are the exact ones."""
    from anyloc_amd import ops
    nq, ndb, dim = 130, 700, 2048
    qu, db = R.planted_rows(nq, ndb, dim, nq + ndb + dim)
    db_bad = NF.plant(db, 333, WHERE_OF[value], value)
    scale = float(db[torch.arange(ndb, device=DEV) != 333].double().norm(dim=1).max()) ** (2 if metric == "l2" else 1)
    with ops.options(**SCREEN):
        if path == "rows-free":
            planes = ops.topk_index_build(db_bad)
            (d, i), prof = R.profiled(lambda: ops.topk_indexed(qu, planes, ndb, KTOP, metric, rescore_planes=True))
        else:
            (d, i), prof = R.profiled(lambda: ops.topk(qu, db_bad, KTOP, metric))
    assert R._screened_without_fallback(prof), sorted(prof)
    assert not bool((i == 333).any())
    s = R.exact_scores64(qu, NF.split_view(db_bad), metric, normalize=False)
    NF.check_lists_nan(d, i, s, KTOP, metric, f"{path} raw rows {metric} {value}", scale=scale, cap="gaps")


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("path", list(TOPK_PATHS))
def test_tail_rule_on_every_path_with_a_database_of_bad_rows(path, metric):
    """The tail rule when fewer than k rows can be listed: 12 rows, 9 of them bad (NaN, +inf, -inf in turn), k = 20, normalize_db.
    Every path lists the 3 good rows, best first, and pads with index -1 and distance -inf (inner product) / +inf (L2)."""
    from anyloc_amd import ops
    nq, dim, opts, _ = TOPK_PATHS[path]
    qu, db = R.planted_rows(nq, 12, dim, 7)
    good = [1, 5, 10]
    for r in range(12):
        if r not in good:
            db = NF.plant(db, r, NF.WHERE[r % 3], VALUES[r % 3])
    with ops.options(**opts):
        (d, i), _, q_used = _search(path, qu, db, metric, True)
    assert torch.equal(i[:, :3].sort(dim=1).values, torch.tensor(good, device=DEV).expand(nq, 3)), (path, metric)
    assert bool((i[:, 3:] == -1).all()) and bool((d[:, 3:] == NF.pad_distance(metric)).all())
    s = R.exact_scores64(q_used, db[good], metric)
    R.check_lists(d[:, :3], torch.searchsorted(torch.tensor(good, device=DEV), i[:, :3]), s, 3, metric, f"tail rule, {path} {metric}")


def test_topk_index_base_with_a_database_of_bad_rows():
    """The range rule with an index_base on the fp32, fp16-panel and screened searches of the same 12 rows."""
    from anyloc_amd import ops
    qu, db = R.planted_rows(130, 12, 2048, 7)
    good = [1, 5, 10]
    for r in range(12):
        if r not in good:
            db = NF.plant(db, r, NF.WHERE[r % 3], VALUES[r % 3])
    for opts in (dict(topk_h3=0), dict(topk_h3=1, topk_screen=0), SCREEN):
        for metric in ("ip", "l2"):
            with ops.options(**opts):
                d, i = ops.topk(qu, db, KTOP, metric, normalize_db=True, index_base=5000)
            assert bool(((i == -1) | ((i >= 5000) & (i < 5012))).all())
            assert torch.equal(i[:, :3].sort(dim=1).values, torch.tensor(good, device=DEV).expand(130, 3) + 5000), (opts, metric)
            assert bool((i[:, 3:] == -1).all()) and bool((d[:, 3:] == NF.pad_distance(metric)).all())
