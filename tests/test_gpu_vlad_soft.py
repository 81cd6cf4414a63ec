"""Soft-assignment VLAD, VLAD from a given assignment and the k-means centre update (csrc/vlad.hip) against the CPU oracle
and a float64 evaluation, at the sizes where their launches change: the score stride kpad = 64 (K > 32), the dynamic-LDS
request of soft_accumulate_kernel on both sides of 64 KB (K = 42 / 43) and at its largest (K = 64), feature widths that
are no multiple of the 128-column slice, ragged batches with empty and single-token images, every flag pair; the dense
[N, K] weights of a cache hit (row stride K, not kpad); given labels on the half-width slices of K > 128.

Yardstick (the one of test_vlad_tight_clusters): the fp32 oracle is the reference's own arithmetic, the float64 value the
truth.  A descriptor must be as close to float64 as the oracle is (factor 3 + 1e-6; the vectors are unit norm, so the
norm of the difference is the L2-relative error) and within VLAD_RTOL of the oracle; a weight must be within 3 x the
oracle's largest absolute weight error + 1e-6, both taken per case and temperature.  With the inputs below the oracle
itself stays within 7.3e-7 (soft descriptors), 2.5e-7 (given labels) and 1.6e-7 (given weights) of float64; its weights
within 4.4e-7 up to temperature 7.5 and 2.1e-6 at temperature 50 (two centres drawn from one mode compete for its tokens,
and temp * w (1 - w) <= 12.5 times the ~1.6e-7 fp32 error of a cosine lands there, whatever the seed) -- re-check those
figures on the CPU before changing the recipe."""
import functools

import pytest
import torch
from torch.nn import functional as F

from _vlad_refs import hard_vlad_f64, l2rel
from anyloc_amd import synth
from oracle import vlad_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
VLAD_RTOL = 1e-5      # north_star: VLAD descriptors within 1e-5 relative (L2-relative, fp32)
FLAGS = ((True, True), (False, True), (True, False), (False, False))      # (norm_descs, intra_norm)
TEMPS = (1.0, 7.5, 50.0)

# K, D, tokens per image
SOFT_CASES = [
    (33, 68, (97, 0, 1, 40)),     # kpad 64 with 31 padded columns; one partly live slice; empty and single-token images
    (42, 132, (129, 16)),         # last K under the default LDS limit (64 512 bytes); second slice has 4 live columns
    (43, 200, (257, 8)),          # first K over 64 KB (66 048 bytes)
    (64, 128, (300, 3)),          # largest LDS request (98 304 bytes); exactly one full slice
    (64, 1536, (64,)),            # the workload's width at the largest K; 12 slices
    (1, 64, (50,)),               # soft-max over one cluster
    (32, 384, (130,)),            # K equal to kpad
]
SOFT_IDS = [f"K{K}_D{D}_N{'_'.join(map(str, ns))}" for K, D, ns in SOFT_CASES]
LABEL_CASES = [(129, 100, 300), (256, 100, 700), (128, 260, 257), (200, 64, 1), (5, 64, 77)]      # K, D, N
WEIGHT_CASES = [(33, 68, 97), (43, 200, 129), (64, 132, 60)]


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def _inputs(K, D, counts):
    """-> (centres [K, D], one [N_i, D] token tensor per image): tokens around the centres' own directions with norms in
    [0.5, 1.5); row 3 of every image with more than 5 tokens is zero (the 1e-8 clamp of the cosine, the 1e-12 clamp of the
    normalisation)."""
    seed = K + D + sum(counts)
    g = torch.Generator().manual_seed(K * D + sum(counts))
    centers = 0.7 * synth.clustered_tokens(1, K, D, n_modes=K, seed=seed)[0] + 0.01 * torch.randn(K, D, generator=g)
    n_max = max(max(counts), 1)
    x = synth.clustered_tokens(len(counts), n_max, D, n_modes=K, seed=seed) * (0.5 + torch.rand(len(counts), n_max, 1, generator=g))
    imgs = []
    for i, n in enumerate(counts):
        t = x[i, :n].clone()
        if n > 5:
            t[3] = 0.0
        imgs.append(t)
    return centers, tuple(imgs)


# ------------------------------------------------------------------------------------------------- float64 restatements
def _weights_f64(x, centers, temp):
    """softmax_k(temp * F.cosine_similarity(x, c)) in float64 (each norm clamped at 1e-8)."""
    x, c = x.double(), centers.double()
    cos = (x @ c.t()) / (x.norm(dim=1).clamp_min(1e-8)[:, None] * c.norm(dim=1).clamp_min(1e-8)[None, :])
    return F.softmax(temp * cos, dim=1)


def _soft_f64(x, centers, w, norm_descs=True, intra_norm=True):
    """The reference's all-cluster sum (utilities.py:881-884) in closed form and float64:
    block k = sum_q w[q,k] * (K * xh[q] - sum_c c[c]), then utilities.py:885-889."""
    K, D = centers.shape
    x, c, w = x.double(), centers.double(), w.double()
    xh = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12) if norm_descs else x
    out = K * (w.t() @ xh) - w.sum(dim=0)[:, None] * c.sum(dim=0)[None, :]
    if intra_norm:
        out = F.normalize(out, dim=1)
    return F.normalize(out.reshape(-1), dim=0)


@functools.lru_cache(maxsize=None)
def _soft_refs(case, img, temp, norm_descs, intra_norm):
    """-> (oracle descriptor, oracle weights, float64 descriptor, float64 weights) of one image of a soft case."""
    K, D, counts = SOFT_CASES[case]
    centers, imgs = _inputs(K, D, counts)
    v32, w32 = vlad_ref.vlad_soft(imgs[img], centers, temp, norm_descs, intra_norm)
    w64 = _weights_f64(imgs[img], centers, temp)
    return v32, w32, _soft_f64(imgs[img], centers, w64, norm_descs, intra_norm), w64


def _judge(got, v32, v64, what):
    """The descriptor yardstick; -> (kernel / oracle distance to float64, l2rel to the oracle)."""
    got = got.detach().cpu()
    e_or = float((v32.double() - v64).norm())
    e_k = float((got.double() - v64).norm())
    rel = l2rel(got, v32)
    print(f"[{what}] to float64: kernel {e_k:.3e} oracle {e_or:.3e}; l2rel to the oracle {rel:.3e}")
    assert e_k <= 3.0 * e_or + 1e-6, (what, e_k, e_or)
    assert rel < VLAD_RTOL, (what, rel)
    return e_k / max(e_or, 1e-30), rel


# ------------------------------------------------------------------------------------- 1. ops.vlad(mode="soft")
@pytest.mark.parametrize("case", range(len(SOFT_CASES)), ids=SOFT_IDS)
def test_vlad_soft_ragged_vs_oracle(case):
    """One ragged batch per case as a list, every flag pair, temperatures 1 / 7.5 / 50: each image against the oracle and
    float64; the empty image's row is exactly zero; the packed (tokens, offsets) pair and a second call give the same bits
    (the kernel's sums are sequential)."""
    from anyloc_amd import ops
    K, D, counts = SOFT_CASES[case]
    centers, imgs = _inputs(K, D, counts)
    c_dev = centers.to(DEV)
    parts = [t.to(DEV) for t in imgs]
    packed = torch.cat(parts, 0)
    offsets = torch.tensor([0] + list(counts), dtype=torch.int64).cumsum(0).to(DEV)
    worst_ratio = worst_rel = 0.0
    for temp in TEMPS:
        for nd, intra in FLAGS:
            out = ops.vlad(parts, c_dev, mode="soft", soft_temp=temp, norm_descs=nd, intra_norm=intra)
            assert tuple(out.shape) == (len(counts), K * D)
            out = out.clone()
            for i, n in enumerate(counts):
                if n == 0:
                    assert float(out[i].abs().max()) == 0.0
                    continue
                v32, _, v64, _ = _soft_refs(case, i, temp, nd, intra)
                ratio, rel = _judge(out[i], v32, v64, f"soft {SOFT_IDS[case]} img {i} temp {temp} norm_descs {nd} intra {intra}")
                worst_ratio, worst_rel = max(worst_ratio, ratio), max(worst_rel, rel)
            same = ops.vlad((packed, offsets), c_dev, mode="soft", soft_temp=temp, norm_descs=nd, intra_norm=intra)
            assert torch.equal(same, out), "packed (tokens, offsets) pair differs from the list"
            again = ops.vlad(parts, c_dev, mode="soft", soft_temp=temp, norm_descs=nd, intra_norm=intra)
            assert torch.equal(again, out), "second call differs from the first"
    print(f"[soft {SOFT_IDS[case]}] worst kernel / oracle distance to float64: {worst_ratio:.2f}; worst l2rel to the oracle: "
          f"{worst_rel:.3e}")


@pytest.mark.parametrize("K,D", [(33, 68), (64, 128)])
def test_vlad_soft_all_images_empty(K, D):
    from anyloc_amd import ops
    centers = _inputs(K, D, (8,))[0].to(DEV)
    for nd, intra in FLAGS:
        out = ops.vlad([torch.empty(0, D), torch.empty(0, D)], centers, mode="soft", soft_temp=7.5, norm_descs=nd,
                       intra_norm=intra)
        assert tuple(out.shape) == (2, K * D)
        assert float(out.abs().max()) == 0.0


# ------------------------------------------------------------------------------------- 2. ops.vlad_soft_weights
@pytest.mark.parametrize("case", range(len(SOFT_CASES)), ids=SOFT_IDS)
def test_soft_weights_vs_float64(case):
    """The first image of every soft case: shape [N, K], rows sum to 1, the zero row is uniform, and every weight as close
    to the float64 soft-max as the oracle's."""
    from anyloc_amd import ops
    K, D, counts = SOFT_CASES[case]
    centers, imgs = _inputs(K, D, counts)
    x = imgs[0]
    N = x.shape[0]
    worst_ratio = 0.0
    for temp in TEMPS:
        w = ops.vlad_soft_weights(x.to(DEV), centers.to(DEV), temp)
        assert tuple(w.shape) == (N, K) and w.dtype == torch.float32
        w = w.cpu()
        assert float((w.double().sum(dim=1) - 1.0).abs().max()) <= 1e-6
        assert N > 5 and float(x[3].abs().max()) == 0.0
        assert bool((w[3] == w[3, 0]).all()) and abs(float(w[3, 0]) - 1.0 / K) <= 2.0 ** -23 / K
        _, w32, _, w64 = _soft_refs(case, 0, temp, True, True)
        e_or = float((w32.double() - w64).abs().max())
        e_k = float((w.double() - w64).abs().max())
        print(f"[weights {SOFT_IDS[case]} temp {temp}] largest error to float64: kernel {e_k:.3e} oracle {e_or:.3e}")
        assert e_k <= 3.0 * e_or + 1e-6, (temp, e_k, e_or)
        worst_ratio = max(worst_ratio, e_k / max(e_or, 1e-30))
    print(f"[weights {SOFT_IDS[case]}] worst kernel / oracle error to float64: {worst_ratio:.2f}")


# ------------------------------------------------------------------------------------- 3. ops.vlad_assigned
@pytest.mark.parametrize("K,D,N", LABEL_CASES)
def test_vlad_assigned_labels_vs_oracle(K, D, N):
    """Labels drawn uniformly at random (some clusters stay unused), every flag pair, against the oracle and float64 under
    the same labels -- not against the library's own choice.  K > 128 runs accumulate_kernel on half-width slices."""
    from anyloc_amd import ops
    centers, (x,) = _inputs(K, D, (N,))
    labels = torch.randint(0, K, (N,), generator=torch.Generator().manual_seed(K + N))
    unused = sorted(set(range(K)) - set(labels.tolist()))
    worst_ratio = worst_rel = 0.0
    for nd, intra in FLAGS:
        out = ops.vlad_assigned(x.to(DEV), centers.to(DEV), labels=labels.to(DEV), norm_descs=nd, intra_norm=intra)
        assert tuple(out.shape) == (K * D,)
        v32 = vlad_ref.vlad_hard(x, centers, nd, intra, labels=labels)[0]
        v64 = hard_vlad_f64(x, centers, labels, nd, intra)
        ratio, rel = _judge(out, v32, v64, f"labels K{K} D{D} N{N} norm_descs {nd} intra {intra}")
        worst_ratio, worst_rel = max(worst_ratio, ratio), max(worst_rel, rel)
        assert not unused or float(out.reshape(K, D)[unused].abs().max()) == 0.0
    print(f"[labels K{K} D{D} N{N}] worst kernel / oracle distance to float64: {worst_ratio:.2f}; worst l2rel to the oracle: "
          f"{worst_rel:.3e}")
    none = ops.vlad_assigned(torch.empty(0, D, device=DEV), centers.to(DEV), labels=torch.empty(0, dtype=torch.int64, device=DEV))
    assert tuple(none.shape) == (K * D,) and float(none.abs().max()) == 0.0


@pytest.mark.parametrize("K,D,N", WEIGHT_CASES)
def test_vlad_assigned_weights_vs_oracle(K, D, N):
    """Dense [N, K] weights, sparse and not summing to one per row: the kernel reads them with row stride K where
    ops.vlad(mode="soft") reads its own with stride kpad."""
    from anyloc_amd import ops
    centers, (x,) = _inputs(K, D, (N,))
    g = torch.Generator().manual_seed(K + D + N)
    w = torch.rand(N, K, generator=g) * (torch.rand(N, K, generator=g) < 0.3)
    worst_ratio = worst_rel = 0.0
    for nd, intra in ((True, True), (False, False)):
        out = ops.vlad_assigned(x.to(DEV), centers.to(DEV), soft=w.to(DEV), norm_descs=nd, intra_norm=intra)
        v32 = vlad_ref.vlad_soft(x, centers, 1.0, nd, intra, weights=w)[0]
        v64 = _soft_f64(x, centers, w, nd, intra)
        ratio, rel = _judge(out, v32, v64, f"given weights K{K} D{D} N{N} norm_descs {nd} intra {intra}")
        worst_ratio, worst_rel = max(worst_ratio, ratio), max(worst_rel, rel)
    print(f"[given weights K{K} D{D} N{N}] worst kernel / oracle distance to float64: {worst_ratio:.2f}; worst l2rel to the "
          f"oracle: {worst_rel:.3e}")


def test_vlad_assigned_own_soft_weights_match_soft_mode():
    """vlad_assigned fed the library's own weights == ops.vlad(mode="soft"), at K = 43: strides 43 and 64."""
    from anyloc_amd import ops
    K, D, N = 43, 200, 129
    centers, (x,) = _inputs(K, D, (N,))
    x_dev, c_dev = x.to(DEV), centers.to(DEV)
    for temp in (2.0, 50.0):
        w = ops.vlad_soft_weights(x_dev, c_dev, temp)
        assert tuple(w.shape) == (N, K)
        full = ops.vlad(x_dev[None], c_dev, mode="soft", soft_temp=temp)
        assert l2rel(ops.vlad_assigned(x_dev, c_dev, soft=w), full[0]) < 1e-6


# ------------------------------------------------------------------------------------- 4. ops.kmeans_update
def test_kmeans_update_empty_clusters():
    """sums / counts of an assignment that leaves two clusters empty: their new centres are exactly 0 (fpk: 0/0 -> NaN -> 0),
    every other entry is one fp32 division (within one ulp, a relative 2^-23, of the float64 quotient), and the error is the
    float64 sum of the fp32 squares (new - old)^2 up to the re-ordering of 900 float64 terms (1e-12)."""
    check_kmeans_update(9, 100, 400, [2, 6])


def check_kmeans_update(K, D, n, empty):
    """``n`` rows dealt at random over the K clusters but those of ``empty``: ops.kmeans_update against the expressions above."""
    from anyloc_amd import ops
    g = torch.Generator().manual_seed(K * D)
    x = torch.randn(n, D, generator=g)
    live = torch.tensor([k for k in range(K) if k not in empty])
    closest = live[torch.randint(0, len(live), (n,), generator=g)]
    onehot = (closest[None, :] == torch.arange(K)[:, None]).to(x.dtype)
    sums, counts = onehot @ x, onehot.sum(-1)                    # as oracle/fpk_kmeans.py forms them
    assert bool((counts[empty] == 0).all()) and float(sums[empty].abs().max()) == 0.0 and int((counts > 0).sum()) == K - len(empty)
    old = torch.randn(K, D, generator=g)
    new, err = ops.kmeans_update(sums.to(DEV), counts.to(DEV), old.to(DEV))
    new, err = new.cpu(), float(err.cpu())
    assert tuple(new.shape) == (K, D) and bool(torch.isfinite(new).all())
    assert float(new[empty].abs().max()) == 0.0
    used = counts > 0
    q = sums[used].double() / counts[used].double()[:, None]
    assert bool(((new[used].double() - q).abs() <= 2.0 ** -23 * q.abs()).all())
    d = new - old                                                # fp32, as kmeans_update_kernel forms it
    want = float((d * d).double().sum())
    assert abs(err - want) <= 1e-12 * want, (err, want)
