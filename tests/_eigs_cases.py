"""The matrices and the checks that tests/test_eigs_cpu.py and tests/test_gpu_eigs.py share (not a test module): five
symmetric matrices  S = V diag(lambda) V^T  with a seeded orthogonal V and a known spectrum, their LAPACK decomposition
(computed once), and the properties a result of ``eigs.sym_topk`` must have -- all of that on the CPU in float64; and
``decaying``, the fp32 data of the PCA tests (tests/test_gpu_pca.py, tests/test_gpu_eigs.py), drawn in float64 on the CPU."""
import math

import torch

TOL = 1e-11


def _special(m):
    head = torch.tensor([10, 9, 8, 7, 7, 7, 6, 5, 4.5, 4, 3.5, 3, 2.5, 2.2, 2, 1.8], dtype=torch.float64)
    return torch.cat([head, 1.5 * 0.95 ** torch.arange(m - head.numel(), dtype=torch.float64)])


# name -> (m, k, spectrum(m))
SPECTRA = {
    "geometric_0.9": (300, 24, lambda m: 0.9 ** torch.arange(m, dtype=torch.float64)),
    "geometric_0.99": (700, 40, lambda m: 0.99 ** torch.arange(m, dtype=torch.float64)),
    "geometric_0.97_odd_m": (509, 32, lambda m: 0.97 ** torch.arange(m, dtype=torch.float64)),
    "harmonic": (600, 32, lambda m: 1.0 / (1.0 + torch.arange(m, dtype=torch.float64))),
    "cluster_7_7_7": (400, 16, _special),
}
_cache = {}


def orthogonal(m, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.linalg.qr(torch.randn(m, m, generator=g, dtype=torch.float64))[0]


def case(name):
    """-> dict(S, m, k, lam [m] descending and vec [m, m] of torch.linalg.eigh): built once, never modified."""
    if name not in _cache:
        m, k, spectrum = SPECTRA[name]
        v = orthogonal(m, seed=100 + len(name))
        s = (v * spectrum(m)) @ v.t()
        s = 0.5 * (s + s.t())
        lam, vec = torch.linalg.eigh(s)
        _cache[name] = dict(S=s, m=m, k=k, lam=lam.flip(0), vec=vec.flip(1))
    return _cache[name]


def decaying(n, f, seed, decay=0.9, rank=None):
    """[n, f] fp32 rows with singular values 10 * decay^j (a well-separated spectrum) around a common offset: the PCA tests' data"""
    g = torch.Generator().manual_seed(seed)
    r = min(n, f) if rank is None else rank
    q1, _ = torch.linalg.qr(torch.randn(n, r, generator=g, dtype=torch.float64))
    q2, _ = torch.linalg.qr(torch.randn(f, r, generator=g, dtype=torch.float64))
    s = 10.0 * decay ** torch.arange(r, dtype=torch.float64)
    return ((q1 * s) @ q2.t() + 0.3 * torch.randn(1, f, generator=g, dtype=torch.float64)).float()


def rank_deficient(m=300, rank=20):
    v = orthogonal(m, seed=7)[:, :rank]
    s = (v * (10.0 * 0.9 ** torch.arange(rank, dtype=torch.float64))) @ v.t()
    return 0.5 * (s + s.t())


def check_pairs(name, lam, vec_t, n_iter, tol=TOL):
    """The assertions on one result, recomputed in float64 on the CPU from the returned pairs."""
    from anyloc_amd import eigs
    c = case(name)
    S, m, k, ref, vref = c["S"], c["m"], c["k"], c["lam"], c["vec"]
    lam, q = lam.cpu(), vec_t.cpu()
    assert lam.shape == (k,) and q.shape == (k, m) and lam.dtype == q.dtype == torch.float64
    l0 = float(ref[0])
    assert bool((lam[:-1] >= lam[1:]).all())                                            # descending
    res = (q @ S - lam[:, None] * q).norm(dim=1)
    print(f"{name}: n_iter {n_iter}, max residual / lambda_0 {float(res.max()) / l0:.2e}")
    assert float(res.max()) <= tol * l0                                                 # 1. residuals
    err = (lam - ref[:k]).abs().max()
    assert float(err) <= tol * l0 + 1e-13 * l0, float(err)                              # 2. position by position
    orth = (q @ q.t() - torch.eye(k, dtype=torch.float64)).abs().max()
    assert float(orth) <= 1e-12, float(orth)                                            # 3. orthonormal
    # 4. separated eigenvectors within the Davis-Kahan bound of their residual
    gaps = torch.minimum(torch.cat([torch.tensor([math.inf], dtype=torch.float64), ref[:-1] - ref[1:]])[:k], (ref[:-1] - ref[1:])[:k])
    checked = 0
    for j in range(k):
        gap = float(gaps[j])
        if gap <= 1e-9 * l0:
            continue
        v = vref[:, j]
        d = min(float((q[j] - v).norm()), float((q[j] + v).norm()))
        assert d <= 2 * tol * l0 / gap + 1e-12, (j, d, gap)
        checked += 1
    # 5. a cluster of equal eigenvalues: the invariant subspace (projector), not the vectors
    if name == "cluster_7_7_7":
        idx = [3, 4, 5]
        assert checked == k - 3
        p_got = q[idx].t() @ q[idx]
        p_ref = vref[:, idx] @ vref[:, idx].t()
        gap = 1.0                                                                       # 8 - 7 and 7 - 6
        assert float((p_got - p_ref).abs().max()) <= 2 * math.sqrt(3) * tol * l0 / gap + 1e-12
    else:
        assert checked == k
    # 6. pair j converges at the rate lambda_{b+1} / lambda_j, slowest for j = k; the slack covers the check interval
    b = eigs.block_size(k)
    rate = float(ref[b] / ref[k - 1])
    assert n_iter <= 1.5 * math.log(tol) / math.log(rate) + 8, (n_iter, rate)
