"""The leading eigenpairs of a symmetric positive semi-definite matrix by blocked subspace iteration with Rayleigh-Ritz
(the truncated decomposition behind ``PCA(solver="subspace")``; the reference's sklearn PCA takes every pair from LAPACK,
``utilities.py:561-564``).

A block of vectors is stored as ROWS, ``Qt [b, m]`` float64 row-major, so that every large product of the iteration has the
form  C[i, j] = sum_c A(i, c) B(j, c)  of ``ops.gemm_nt_f64`` (csrc/pca_f64.hip, the float64 matrix cores) on operands read
where they lie:

* apply          Yt = Qt S            A = Qt, B = S (symmetric), both contiguous along c
* orthonormalise CholQR, twice:       W = Yt Yt^T (symmetric product), L = chol(W), Qt = L^-1 Yt -- a product of the explicit
                                      b x b inverse with B(j, c) = Yt[c, j], contiguous along its row index
* Rayleigh-Ritz  T = Qt (Qt S)^T      at a growing interval; eigh(T) rotates Qt and Qt S, the residuals
                                      |S q_j - theta_j q_j| of the leading k rows decide convergence

The b x b Cholesky factor, its inverse and the eigendecomposition of T are ``torch.linalg`` calls on device b x b matrices
(O(b^3), under 1 % of the flops); the host reads one small status vector per Rayleigh-Ritz check, nothing in between.
"""
import math

import torch

# CholQR forms W = Yt Yt^T, which squares the condition number of the block: the factor is meaningful while
# cond(Yt)^2 eps64 << 1.  diag(L) brackets the singular values of Yt from inside (max diag <= s_max, min diag >= s_min), so
# max / min of it is a lower bound of cond(Yt); above 1e6 (cond^2 eps64 ~ 1e-4) the block has lost a direction --
# a matrix of rank below b -- and the solver gives up instead of orthonormalising noise.
_COND_MAX = 1e6


def block_size(k):
    """Rows of the iterated block for k wanted pairs: k plus a guard of max(16, k // 4), rounded up to the 16 rows of an MFMA
    tile.  Pair j converges at the rate lambda_{b+1} / lambda_j, so the guard buys the ratio for j = k."""
    return 16 * math.ceil((k + max(16, k // 4)) / 16)


def eligible(m, k):
    """The truncated solver pays off, and its block leaves room, when three blocks fit in the matrix."""
    return k >= 1 and 3 * block_size(k) <= m


def _hip_products(a, b, symmetric=False):
    from . import ops
    return ops.gemm_nt_f64(a, b, symmetric=symmetric)


def _cholqr(nt, yt, bad):
    """One CholQR pass on the rows of yt -> (orthonormal rows spanning the same space, bad flag updated on the device)."""
    w = nt(yt, yt, symmetric=True)
    l, info = torch.linalg.cholesky_ex(w)
    d = l.diagonal()
    # (comparisons with NaN are False: a non-finite factor raises the flag as well)
    bad = bad | (info != 0) | ~(d.min() * _COND_MAX > d.max())
    linv = torch.linalg.solve_triangular(l, torch.eye(l.shape[0], dtype=l.dtype, device=l.device), upper=False)
    return nt(linv, yt.t()), bad


def sym_topk(S, k, tol=1e-11, max_iter=3000, seed=0, _products=None):
    """-> (lam [k] descending, vec_t [k, m] with the eigenvectors as rows, n_iter), or None when the solver does not apply
    (shape not ``eligible``) or broke down (a Cholesky factor failed or lost a direction, a non-finite value, no
    convergence within ``max_iter``): the caller then runs the full decomposition.

    Converged when every leading residual |S q_j - theta_j q_j|_2, j < k, is at most tol * theta_0.  The start block is
    ``torch.randn`` from a generator seeded on S's device: the same shape and seed give the same bits.
    ``_products(a, b, symmetric=False) = a @ b.t()`` is the product backend (default: the HIP kernel, no CPU fallback)."""
    nt = _hip_products if _products is None else _products
    m = S.shape[0]
    if S.dim() != 2 or S.shape[1] != m or S.dtype != torch.float64:
        raise ValueError(f"sym_topk needs a square float64 matrix, got {S.dtype} {tuple(S.shape)}")
    if not eligible(m, k):
        return None
    b = block_size(k)
    S = S.contiguous()
    gen = torch.Generator(device=S.device).manual_seed(seed)
    bad = torch.zeros((), dtype=torch.bool, device=S.device)
    qt = torch.randn(b, m, generator=gen, dtype=torch.float64, device=S.device)
    qt, bad = _cholqr(nt, qt, bad)
    yt = None                                             # S applied to the current block, when a check left it behind
    it, check_at = 0, 4
    while it < max_iter:
        if yt is None:
            yt = nt(qt, S)
        qt, bad = _cholqr(nt, yt, bad)
        qt, bad = _cholqr(nt, qt, bad)
        yt = None
        it += 1
        if it < check_at and it < max_iter:
            continue
        # Rayleigh-Ritz on the block: T = Q^T S Q, rotate to its eigenvectors, largest first
        zt = nt(qt, S)
        t = nt(qt, zt)
        try:
            theta, u = torch.linalg.eigh(0.5 * (t + t.t()))
        except RuntimeError:                              # (torch.linalg.LinAlgError: no convergence on a non-finite T)
            return None
        theta, ut = theta.flip(0), u.flip(1).t().contiguous()
        qt, zt = nt(ut, qt.t()), nt(ut, zt.t())          # (S is linear: the rotated S q_j need no second apply)
        res = (zt[:k] - theta[:k, None] * qt[:k]).norm(dim=1).max()
        status = torch.stack([bad.double(), res, theta[0]]).tolist()           # the one host read of the check
        if status[0] != 0.0 or not all(math.isfinite(v) for v in status) or not status[2] > 0.0:
            return None
        if status[1] <= tol * status[2]:
            return theta[:k].clone(), qt[:k].clone(), it
        yt = zt
        check_at = it + max(4, it // 4)
    return None
