"""``eigs.sym_topk`` (blocked subspace iteration with Rayleigh-Ritz, the truncated decomposition of ``PCA(solver="subspace")``):
its control flow on the CPU, with the three large products served by float64 ``torch.matmul`` through the private
``_products`` parameter (the product's own backend is the HIP kernel and has no CPU fallback; tests/test_gpu_eigs.py runs
that).  Matrices, references and assertions: tests/_eigs_cases.py."""
import pytest
import torch

import _eigs_cases as E


def matmul_products(a, b, symmetric=False):
    return a @ b.t()


@pytest.mark.parametrize("name", list(E.SPECTRA))
def test_sym_topk_five_spectra(name):
    from anyloc_amd import eigs
    c = E.case(name)
    got = eigs.sym_topk(c["S"], c["k"], tol=E.TOL, _products=matmul_products)
    assert got is not None
    lam, vec_t, n_iter = got
    E.check_pairs(name, lam, vec_t, n_iter)
    again = eigs.sym_topk(c["S"], c["k"], tol=E.TOL, _products=matmul_products)           # 7. deterministic
    assert torch.equal(again[0], lam) and torch.equal(again[1], vec_t) and again[2] == n_iter
    other = eigs.sym_topk(c["S"], c["k"], tol=E.TOL, seed=1, _products=matmul_products)   # (and the seed is honoured)
    assert not torch.equal(other[1], vec_t)


def test_rank_below_the_block_returns_none():
    """A rank-20 matrix with k = 32: the 48-row block loses directions, the Cholesky factor breaks down, the caller falls back."""
    from anyloc_amd import eigs
    assert eigs.sym_topk(E.rank_deficient(300, 20), 32, _products=matmul_products) is None


def test_no_convergence_and_non_finite_return_none():
    from anyloc_amd import eigs
    c = E.case("geometric_0.99")
    assert eigs.sym_topk(c["S"], c["k"], max_iter=8, _products=matmul_products) is None
    bad = c["S"].clone()
    bad[5, 5] = float("nan")
    assert eigs.sym_topk(bad, c["k"], _products=matmul_products) is None


@pytest.mark.parametrize("m,k,b,ok", [(300, 24, 48, True), (144, 24, 48, True), (143, 24, 48, False), (96, 1, 32, True), (95, 1, 32, False),
                                      (10000, 512, 640, True), (1920, 512, 640, True), (1919, 512, 640, False), (600, 32, 48, True),
                                      (700, 40, 64, True), (400, 16, 32, True), (640, 24, 48, True), (100, 64, 80, False)])
def test_block_size_and_eligibility(m, k, b, ok):
    from anyloc_amd import eigs
    assert eigs.block_size(k) == b and eigs.eligible(m, k) is ok
    if not ok:                                                   # the solver itself declines, whatever the backend
        assert eigs.sym_topk(torch.eye(m, dtype=torch.float64), k, _products=matmul_products) is None


def test_default_backend_is_the_hip_kernel():
    """No CPU fallback: without a GPU the default products raise instead of quietly running torch."""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from anyloc_amd import _lib, eigs
    with pytest.raises(_lib.AnylocHipError):
        eigs.sym_topk(E.case("geometric_0.9")["S"], 24)


def test_gemm_nt_f64_entry_validates_without_a_gpu():
    """The additive C entry: declared, exported, bound, and its arguments are checked before any HIP call."""
    import ctypes
    from anyloc_amd import _lib, build
    build.build_library(verbose=False)
    lib = _lib.load()
    assert "anyloc_gemm_nt_f64" in _lib.SIGNATURES
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)
    assert lib.anyloc_gemm_nt_f64(None, 4, 1, p, 4, 1, 4, 4, 4, 0, p, None) == -1 and b"gemm_nt_f64" in lib.anyloc_last_error()
    assert lib.anyloc_gemm_nt_f64(p, 0, 1, p, 4, 1, 4, 4, 4, 0, p, None) == -1 and b"strides" in lib.anyloc_last_error()
    assert lib.anyloc_gemm_nt_f64(p, 4, 1, p, 1, 4, 4, 4, 4, 1, p, None) == -1 and b"symmetric" in lib.anyloc_last_error()
    assert lib.anyloc_gemm_nt_f64(p, 4, 1, p, 4, 1, 4, 0, 4, 0, p, None) == -1 and b"bad shape" in lib.anyloc_last_error()
