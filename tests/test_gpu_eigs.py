"""The truncated PCA fit on the device (``pytest -m gpu``): ``ops.gemm_nt_f64`` (csrc/pca_f64.hip with float64 operands, both
16-byte fetch modes and the element-wise one) against a CPU float64 matmul, ``eigs.sym_topk`` on the HIP products with the
assertions of tests/test_eigs_cpu.py evaluated on the CPU, ``PCA(solver="subspace")`` against sklearn's full SVD, every
fallback to the full solver, and the stream contract of both."""
import numpy as np
import pytest
import torch

import _eigs_cases as E

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rand64(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(DEV)


def _offset_by_one(t):
    """The same values in storage that starts one element (8 bytes) past a 16-byte boundary, same strides."""
    flat = torch.empty(t.untyped_storage().nbytes() // 8 + 1, dtype=torch.float64, device=t.device)
    view = flat[1:].as_strided(t.shape, t.stride())
    view.copy_(t)
    assert view.data_ptr() % 16 == 8
    return view


def _product(a, b, symmetric=False):
    """ops.gemm_nt_f64 on device operands read with their strides, against the CPU float64 matmul of the same values."""
    from anyloc_amd import ops
    want = a.cpu() @ b.cpu().t()
    got = ops.gemm_nt_f64(a, b, symmetric=symmetric)
    assert got.dtype == torch.float64 and got.shape == want.shape and got.is_contiguous()
    err, bar = float((got.cpu() - want).abs().max()), 1e-13 * float(want.abs().max()) * a.shape[1] ** 0.5
    print(f"gemm_nt_f64 {tuple(a.shape)} x {tuple(b.shape)}^T: max err {err:.2e}, bar {bar:.2e}")
    assert err <= bar
    return got


def test_gemm_nt_f64_vector_mode_along_c():
    a, b = _rand64(48, 512, seed=1), _rand64(512, 512, seed=2)
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
    got = _product(a, b)
    # the 16-byte fetch changes how an element reaches LDS, not the order of the sums: the element-wise fetch of the same
    # values (operands moved off the 16-byte boundary) gives the same bits
    assert torch.equal(_product(_offset_by_one(a), _offset_by_one(b)), got)


def test_gemm_nt_f64_scalar_fallback_odd_extent_and_offset_view():
    a, b = _rand64(48, 509, seed=3), _rand64(509, 509, seed=4)
    got = _product(a, b)                                                  # odd K and row stride
    assert torch.equal(_product(_offset_by_one(a), b), got)               # one operand off the boundary
    wide = _rand64(48, 513, seed=5)
    _product(wide[:, 1:], _rand64(512, 512, seed=6))                      # a view offset by one element, even extent


def test_gemm_nt_f64_vector_mode_along_r():
    a, bt = _rand64(32, 48, seed=7), _rand64(48, 512, seed=8)
    b = bt.t()                                                            # [512, 48], strides (1, 512): no copy
    assert b.stride() == (1, 512) and b.data_ptr() == bt.data_ptr()
    got = _product(a, b)
    assert torch.equal(_product(a, _offset_by_one(bt).t()), got)          # element-wise fetch, same bits
    assert torch.equal(_product(a, b.contiguous()), got)                  # B contiguous along c instead


def test_gemm_nt_f64_tile_edges():
    _product(_rand64(129, 130, seed=9), _rand64(257, 130, seed=10))
    bt = _rand64(130, 258, seed=11)
    _product(_rand64(129, 130, seed=9), bt.t())                           # 258 rows along r, 16-byte fetches
    _product(_rand64(129, 130, seed=9), bt.t()[:257])                     # odd extent: element-wise


def test_gemm_nt_f64_symmetric_is_mirrored():
    a = _rand64(64, 300, seed=12)
    c = _product(a, a, symmetric=True)
    assert torch.equal(c, c.t())
    big = _rand64(300, 64, seed=13)
    c = _product(big, big, symmetric=True)                                # three tile rows: paired rows and the middle one
    assert torch.equal(c, c.t())
    col = big.t().contiguous().t()                                        # the same values stored column-major
    assert torch.equal(_product(col, col, symmetric=True), c)


def test_gemm_nt_f64_rejects_what_it_cannot_serve():
    from anyloc_amd import ops
    a = _rand64(8, 16, seed=14)
    with pytest.raises(ValueError):
        ops.gemm_nt_f64(a.float(), a)
    with pytest.raises(ValueError):
        ops.gemm_nt_f64(a, _rand64(8, 18, seed=15))
    with pytest.raises(ValueError):
        ops.gemm_nt_f64(a, a.clone(), symmetric=True)


@pytest.mark.parametrize("name", list(E.SPECTRA))
def test_sym_topk_on_the_device(name):
    from anyloc_amd import eigs
    c = E.case(name)
    S = c["S"].to(DEV)
    got = eigs.sym_topk(S, c["k"], tol=E.TOL)
    assert got is not None
    lam, vec_t, n_iter = got
    assert lam.is_cuda and vec_t.is_cuda
    E.check_pairs(name, lam, vec_t, n_iter)
    again = eigs.sym_topk(S, c["k"], tol=E.TOL)
    assert torch.equal(again[0], lam) and torch.equal(again[1], vec_t) and again[2] == n_iter


def test_sym_topk_rank_below_the_block_returns_none_on_the_device():
    from anyloc_amd import eigs
    assert eigs.sym_topk(E.rank_deficient(300, 20).to(DEV), 32) is None


_sk = {}


def _sklearn_fit(shape, k, whiten):
    """sklearn's full float64 SVD of the case's data, fitted once per (shape, k, whiten)."""
    from sklearn.decomposition import PCA as SkPCA
    key = (shape, k, whiten)
    if key not in _sk:
        x = E.decaying(*shape, seed=1, rank=100)
        _sk[key] = (x, SkPCA(k, svd_solver="full", whiten=whiten).fit(x.double().numpy()))
    return _sk[key]


@pytest.mark.parametrize("shape,k", [((600, 2048), 32), ((3000, 640), 24)])
@pytest.mark.parametrize("whiten", [False, True])
def test_pca_subspace_matches_sklearn_full_svd(shape, k, whiten):
    from anyloc_amd import pca
    x, sk = _sklearn_fit(shape, k, whiten)
    xd = x.to(DEV)
    ours = pca.PCA(k, whiten=whiten, solver="subspace").fit(xd)
    assert ours.solver_used_ == "subspace" and ours.n_iter_ > 0
    err = np.abs(ours.components_.cpu().numpy() - sk.components_).max()
    print(f"PCA subspace {shape} k={k} whiten={whiten}: n_iter {ours.n_iter_}, components max err {err:.2e}")
    assert err < 2e-5
    assert np.allclose(ours.explained_variance_.cpu().numpy(), sk.explained_variance_, rtol=2e-5)
    full = pca.PCA(k, whiten=whiten).fit(xd)
    assert full.solver_used_ == "full" and full.n_iter_ == 0
    # the total variance from the trace against the sum of all eigenvalues of the same float64 matrix
    assert torch.allclose(ours.explained_variance_ratio_.double(), full.explained_variance_ratio_.double(), rtol=1e-10, atol=0)
    y = E.decaying(33, shape[1], seed=2, rank=33).to(DEV)
    want = sk.transform(y.double().cpu().numpy())
    tol = 5e-4 if whiten else 1e-4                       # (the bars of test_pca_matches_sklearn_full_svd)
    assert np.abs(ours.transform(y).cpu().numpy() - want).max() < tol * np.abs(want).max()


def test_pca_subspace_falls_back_on_rank_deficient_data():
    from anyloc_amd import pca
    x = E.decaying(600, 2048, seed=1, rank=20).to(DEV)
    sub, full = pca.PCA(32, solver="subspace").fit(x), pca.PCA(32).fit(x)
    assert sub.solver_used_ == "full" and sub.n_iter_ == 0
    assert torch.equal(sub.components_, full.components_) and torch.equal(sub.explained_variance_, full.explained_variance_)


def test_pca_subspace_falls_back_on_an_ineligible_shape():
    from anyloc_amd import eigs, pca
    x = E.decaying(100, 2048, seed=1, rank=60).to(DEV)
    assert not eigs.eligible(100, 32)
    sub, full = pca.PCA(32, solver="subspace").fit(x), pca.PCA(32).fit(x)
    assert sub.solver_used_ == "full" and full.solver_used_ == "full"
    assert torch.equal(sub.components_, full.components_)
    with pytest.raises(ValueError):
        pca.PCA(32, solver="arpack")


def test_reduce_pca_maps_arpack_to_the_subspace_solver(monkeypatch):
    import utilities
    from anyloc_amd import eigs
    calls = []
    real = eigs.sym_topk

    def spy(*a, **kw):
        calls.append(a[1])
        return real(*a, **kw)
    monkeypatch.setattr(eigs, "sym_topk", spy)
    x, y = E.decaying(600, 2048, seed=1, rank=100), E.decaying(33, 2048, seed=2, rank=33)
    a_full, b_full = utilities.reduce_pca(x.numpy(), y.numpy(), 32, svd_solver="full")
    assert calls == []
    utilities.reduce_pca(x.numpy(), y.numpy(), 32)
    utilities.reduce_pca(x.numpy(), y.numpy(), 32, svd_solver="randomized")
    assert calls == []
    a_sub, b_sub = utilities.reduce_pca(x.numpy(), y.numpy(), 32, svd_solver="arpack")
    assert calls == [32]
    scale = np.abs(a_full).max()
    assert isinstance(a_sub, np.ndarray) and np.abs(a_sub - a_full).max() < 1e-4 * scale and np.abs(b_sub - b_full).max() < 1e-4 * scale
    # the low_factor > 0 branch needs every component: it stays on the full solver
    utilities.reduce_pca(x[:, :256].numpy(), y[:, :256].numpy(), 32, low_factor=0.25, svd_solver="arpack")
    assert calls == [32]


def test_gemm_nt_f64_on_a_side_stream():
    import _stream_harness as H
    from anyloc_amd import ops
    a, s = _rand64(48, 512, seed=20), _rand64(512, 512, seed=21)
    H.run_case("gemm_nt_f64_48x512x512", lambda a, s: (ops.gemm_nt_f64(a, s), ops.gemm_nt_f64(a, a, symmetric=True),
                                                      ops.gemm_nt_f64(a[:32, :48], s[:48].t())), [a, s], asynchronous=True)


def test_sym_topk_on_a_side_stream():
    """The solver reads a status vector back at every Rayleigh-Ritz check (a syncing op); everything it enqueues -- the
    start block, the products, the small torch.linalg steps -- must be on the caller's stream."""
    import _stream_harness as H
    from anyloc_amd import eigs
    S = E.case("geometric_0.9")["S"].to(DEV)
    H.run_case("sym_topk_300_k24", lambda S: eigs.sym_topk(S, 24)[:2], [S], asynchronous=False)
