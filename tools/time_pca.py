"""The PCA fit on the device, timed (synchronised wall time; one process, one mode per call):

    python tools/time_pca.py products [n] [f] [k]      the float64 products of csrc/pca_f64.hip at the reference's descriptor
                                                       width against a float64 copy + torch.matmul, and one small PCA.fit
    python tools/time_pca.py fit SOLVER [n] [f] [k]    PCA(k, solver=SOLVER).fit on n x f, split into Gram / scatter, eigen
                                                       step and the rest (back-projection, signs); SOLVER = full | subspace.
                                                       subspace: n_iter_, the three products of one iteration timed alone,
                                                       and lambda_{b+1} / lambda_k of the data when --ratio is given (costs
                                                       a full eigvalsh).  --save FILE / --against FILE: keep the fit's
                                                       components and singular values / compare with a kept fit.
    python tools/time_pca.py eigh M                    torch.linalg.eigh of a random symmetric M x M float64 matrix alone (to
                                                       size a time limit before a large full fit)

The data: rows of unit norm around a common offset with a decaying spectrum (``--decay``, default 0.995 per axis on top of
white noise) -- synthetic: no VPR dataset is available offline, so iteration counts on real VLAD spectra are not measured here.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from anyloc_amd import eigs, ops, pca  # noqa: E402

dev = "cuda"


def timed(fn, reps=2):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def vlad_like(n, f, decay, seed=0):
    """[n, f] fp32 rows of unit norm: white noise + a common offset + min(n, f, 2048) directions of geometrically decaying weight."""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(n, f, generator=g, device=dev) + 0.5
    r = min(n, f, 2048)
    coef = torch.randn(n, r, generator=g, device=dev) * (40.0 * decay ** torch.arange(r, device=dev, dtype=torch.float32))
    rows = max(1, (256 << 20) // (4 * f))
    basis = torch.randn(r, f, generator=g, device=dev)
    for r0 in range(0, n, rows):
        x[r0:r0 + rows] += coef[r0:r0 + rows] @ basis
    return torch.nn.functional.normalize(x, dim=1)


def products(n, f, k):
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.nn.functional.normalize(torch.randn(n, f, generator=g, device=dev) + 0.5, dim=1)     # VLAD-like rows of unit norm
    mean = x.mean(dim=0, dtype=torch.float64)
    t_own, gram = timed(lambda: ops.pca_gram_f64(x, mean, 0))
    flop = n * n * f                                    # the upper tiles only: 2 n^2 f / 2
    print(f"anyloc_pca_gram_f64 {n} x {f}: {t_own * 1e3:.1f} ms = {flop / t_own / 1e12:.1f} TFLOP/s float64 (symmetric half)", flush=True)
    torch.cuda.reset_peak_memory_stats()
    t_lib, ref = timed(lambda: (lambda xw: xw @ xw.t())(x.double() - mean))
    print(f"float64 copy + torch.matmul: {t_lib * 1e3:.1f} ms (peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB); "
          f"max |difference| {float((gram - ref).abs().max()):.2e} at entries up to {float(ref.abs().max()):.2e}", flush=True)
    del ref
    vec = torch.linalg.qr(torch.randn(n, k, generator=g, device=dev, dtype=torch.float64))[0]
    t_own, axes = timed(lambda: ops.pca_axes_f64(vec, k, x, mean))
    print(f"anyloc_pca_axes_f64 k = {k}: {t_own * 1e3:.1f} ms = {2 * k * n * f / t_own / 1e12:.1f} TFLOP/s float64", flush=True)
    t_lib, ref = timed(lambda: vec.t() @ (x.double() - mean))
    print(f"float64 copy + torch.matmul: {t_lib * 1e3:.1f} ms; max |difference| {float((axes - ref).abs().max()):.2e}", flush=True)
    del ref, axes, gram
    m = min(n, 2048)
    t0 = time.perf_counter()
    pca.PCA(min(k, m)).fit(x[:m])
    torch.cuda.synchronize()
    print(f"PCA({min(k, m)}).fit on {m} x {f} (Gram side, eigh of {m} x {m} included): {time.perf_counter() - t0:.2f} s", flush=True)


def fit(solver, n, f, k, args):
    x = vlad_like(n, f, args.decay)
    pca.PCA(8, solver=solver).fit(x[:256, :512].contiguous())          # untimed: library load, solver handles
    torch.cuda.synchronize()
    print(f"data {n} x {f}, decay {args.decay}; PCA({k}, solver={solver!r})", flush=True)
    stamps = {}
    real_gram, real_decompose = ops.pca_gram_f64, pca.PCA._decompose

    def gram(*a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = real_gram(*a)
        torch.cuda.synchronize()
        stamps["gram"] = time.perf_counter() - t0
        return out

    def decompose(self, sym, kk):
        stamps["sym"] = sym
        t0 = time.perf_counter()
        out = real_decompose(self, sym, kk)
        torch.cuda.synchronize()
        stamps["eigen"] = time.perf_counter() - t0
        return out

    ops.pca_gram_f64, pca.PCA._decompose = gram, decompose
    try:
        for run in range(args.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p = pca.PCA(k, solver=solver).fit(x)
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
            rest = total - stamps["gram"] - stamps["eigen"]
            print(f"run {run}: fit {total:.3f} s = Gram/scatter {stamps['gram'] * 1e3:.1f} ms + eigen step {stamps['eigen']:.3f} s + "
                  f"rest (mean, back-projection, signs) {rest * 1e3:.1f} ms; solver_used_ {p.solver_used_}, n_iter_ {p.n_iter_}", flush=True)
    finally:
        ops.pca_gram_f64, pca.PCA._decompose = real_gram, real_decompose
    if args.save:
        torch.save({"components": p.components_.cpu(), "singular_values": p.singular_values_.cpu()}, args.save)
    sym = stamps["sym"]
    m = sym.shape[0]
    if solver == "subspace":
        b = eigs.block_size(k)
        g = torch.Generator(device=dev).manual_seed(1)
        qt = torch.linalg.qr(torch.randn(m, b, generator=g, device=dev, dtype=torch.float64))[0].t().contiguous()
        small = torch.randn(b, b, generator=g, device=dev, dtype=torch.float64)
        t_apply, yt = timed(lambda: ops.gemm_nt_f64(qt, sym), reps=5)
        t_cross, _ = timed(lambda: ops.gemm_nt_f64(yt, yt, symmetric=True), reps=5)
        t_back, _ = timed(lambda: ops.gemm_nt_f64(small, yt.t()), reps=5)
        print(f"block b = {b}, m = {m}: apply Qt S {t_apply * 1e3:.2f} ms = {2 * m * m * b / t_apply / 1e12:.1f} TFLOP/s; "
              f"cross Yt Yt^T {t_cross * 1e3:.2f} ms = {m * b * b / t_cross / 1e12:.1f} TFLOP/s (symmetric half); "
              f"L^-1 Yt {t_back * 1e3:.2f} ms = {2 * m * b * b / t_back / 1e12:.1f} TFLOP/s; one iteration = apply + 2 x (cross + L^-1 Yt) "
              f"= {(t_apply + 2 * (t_cross + t_back)) * 1e3:.2f} ms of products", flush=True)
        if args.ratio:
            lam = torch.linalg.eigvalsh(sym).flip(0)
            print(f"lambda_(b+1) / lambda_k = {float(lam[b] / lam[k - 1]):.4f} (lambda_0 {float(lam[0]):.3e}, lambda_k {float(lam[k - 1]):.3e})", flush=True)
    if args.against:
        other = torch.load(args.against)
        dc = float((p.components_.cpu() - other["components"]).abs().max())
        ds = float(((p.singular_values_.cpu() - other["singular_values"]).abs() / other["singular_values"]).max())
        print(f"against {os.path.basename(args.against)}: components max |difference| {dc:.2e}, singular values max relative difference {ds:.2e}", flush=True)


def eigh_alone(m):
    g = torch.Generator(device=dev).manual_seed(0)
    a = torch.randn(m, m, generator=g, device=dev, dtype=torch.float64)
    a = a @ a.t()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch.linalg.eigh(a)
    torch.cuda.synchronize()
    print(f"torch.linalg.eigh of {m} x {m} float64: {time.perf_counter() - t0:.2f} s", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["products", "fit", "eigh"])
    ap.add_argument("rest", nargs="*")
    ap.add_argument("--decay", type=float, default=0.995)
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--ratio", action="store_true")
    ap.add_argument("--save")
    ap.add_argument("--against")
    args = ap.parse_args()
    if args.mode == "eigh":
        return eigh_alone(int(args.rest[0]))
    solver = args.rest.pop(0) if args.mode == "fit" else None
    n, f, k = (int(v) for v in (args.rest + ["10000", "49152", "512"][len(args.rest):]))
    if args.mode == "products":
        products(n, f, k)
    else:
        fit(solver, n, f, k, args)


if __name__ == "__main__":
    main()
