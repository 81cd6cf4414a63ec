"""Inputs of the k-means cases of tests/test_gpu_limits.py, shared with tests/test_limits_cpu.py: the CPU module checks,
without a GPU, that every case keeps what the GPU test relies on -- few rows on an fp32 near-tie of the oracle, and
clusters that stay empty."""
import torch

from anyloc_amd import synth
from oracle.fpk_kmeans import KMeans as RefKM

LABEL_TIE_CAP = 8          # labels a case may have excused as near-ties (the cap of tests/_vlad_parts_job.py)
KMEANS_N = 2500            # three chunks of >= 1024 rows, the last one ragged (452 rows)
# K: both sides of the full-width / half-width slice edge of accumulate_kernel (128 | 129: one | two passes of the label
# histogram too) and the last two K (256: the largest LDS request).  D = 260: a second slice with 4 live columns at the
# full width (256) and a third one at the half width (128), so a wrong slice width moves live columns.
KMEANS_CASES = [(K, D, KMEANS_N, mode) for K in (128, 129, 255, 256) for D in (64, 260) for mode in ("cosine", "euclidean")]
KMEANS_CASES += [(33, 384, KMEANS_N, mode) for mode in ("cosine", "euclidean")]      # the first K off the fused kernel at a ViT width


def kmeans_case(K, D, n):
    """-> (rows [n, D], centres [K, D]): rows around K // 8 directions with norms in [0.5, 1.5), centres drawn from the
    rows as tests/test_gpu_vlad_topk.py::test_kmeans_step_fused_path_vs_oracle draws them, the last two replaced by
    centres far from every row (50 in every coordinate: no row's nearest centre in either metric)."""
    x = synth.clustered_tokens(1, n, D, n_modes=max(K // 8, 2), seed=n + K, noise=0.5)[0]
    g = torch.Generator().manual_seed(K)
    x = x * (0.5 + torch.rand(n, 1, generator=g))
    c = x[torch.randperm(n, generator=g)[:K]].clone() + 0.01 * torch.randn(K, D, generator=g)
    c[K - 2:] = 50.0
    return x, c


def oracle_sim(x, c, mode):
    return RefKM.cos_sim(x, c) if mode == "cosine" else RefKM.euc_sim(x, c)
