"""Round-4 GPU tests: a 4-rank run of ``bench.py --workload config3`` on one GPU, the patch embedding on the fp16 GEMM, and the
N > 1 collectives on real RCCL with one rank.  The round's index-identity and few-query top-k tests are in
tests/test_gpu_topk_panels.py and tests/test_gpu_topk_fewq.py, its call-pattern tests in tests/test_gpu_call_patterns.py."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def test_bench_config3_four_ranks_on_one_gpu():
    """``bench.py --workload config3 --gpus 4`` at a reduced shard (4 x 2 048 rows, 512 queries) with the ranks sharing the one
    GPU over gloo: the query all-gather with static counts, four per-shard searches with global indices, the single packed
    gather and the host merge -- the planted neighbour of every rank-0 query is found in ITS shard.  Four ranks, not the
    eight of configs[2]: with this test process they are five processes holding the one GPU, and the suite keeps that
    number at six or fewer."""
    env = dict(os.environ, ANYLOC_DIST_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "config3", "--gpus", "4", "--steps", "1",
                          "--warmup", "0", "--queries", "512", "--shard-rows", "2048"], env=env, capture_output=True, text=True,
                         timeout=1500)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 4 and out["unit"] == "queries/s" and out["value"] > 0
    assert out["planted_neighbours_found"] is True
    assert out["config"]["db_rows_total"] == 4 * 2048 and out["config"]["queries"] == 512


@pytest.mark.parametrize("name,batch,hw", [("dinov2_vits14", 1, (224, 322)), ("dinov2_vitg14", 3, (322, 322))])
def test_patch_embedding_on_the_fp16_gemm_agrees_with_the_fp32_gemm(name, batch, hw):
    """fp16 mode runs the patch embedding (conv 14x14 / 14 = a GEMM over 588-element patches, zero-padded to 592) on the
    two-term fp16 GEMM, the gathered patches and the weights quantised like every other operand (22 bits).  Against the fp32
    matrix-core GEMM (option h3_patch = 0) the layer-0 tokens -- the embedding after one block -- agree to 2e-6 of their
    scale, for unnormalised pixel values too (0 .. 255: the row scale is a power of two of the row's own maximum), and the
    result is the same run to run."""
    import utilities
    from anyloc_amd import ops, synth, weights
    weights.register_state_dict(name, synth.synthetic_state_dict(name, 7, device=DEV, depth=1))
    try:
        ext = utilities.DinoV2ExtractFeatures(name, 0, "token", device=DEV)
        ext.dino_model.ffn_check = False
        g = torch.Generator().manual_seed(5)
        for img in (torch.randn(batch, 3, *hw, generator=g), torch.rand(batch, 3, *hw, generator=g) * 255.0):
            img = img.to(DEV)
            with ops.options(h3_patch=0):
                want = ext(img).clone()
            got = ext(img).clone()
            assert torch.isfinite(got).all()
            assert float((got - want).abs().max()) <= 2e-6 * max(1.0, float(want.abs().max()))
            assert torch.equal(got, ext(img))
    finally:
        weights.unregister_state_dict(name)


@pytest.mark.parametrize("workload", ["config2", "config3"])
def test_sharded_step_on_real_rccl_with_one_rank(workload):
    """``ANYLOC_DIST_FORCE=1 python bench.py --gpus 1``: the process group is created with backend "nccl" (= RCCL) although
    there is one rank, and the step takes the SHARDED route -- all-gather of the query VLADs, per-shard top-k on the HIP
    kernels, gather of the [Q, k] lists to rank 0, host merge (retrieval.sharded_search) -- so every collective of the
    N > 1 path (device tensors, their dtypes, the barrier + MAX-over-ranks timing) executes on real RCCL, which a one-GPU
    box otherwise never does.  Recalls / planted neighbours as in the single-process run."""
    env = dict(os.environ, ANYLOC_DIST_FORCE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29533")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "ANYLOC_DIST_BACKEND"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"]
    if workload == "config2":
        cmd += ["--batch", "8", "--full", "--no-cpu-baseline", "--no-modes", "--no-stages"]
    else:
        cmd += ["--workload", "config3", "--queries", "300", "--shard-rows", "4096"]
    def run(e):
        res = subprocess.run(cmd, env=e, cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert res.returncode == 0, (res.stdout[-1500:], res.stderr[-3000:])
        lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, res.stdout[-2000:]
        return json.loads(lines[0])
    out = run(env)
    assert out["n_gpus"] == 1 and out["value"] > 0
    if workload == "config2":
        assert out["config"]["parallelism"] == "dp1+db-shard1"
        plain = run({k: v for k, v in env.items() if k != "ANYLOC_DIST_FORCE"})  # the single-process route: same recalls
        assert plain["config"]["parallelism"] == "single" and plain["recall"] == out["recall"]
    else:
        assert out["config"]["parallelism"] == "db-shard1" and out["planted_neighbours_found"] is True


_RCCL_ONE_RANK_JOB = r"""
import numpy as np, torch, torch.distributed as dist
from anyloc_amd import kmeans as hk, retrieval, synth
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
assert dist.get_backend() == "nccl"
dev = torch.device("cuda", 0)
g = torch.Generator().manual_seed(0)
db, qu = torch.randn(1501, 4096, generator=g).to(dev), torch.randn(13, 4096, generator=g).to(dev)
d, i = retrieval.sharded_search(db, 0, qu, 7)                       # all-gather of the queries, top-k, gather, host merge
d_ref, i_ref = retrieval.search(db, qu, 7)
assert np.array_equal(i, i_ref.cpu().numpy()) and np.allclose(d, d_ref.cpu().numpy(), atol=1e-6)
x = synth.clustered_tokens(1, 3000, 384, n_modes=6, seed=2, noise=0.5)[0].to(dev)
np.random.seed(11)
km = hk.KMeans(6, mode="cosine", process_group=dist.group.WORLD)    # sharded init (broadcast + all-reduce), all-reduce per iteration
km.fit(x)
np.random.seed(11)
flat = hk.KMeans(6, mode="cosine")
flat.fit(x)
assert km.n_iter_ == flat.n_iter_ and torch.equal(km.centroids, flat.centroids)
assert torch.equal(km.predict(x), flat.predict(x))
dist.barrier()
dist.destroy_process_group()
print("RCCL-ONE-RANK-OK")
"""


def test_sharded_search_and_sharded_kmeans_on_real_rccl_with_one_rank():
    """The library-level N > 1 entry points -- ``retrieval.sharded_search`` and ``KMeans(process_group=...)`` -- on a process
    group whose backend IS RCCL (one rank, cuda:0): broadcast, all-reduce, all-gather and gather of device tensors all run,
    and the results are those of the unsharded calls (bitwise for k-means: one shard = the flat fit)."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29537", PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, "-c", _RCCL_ONE_RANK_JOB], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "RCCL-ONE-RANK-OK" in res.stdout, (res.stdout[-1500:], res.stderr[-3000:])
