"""Round-3 additions (GPU box):

* ``bench.py --gpus 2`` started from a PLAIN subprocess (no torchrun in the command line) spawns its own ranks and
  prints one JSON line with ``n_gpus: 2`` -- through the ``ANYLOC_DIST_BACKEND=gloo`` override, both ranks on cuda:0;
* every tensor the sharded retrieval / sharded k-means hand to a collective lives on the comm device when the backend is
  not gloo (a "fake RCCL" group: gloo transport, ``get_backend`` answering "nccl", collectives asserting ``is_cuda``);
* scheduling variants of LayerNorm, the transposed SwiGLU epilogue and gemm_h3 on the 16x16x32 MFMA against the forms they
  replace.

The round's top-k tests are in tests/test_gpu_topk_panels.py and tests/test_gpu_topk_fewq.py, its checkpoint-file test in
tests/test_gpu_call_patterns.py.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from _ranks import free_port
from anyloc_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ bench --gpus 2
def test_bench_gpus2_plain_invocation_spawns_its_ranks():
    env = dict(os.environ, ANYLOC_DIST_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                          "--no-cpu-baseline", "--batch", "8", "--full"], env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 1 and out["unit"] == "images/s" and out["value"] > 0
    assert out["config"]["images_per_step"] == 16 and out["config"]["parallelism"] == "dp2+db-shard2"
    # merged global indices over both shards (rank r's places live at rows r * 10 000 ...): recalls are fractions, nested in k
    assert 0.0 <= out["recall"]["1"] <= out["recall"]["5"] <= out["recall"]["10"] <= 1.0


def _fake_rccl():
    """gloo transport, but the group answers "nccl" and every collective insists on device tensors (what RCCL does:
    "No backend type associated with device type cpu"), staging them through the host itself."""
    seen = []

    def staged(fn_name, tensor_args):
        real = getattr(dist, fn_name)

        def wrapper(*args, **kw):
            args = list(args)
            devs = []
            for i in tensor_args:
                if i < len(args) and torch.is_tensor(args[i]):
                    assert args[i].is_cuda, f"{fn_name}: argument {i} is on {args[i].device}, RCCL needs a device tensor"
                    devs.append((i, args[i]))
                elif i < len(args) and isinstance(args[i], (list, tuple)):
                    assert all(t.is_cuda for t in args[i]), f"{fn_name}: list argument {i} holds CPU tensors"
                    devs.append((i, list(args[i])))
            host = list(args)
            for i, t in devs:
                host[i] = [x.cpu() for x in t] if isinstance(t, list) else t.cpu()
            seen.append(fn_name)
            r = real(*host, **kw)
            for i, t in devs:                              # results back to the device tensors the caller passed
                if isinstance(t, list):
                    for dst, src in zip(t, host[i]):
                        dst.copy_(src)
                else:
                    t.copy_(host[i])
            return r
        return wrapper

    patched = {"all_reduce": staged("all_reduce", [0]), "broadcast": staged("broadcast", [0]),
               "all_gather_into_tensor": staged("all_gather_into_tensor", [0, 1]),
               "all_gather": staged("all_gather", [0, 1]), "get_backend": lambda group=None: "nccl"}
    real_gather = dist.gather

    def gather(tensor, gather_list=None, dst=0, group=None):
        assert tensor.is_cuda and (gather_list is None or all(t.is_cuda for t in gather_list)), "gather: CPU tensor under RCCL"
        seen.append("gather")
        host_list = [t.cpu() for t in gather_list] if gather_list is not None else None
        r = real_gather(tensor.cpu(), host_list, dst=dst, group=group)
        if gather_list is not None:
            for d_, s_ in zip(gather_list, host_list):
                d_.copy_(s_)
        return r
    patched["gather"] = gather
    return patched, seen


def _fake_rccl_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from anyloc_amd import kmeans as hk, retrieval
        patched, seen = _fake_rccl()
        saved = {k: getattr(dist, k) for k in patched}
        for k, v in patched.items():
            setattr(dist, k, v)
        try:
            dev = torch.device("cuda", 0)
            g = torch.Generator().manual_seed(0)
            dim = 4096
            db = torch.randn(1501, dim, generator=g)
            qu = torch.randn(13, dim, generator=g)
            bounds, q_bounds = [0, 700, 1501], [0, 5, 13]                       # uneven shards and query shares
            d, i = retrieval.sharded_search(db[bounds[rank]:bounds[rank + 1]].to(dev), bounds[rank],
                                            qu[q_bounds[rank]:q_bounds[rank + 1]].to(dev), 7)
            # even query shares: the single all_gather_into_tensor path
            d2, i2 = retrieval.sharded_search(db[bounds[rank]:bounds[rank + 1]].to(dev), bounds[rank],
                                              qu[6 * rank:6 * rank + 6].to(dev), 7)
            if rank == 0:
                d_ref, i_ref = retrieval.search(db.to(dev), qu.to(dev), 7)
                assert np.array_equal(i, i_ref.cpu().numpy()) and np.array_equal(i2, i_ref[:12].cpu().numpy())
            x = synth.clustered_tokens(1, 3000, 384, n_modes=6, seed=2, noise=0.5)[0]
            half = 1300
            x_loc = (x[:half] if rank == 0 else x[half:]).to(dev)
            np.random.seed(11)
            km = hk.KMeans(6, mode="cosine", process_group=dist.group.WORLD)
            km.fit(x_loc)                                                        # _sharded_init + per-iteration all-reduce
            np.random.seed(11)
            flat = hk.KMeans(6, mode="cosine")
            flat.fit(x.to(dev))
            assert km.n_iter_ == flat.n_iter_
            assert float((km.centroids.cpu() - flat.centroids.cpu()).abs().max()) < 1e-5
            assert {"all_gather_into_tensor", "broadcast", "all_reduce", "gather"} <= set(seen)
        finally:
            for k, v in saved.items():
                setattr(dist, k, v)
        torch.cuda.synchronize()
        if rank == 0:
            open(os.path.join(out_dir, "ok"), "w").write("1")
    finally:
        dist.destroy_process_group()


def test_collectives_get_device_tensors_under_a_non_gloo_backend(tmp_path):
    mp.spawn(_fake_rccl_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    assert (tmp_path / "ok").exists()


# ------------------------------------------------------------------- scheduling variants must not change a bit
def test_scheduling_variants_are_bitwise_equal():
    """layernorm_h2 with 1 / 2 / 4 rows per wave (option ln_rows_per_wave) reorders instructions, not arithmetic: the
    tokens are the same bits."""
    import utilities
    from anyloc_amd import ops, weights
    name = "dinov2_vitg14"
    weights.register_state_dict(name, synth.synthetic_state_dict(name, 3, device="cuda", depth=3))
    try:
        ext = utilities.DinoV2ExtractFeatures(name, 2, "token", use_cls=True, norm_descs=False, device="cuda")
        img = torch.randn(5, 3, 322, 322, generator=torch.Generator().manual_seed(4)).to("cuda")
        base = ext(img).clone()
        assert torch.isfinite(base).all()
        for opts in (dict(ln_rows_per_wave=1), dict(ln_rows_per_wave=2), dict(ln_rows_per_wave=4), dict(ln_waves=4), dict(ln_waves=8),
                     dict(ln_rows_per_wave=2, ln_waves=4)):
            with ops.options(**opts):
                assert torch.equal(ext(img), base), opts
    finally:
        weights.unregister_state_dict(name)


def test_swiglu_transposed_epilogue_agrees_with_the_lds_one():
    """Option h3_swiglu_t (read when the model is built): the w12 weights in the 16-channel block layout, the product
    formed transposed (weights as the MFMA's A operand), SiLU(gate) * value written as 16-byte image chunks straight from
    the accumulators -- against the 32 / 32 interleave whose epilogue goes through LDS: the same products and epilogue
    formula (the matrix cores sum a transposed block in another order: not the same bits), fused and unfused, at the
    bench tile configuration and at the small-tile ones.  The full-depth oracle parity suite runs with either layout."""
    import utilities
    from anyloc_amd import ops, weights
    name = "dinov2_vitg14"
    weights.register_state_dict(name, synth.synthetic_state_dict(name, 3, device="cuda", depth=3))
    try:
        img = torch.randn(5, 3, 322, 322, generator=torch.Generator().manual_seed(4)).to("cuda")
        out = {}
        for t in (0, 1):
            with ops.options(h3_swiglu_t=t):
                ext = utilities.DinoV2ExtractFeatures(name, 2, "token", use_cls=True, norm_descs=False, device="cuda")
            out[t, 1] = ext(img).clone()
            with ops.options(h3_fuse=0):
                out[t, 0] = ext(img).clone()
            one = ext(img[:1]).clone()                                   # the small-tile configurations (one image)
            assert torch.equal(one, ext(img[:1])) and float((one - out[t, 1][:1]).abs().max()) < 2e-6 * float(one.abs().max())
        assert torch.isfinite(out[0, 1]).all()
        scale = float(out[0, 1].abs().max())
        assert float((out[0, 1] - out[1, 1]).abs().max()) <= 2e-6 * scale
        assert float((out[0, 0] - out[1, 0]).abs().max()) <= 2e-6 * scale
        assert float((out[1, 1] - out[1, 0]).abs().max()) <= 2e-6 * scale
    finally:
        weights.unregister_state_dict(name)


def test_gemm_h3_on_the_16x16x32_mfma():
    """csrc/gemm_h3m.hip (option h3_mfma16; by default the retrieval panels' kernel): the two-term fp16 GEMM on
    v_mfma_f32_16x16x32_f16 with 256 x 256 tiles -- same operand images, same three products per k, against float64 at the
    bar of gemm_h3_kernel; ragged rows / columns, an odd number of 16-k blocks (the last ring stage half empty)."""
    from anyloc_amd import ops
    g = torch.Generator(device="cuda").manual_seed(1)
    M, N, K = 4500, 4200, 1552
    a = torch.randn(M, K, generator=g, device="cuda") * (0.5 + torch.rand(M, 1, generator=g, device="cuda"))
    w = torch.randn(N, K, generator=g, device="cuda") * 0.02
    bias = torch.randn(N, generator=g, device="cuda")
    a2, w2 = ops.split_h2(a), ops.split_h2(w)
    with ops.options(h3_mfma16=0):
        base = ops.gemm_nt_h3(a2, w2, M, N, K, bias)
    with ops.options(h3_mfma16=1):
        c = ops.gemm_nt_h3(a2, w2, M, N, K, bias)
    rows = torch.cat([torch.arange(0, 300, device="cuda"), torch.arange(M - 300, M, device="cuda")])
    ref = a[rows].double() @ w.double().t() + bias.double()
    mag = a[rows].double().abs() @ w.double().abs().t() + bias.double().abs()
    assert float(((c[rows].double() - ref).abs() / mag).max()) <= 6e-7
    assert float(((base[rows].double() - ref).abs() / mag).max()) <= 6e-7
