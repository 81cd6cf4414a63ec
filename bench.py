"""Benchmark of the AnyLoc-VLAD-DINOv2 hot path on MI355X (driver contract).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

One *step* = one pass of the hot path over one batch of synthetic input, per rank:
    B query images (322x322, resident in HBM) -> DINOv2 ViT-G/14 layer-31 'value' tokens
    -> K=32 VLAD descriptors -> cosine top-20 against the resident 10 000-row database
    (N > 1: query VLADs all-gathered over RCCL, per-rank database shard of 10 000 rows,
     per-shard top-k gathered to rank 0 and merged on the host).
Workload = BASELINE.json configs[1].  ``value`` = images/second of the whole job.

A plain run does only what ``value`` needs: setup, W warm-up steps, the K timed steps, ``--dump-outputs`` and the JSON
line (``metric``, ``value``, ``unit``, ``higher_is_better``, ``dtype``, ``ms_per_step``, the configuration, ``setup_s``).
With ``--full`` the same timed steps are followed by everything else the benchmark measures and checks; the JSON line
then also carries ``recall``, ``rccl`` and
  * roofline of the dominant kernel: per-launch ALGORITHMIC FLOPs / average launch duration measured with HIP
    events on the launch stream in the timed region, against the peak of the arithmetic the block GEMMs run in
    (--gemm h3, default: fp16 MFMA peak / 3 products; x6: bf16 MFMA peak / 6; f32: fp32 MFMA peak) and, always,
    against the fp32-MFMA peak (`vs_fp32_mfma_peak`);
  * cpu_baseline (rank 0, N=1): the CPU oracle (reference algorithm restated, torch CPU)
    timed on this box's host cores on a bounded sample of the same workload, doubling as
    the parity check of the GPU run (``parity``);
  * (N=1) ``retrieval_check`` against a float64 flat search, ``modes`` (the other two GEMM arithmetics) and ``stages``
    (the other BASELINE.json configurations and the HBM-bound kernels), each with its own ``--no-*`` switch.
The dominant kernel's launches are bracketed by HIP events in the timed steps of both kinds of run, so that a plain
and a full run time the same steps.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from anyloc_amd import _lib, ops, retrieval, synth, weights  # noqa: E402
from anyloc_amd.extractor import DEFAULT_GEMM  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32
PEAK_BF16_MFMA_TFLOPS = 2500.0     # same guide: dense bf16 (v_mfma_f32_32x32x16_bf16)
X6_PRODUCTS = 6                    # bf16 MFMA products per fp32-accurate product (csrc/gemm_x6.hip)
HW, LAYER, FACET, K_CLUSTERS, TOPK = 322, 31, "value", 32, 20
MODEL = "dinov2_vitg14"
N_DB = 10000


def flops_per_image(dim=1536, depth_hook=31, n_patch=529, hidden=4096):
    """F_img(needed) = 2*N*588*D + L_hook*F_block + 2*T*D^2 (one facet)."""
    t = n_patch + 1
    f_block = 2 * t * dim * 3 * dim + 4 * t * t * dim + 2 * t * dim * dim + \
        2 * t * dim * 2 * hidden + 2 * t * hidden * dim
    return 2 * n_patch * 588 * dim + depth_hook * f_block + 2 * t * dim * dim


def roofline_of(prof, gemm, value_per_gpu, steps):
    """Live roofline of the dominant kernel of a timed region from the per-kernel HIP-event profile."""
    dom_name, dom = max(prof.items(), key=lambda kv: kv[1]["ms"])
    avg_ms = dom["ms"] / dom["calls"]
    achieved = dom["flops"] / dom["calls"] / (avg_ms * 1e-3) / 1e12
    # screened search (csrc/scores_screen.hip): the dominant kernel runs ONE fp16 product per k (peak 2500); unscreened: three (2500 / 3)
    dom_peak = PEAK_BF16_MFMA_TFLOPS if dom_name == "topk_screen_gemm" else PEAK_BF16_MFMA_TFLOPS / 3
    gemm_ms = sum(v["ms"] for k, v in prof.items() if k.endswith("_gemm"))
    gemm_fl = sum(v["flops"] for k, v in prof.items() if k.endswith("_gemm"))
    kern_ms = sum(v["ms"] for v in prof.values())
    products = {"x6": 6, "h3": 3}.get(gemm)      # matrix-core products per fp32-accurate product
    split = products is not None and dom_name.endswith("_gemm") and dom_name != "vit_patch_embed_gemm"
    # split modes: every algorithmic flop costs `products` bf16/fp16-MFMA flops, so the roofline of the fp32-accurate
    # contraction is the dense 16-bit peak / products; `achieved` stays ALGORITHMIC flops / time in every mode.
    peak = PEAK_BF16_MFMA_TFLOPS / products if split else PEAK_FP32_MFMA_TFLOPS
    all_gemm = gemm_fl / (gemm_ms * 1e-3) / 1e12
    e2e = value_per_gpu * flops_per_image() / 1e12
    traffic = pmc_traffic(dom_name, gemm)
    return {
        "bound": "mfma", "kernel": dom_name, "achieved": round(achieved, 2),
        "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(achieved / peak, 4),
        "peak_note": ((f"dense 16-bit MFMA peak 2500 / {products} matrix-core products per fp32-accurate product (" +
                       ("exact 3-way bf16 split" if products == 6 else "row-scaled 2-term fp16 split") + ")")
                      if split else "fp32 MFMA peak"),
        "vs_fp32_mfma_peak": round(achieved / PEAK_FP32_MFMA_TFLOPS, 4),
        "clock_note": ("profiles/r03_pmc_h3_sq_raw.md + r03_pmc_h3_write_raw.md (h3; re-measured in rounds 4 and 5: r04_pmc_sq.md, r05_pmc_summary.md) / "
                       "r01_pmc_x6.md (x6): under these GEMMs the chip runs at its power limit -- ~1.49 GHz under the profiler "
                       "with the matrix cores busy ~82 % of all SIMD cycles for the h3 w12 kernel (1.65 GHz / 83.6 % for x6); "
                       "`peak` is the nominal 2.4 GHz figure.  Calibration (profiles/r03_calib_h3_hipblaslt_warm.log): the same "
                       "h3 kernel runs 39 % faster on all-zero operands, and hipBLASLt's fp16 GEMM sustains 1.19-1.42 PFLOP/s "
                       "on these shapes on random data (this kernel: 1.14-1.28 PFLOP/s of fp16 MFMA work = 3 x achieved)") if split else None,
        # what the matrix cores SUSTAIN inside the chip's power limit on random operands, from registers, with no LDS or HBM
        # traffic at all (tools/micro/mfma_power.hip, profiles/r03_mfma_shape_power.log: 1 700-1 718 TFLOP/s for the 32x32x16
        # fp16 instruction this kernel uses; 2 424 on all-zero operands) -- `peak` above stays the guide's nominal figure
        "power_limited": ({"sustained_mfma_tflops": 1700.0, "peak": round(1700.0 / products, 1),
                           "frac": round(achieved / (1700.0 / products), 4),
                           "note": "register-resident fp16 MFMA loop on random operands, one MI355X; this kernel adds LDS, L2 and "
                                   "HBM traffic inside the same power budget"} if split and products == 3 else None),
        "avg_launch_ms": round(avg_ms, 4), "launches": dom["calls"],
        "traffic": traffic["bytes_per_launch"] if traffic else None, "traffic_detail": traffic,
        "all_gemms": {"achieved": round(all_gemm, 2), "frac": round(all_gemm / peak, 4),
                      "vs_fp32_mfma_peak": round(all_gemm / PEAK_FP32_MFMA_TFLOPS, 4),
                      "share_of_kernel_time": round(gemm_ms / kern_ms, 4)},
        "end_to_end": {"algorithmic_tflops_per_image": round(flops_per_image() / 1e12, 4),
                       "achieved": round(e2e, 2), "frac": round(e2e / peak, 4),
                       "vs_fp32_mfma_peak": round(e2e / PEAK_FP32_MFMA_TFLOPS, 4)},
        "kernels_ms_per_step": {k: round(v["ms"] / steps, 3) for k, v in
                                sorted(prof.items(), key=lambda kv: -kv[1]["ms"])},
        "kernels_note": "the dominant kernel's launches are bracketed by HIP events INSIDE the timed region; the other kernels' "
                        "times come from two fully bracketed steps run right after it, untimed (two events per launch cost a "
                        "step ~1 % when all ~225 launches carry them)",
    }


class PowerSampler:
    """Socket power and shader clock of the bench's GPU while it runs (make the power-cap argument
    evidence).  One background thread reads the amdgpu hwmon files -- ``power1_average`` / ``power1_input`` (microwatts),
    ``power1_cap``, ``freq1_input`` (sclk, Hz) -- every ``period`` seconds.  The box exposes the hwmon nodes of ALL its GPUs
    while the container sees one: the card is the one whose PCI address equals the HIP device's (torch device properties);
    where that cannot be read every card is sampled and the one that draws the most over the window is reported
    (``picked_by`` says which rule applied).  No hwmon: one ``rocm-smi --showpower --showmaxpower --json`` call per second.
    ``window(t0, t1)`` summarises the samples between two ``time.perf_counter()`` stamps.  Cost: a few small sysfs reads
    per sample on a host thread (no GPU work, no stream interaction)."""

    def __init__(self, device_index=0, period=0.02):
        import glob
        import threading
        self.period, self.samples, self._stop, self._active = period, [], threading.Event(), threading.Event()
        self.src, self.cards, self.picked_by = None, [], None
        nodes = sorted(glob.glob("/sys/class/drm/card[0-9]*/device/hwmon/hwmon*"))
        want = None
        try:
            pr = torch.cuda.get_device_properties(device_index)
            want = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}"
        except Exception:  # noqa: BLE001
            want = None
        for hw in nodes:
            files = {}
            for key, names in (("power", ("power1_average", "power1_input")), ("cap", ("power1_cap",)), ("sclk", ("freq1_input",))):
                for n in names:
                    if os.path.exists(os.path.join(hw, n)):
                        files[key] = os.path.join(hw, n)
                        break
            if "power" in files:
                pci = os.path.basename(os.path.realpath(os.path.join(hw, "..", ".."))).lower()
                cap = self._read(files.get("cap"))
                self.cards.append({"hwmon": hw, "pci": pci, "files": files, "cap_w": cap / 1e6 if cap else None})
        match = [c for c in self.cards if want and c["pci"].startswith(want)]
        if match:
            self.cards, self.picked_by = match[:1], "pci address " + want
        elif len(self.cards) > 1:
            self.picked_by = f"highest average power of the box's {len(self.cards)} cards (HIP device pci {want} not found in sysfs)"
        elif self.cards:
            self.picked_by = "the only card"
        if self.cards:
            self.src = "hwmon"
        else:
            import shutil
            if shutil.which("rocm-smi"):
                self.src, self.picked_by = "rocm-smi", "first card of rocm-smi"
                self.period = max(period, 1.0)
                self.cards = [{"hwmon": None, "pci": None, "files": {}, "cap_w": None}]
        self._thread = threading.Thread(target=self._run, daemon=True)
        if self.src:
            self._thread.start()

    @staticmethod
    def _read(path):
        if not path:
            return None
        try:
            with open(path) as fh:
                return float(fh.read().strip())
        except (OSError, ValueError):
            return None

    def _smi(self):
        import subprocess
        try:
            raw = subprocess.run(["rocm-smi", "--showpower", "--showmaxpower", "--json"], capture_output=True, text=True, timeout=5).stdout
            card = next(iter(json.loads(raw).values()))
            pw = next((float(v) for k, v in card.items() if "Power (W)" in k and "Max" not in k), None)
            cap = next((float(v) for k, v in card.items() if "Max" in k and "Power" in k), None)
            if cap:
                self.cards[0]["cap_w"] = cap
            return pw
        except Exception:  # noqa: BLE001
            return None

    def resume(self):
        """Sample from now on (the thread idles between ``pause()`` and ``resume()``: no sysfs reads, no SMU queries)."""
        self._active.set()

    def pause(self):
        self._active.clear()

    def _run(self):
        while not self._stop.is_set():
            if not self._active.wait(0.2):
                continue
            t = time.perf_counter()
            if self.src == "rocm-smi":
                row = [(self._smi(), None)]
            else:
                row = []
                for c in self.cards:
                    pw, clk = self._read(c["files"].get("power")), self._read(c["files"].get("sclk"))
                    row.append((pw / 1e6 if pw is not None else None, clk / 1e6 if clk is not None else None))
            self.samples.append((t, row))
            self._stop.wait(self.period)

    def stop(self):
        self._stop.set()

    def window(self, t0, t1):
        rows = [r for (t, r) in self.samples if t0 <= t <= t1]
        best = None
        for ci, c in enumerate(self.cards):
            pw = [r[ci][0] for r in rows if r[ci][0] is not None]
            ck = [r[ci][1] for r in rows if r[ci][1] is not None]
            if pw and (best is None or sum(pw) / len(pw) > best[0]):
                best = (sum(pw) / len(pw), pw, ck, c)
        if best is None:
            return {"source": self.src, "samples": 0, "avg_w": None, "cap_w": None, "sclk_mhz_avg": None, "picked_by": self.picked_by}
        avg, pw, ck, c = best
        return {"source": self.src, "card": c["hwmon"], "pci": c["pci"], "picked_by": self.picked_by, "samples": len(pw),
                "period_s": self.period, "avg_w": round(avg, 1), "max_w": round(max(pw), 1), "cap_w": c["cap_w"],
                "frac_of_cap": round(avg / c["cap_w"], 3) if c["cap_w"] else None,
                "sclk_mhz_avg": round(sum(ck) / len(ck), 0) if ck else None,
                "sclk_mhz_max": round(max(ck), 0) if ck else None,
                "sclk_note": "hwmon freq1_input; under rocm-smi this node reads the ~94 MHz sleep-state marker when the clock is "
                             "firmware-managed -- the PMC passes (profiles/r05_pmc_summary.md) give the in-kernel clock"}


def pmc_traffic(kernel, gemm):
    """HBM-side traffic of one launch of `kernel` from the committed rocprofv3 --pmc passes (FETCH_SIZE and WRITE_SIZE
    cannot be read in-process): profiles/pmc_traffic.json, written by tools/pmc_traffic.py from the counter CSVs of the
    same forward (B=61).  FETCH_SIZE is doubled as MI355X_MICROARCH.md prescribes for 16-byte-per-lane streaming reads."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        with open(path) as fh:
            tab = json.load(fh)
        return tab[gemm][kernel]
    except (OSError, KeyError, ValueError):
        return None


def synthetic_db(n, k, d, device, seed):
    """Database VLADs generated directly on the device: per-cluster unit blocks, globally
    normalised (SURVEY 8d config 3 recipe) -- extracting 10k images is setup, not the metric."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    db = torch.empty(n, k * d, dtype=torch.float32, device=device)
    for s in range(0, n, 1000):
        e = min(n, s + 1000)
        blk = torch.randn(e - s, k, d, generator=g, device=device)
        blk = torch.nn.functional.normalize(blk, dim=-1) / (k ** 0.5)
        db[s:e] = blk.reshape(e - s, k * d)
    return db


def respawn_under_torchrun(args):
    """``python bench.py --gpus N`` from a plain shell (no RANK / WORLD_SIZE in the environment): re-launch this very
    command line as N ranks, one per GPU, under ``torch.distributed.run`` on 127.0.0.1 and pass its exit code on.  Rank 0
    of the child job prints the JSON line; this parent prints nothing."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd, env=env))


def init_ranks(args):
    """One process per GPU (torch.distributed.run sets RANK / LOCAL_RANK / WORLD_SIZE); backend "nccl" = RCCL over xGMI.
    ``ANYLOC_DIST_BACKEND=gloo`` (tests on a one-GPU box) runs the same code with the collectives staged through the
    host; ranks then share the visible GPUs round-robin.  ``ANYLOC_DIST_FORCE=1`` creates the process group at N = 1 too:
    the sharded step (all-gather of the queries, per-shard top-k, gather + merge) then runs on REAL RCCL with one rank --
    what a one-GPU box can execute of the N > 1 path (tests/test_gpu_round4.py)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world == 1 and args.gpus > 1:
        respawn_under_torchrun(args)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    dist = None
    if world > 1 or os.environ.get("ANYLOC_DIST_FORCE") == "1":
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        backend = os.environ.get("ANYLOC_DIST_BACKEND", "nccl")
        n_vis = torch.cuda.device_count()
        if backend == "nccl" and n_vis < world:
            raise SystemExit(f"--gpus {world} needs {world} visible GPUs for RCCL (found {n_vis}); "
                             f"ANYLOC_DIST_BACKEND=gloo shares the visible ones")
        torch.cuda.set_device(local_rank % max(1, n_vis))
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    else:
        torch.cuda.set_device(0)
    return world, rank, torch.device("cuda", torch.cuda.current_device()), dist


def max_over_ranks(elapsed, dist, dev):
    """MAX of the ranks' wall times (on the group's comm device: the GPU for RCCL, the host for gloo)."""
    if dist is None:
        return elapsed
    t = torch.tensor([elapsed], dtype=torch.float64, device=retrieval.comm_device(None, dev))
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def rccl_record(dist, world, legs, ms_per_step, legs_per_rank=None, overlapped=None):
    """What the first real multi-GPU run needs in one shot: the process group's shape and, from ONE instrumented
    untimed step (device drained after every leg, retrieval.sharded_search(timings=...)), where a sharded step's time goes."""
    rec = {"world_size": world, "backend": None, "n_gpus_visible": torch.cuda.device_count(),
           "hsa_enable_ipc_mode_legacy": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")}
    if dist is None:
        rec["note"] = "single process, no process group (N = 1): the sharded step runs under `--gpus N` or ANYLOC_DIST_FORCE=1"
        return rec
    rec["backend"] = dist.get_backend()
    if legs:
        comm = legs.get("all_gather_ms", 0.0) + legs.get("gather_ms", 0.0)
        rec["legs_ms"] = {k: round(v, 3) for k, v in legs.items()}
        rec["comm_ms"] = round(comm, 3)
        rec["comm_frac_of_step"] = round(comm / ms_per_step, 4) if ms_per_step else None
        if legs_per_rank:
            rec["legs_ms_per_rank"] = [{k: round(v, 3) for k, v in (l or {}).items()} for l in legs_per_rank]
        if overlapped is not None:
            rec["timed_steps_overlap_all_gather_with_own_queries"] = bool(overlapped)
        rec["legs_note"] = ("rank 0's wall time per leg of one extra, instrumented sharded retrieval (all-gather of the query VLADs "
                            "over RCCL -> per-shard top-k -> one packed gather of the [Q,k] lists -> host k-way merge), each leg "
                            "drained before the next starts; the timed steps run without the drains")
    return rec


DUMP_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """``--dump-outputs DIR``: the arrays the timed path handed its caller in the LAST timed step, one ``DIR/<name>.npy``
    each -- float32, or float64 for integer and float64 arrays (indices stay exact).  The arrays share their leading axis
    (one row per query); past DUMP_BYTES in all, every array keeps the same fixed, seeded sample of those rows, whose row
    numbers go to ``DIR/sample_rows.npy``."""
    host = {}
    for name, v in arrays.items():
        a = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        host[name] = a.astype(np.float64 if a.dtype.kind in "biu" or a.dtype == np.float64 else np.float32)
    n = {a.shape[0] for a in host.values()}
    assert len(n) == 1, {k: a.shape for k, a in host.items()}
    n = n.pop()
    total = sum(a.nbytes for a in host.values())
    if total > DUMP_BYTES:
        keep = max(1, DUMP_BYTES // (total // n + 8))                # (+ 8 bytes a row: its number in sample_rows)
        rows = np.sort(np.random.default_rng(0).choice(n, size=keep, replace=False))
        host = {k: a[rows] for k, a in host.items()}
        host["sample_rows"] = rows.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in host.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
    return sorted(host)


def main_config3(args):
    """BASELINE.json configs[2]: 10 000 query VLADs against a 1 M-row database sharded 125 000 rows (24.6 GB) per GPU.
    One step = the whole retrieval: query descriptors all-gathered over RCCL, per-shard normalise + top-20 on the HIP
    kernels, [Q,20] lists gathered to rank 0 and merged on the host (retrieval.sharded_search).  At N < 8 the database
    is the first N shards (weak scaling: per-GPU work is fixed); ``value`` = queries/s of the whole job."""
    world, rank, dev, dist = init_ranks(args)
    _lib.load()
    NQ, NSHARD, KC, D = args.queries, args.shard_rows, K_CLUSTERS, 1536
    steps, warm = args.steps, args.warmup
    t_setup = time.time()
    db_rows = synthetic_db(NSHARD, KC, D, dev, seed=100 + rank)
    # the resident shard as a prepared flat index (faiss index.add, once): the score GEMM's operand images next to the fp32 rows;
    # with them the sharded step searches the rank's own queries while the others' are still in flight (retrieval.sharded_search)
    db = retrieval.FlatIndex(db_rows, "cosine", planes="auto")
    nq_local = NQ // world + (1 if rank < NQ % world else 0)
    q_counts = [NQ // world + (1 if r < NQ % world else 0) for r in range(world)]
    qu = synthetic_db(nq_local, KC, D, dev, seed=500 + rank)
    n_plant = min(64, nq_local)
    rows = torch.arange(n_plant, device=dev) * 17 + 5                     # query j of this rank depicts row 17 j + 5 of its own shard
    qu[:n_plant] = 0.9 * db_rows[rows] + 0.1 * qu[:n_plant]
    shard_base = rank * NSHARD
    torch.cuda.synchronize()
    t_setup = time.time() - t_setup
    results = []

    def step():
        if dist is None:
            d, i = retrieval.search(db, qu, TOPK)
            results.append((d, i))
        else:
            d, i = retrieval.sharded_search(db, shard_base, qu, TOPK, group=None, counts=q_counts)
            if rank == 0:
                results.append((d, i))

    for _ in range(warm):
        step()
    results.clear()
    ops.profile_enable(True)
    ops.profile_reset()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    ops.profile_enable(False)
    prof = ops.profile_dump()
    elapsed = max_over_ranks(elapsed, dist, dev)
    legs, legs_all = {}, None
    if dist is not None:                                                   # one instrumented step, every rank (collectives inside)
        retrieval.sharded_search(db, shard_base, qu, TOPK, group=None, counts=q_counts, timings=legs)
        legs_all = [None] * world
        dist.all_gather_object(legs_all, legs)                             # every rank's legs in rank 0's line
    if rank != 0:
        dist.destroy_process_group()
        return
    if args.dump_outputs:                                                  # the merged top-k lists of the last timed step
        dump_outputs(args.dump_outputs, {"topk_distances": results[-1][0], "topk_indices": results[-1][1]})
    idx = results[-1][1]
    idx = idx.cpu().numpy() if torch.is_tensor(idx) else np.asarray(idx)
    want = (np.arange(n_plant) * 17 + 5)                                  # rank 0's planted queries come first in the merged order
    planted_ok = bool((idx[:n_plant, 0] == want).all())
    dom_name, dom = max(prof.items(), key=lambda kv: kv[1]["ms"])
    avg_ms = dom["ms"] / dom["calls"]
    achieved = dom["flops"] / dom["calls"] / (avg_ms * 1e-3) / 1e12
    # screened search (csrc/scores_screen.hip): the dominant kernel runs ONE fp16 product per k (peak 2500); unscreened: three (2500 / 3)
    dom_peak = PEAK_BF16_MFMA_TFLOPS if dom_name == "topk_screen_gemm" else PEAK_BF16_MFMA_TFLOPS / 3
    out = {
        "metric": f"queries/sec ({NQ} query VLADs x database sharded {NSHARD} rows per GPU, top-20)",
        "value": round(steps * NQ / elapsed, 3), "unit": "queries/s", "n_gpus": world, "steps": steps, "warmup": warm,
        "ms_per_step": round(elapsed / steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": "BASELINE.json configs[2]: 10k query x 1M-row db (49152-d VLADs) sharded across the GPUs, "
                               "RCCL all-gather of the queries + per-shard top-k + host merge",
                   "queries": NQ, "db_rows_per_gpu": NSHARD, "db_rows_total": NSHARD * world, "vlad_dim": KC * D, "k": TOPK,
                   "resident_index": bool(db.has_planes),
                   "parallelism": f"db-shard{world}"},
        "planted_neighbours_found": planted_ok, "setup_s": round(t_setup, 1),
        "rccl": rccl_record(dist, world, legs, elapsed / steps * 1e3, legs_all,
                            overlapped=db.has_planes and world > 1 and len(set(q_counts)) == 1),
        "dtype_note": "screened search: every panel scored on the leading fp16 planes of the power-of-two-scaled two-term splits (one "
                      "fp16 MFMA product per k, fp32 accumulate) under a proven bound, the rows inside the bound re-scored from the fp32 "
                      "rows with float64 sums; option topk_screen = 0: three fp16 products per k for every row (rounds 3-5)",
        "roofline": {"bound": "mfma", "kernel": dom_name, "achieved": round(achieved, 2), "peak": round(dom_peak, 1),
                     "unit": "TFLOP/s", "frac": round(achieved / dom_peak, 4),
                     "job_algorithmic_tflops": round(2.0 * NQ * NSHARD * KC * D * steps / elapsed / 1e12, 1),
                     "vs_fp32_mfma_peak": round(achieved / PEAK_FP32_MFMA_TFLOPS, 4), "avg_launch_ms": round(avg_ms, 4),
                     "launches": dom["calls"], "traffic": None,
                     "kernels_ms_per_step": {k: round(v["ms"] / steps, 3) for k, v in
                                             sorted(prof.items(), key=lambda kv: -kv[1]["ms"])}},
    }
    print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()
    if not planted_ok:
        print("PARITY VIOLATION: planted neighbours not retrieved", file=sys.stderr, flush=True)
        sys.exit(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    # 61 images = 32 330 token rows = 252.6 row-tiles of 128: the 253 x {12,36,64} GEMM tile grids are
    # within 1.2 % of whole multiples of the 512 resident thread blocks (2 per CU) -- no tail wave
    ap.add_argument("--batch", type=int, default=61, help="query images per step per GPU")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check everything else (recall, roofline and per-kernel "
                         "table, power, RCCL legs, float64 retrieval check, CPU baseline + parity, other GEMM modes, stages; "
                         "the --no-* switches below drop parts of it); off: the headline line alone.  --workload config3 "
                         "prints its whole line either way")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--gemm", choices=["x6", "h3", "f32"], default=os.environ.get("ANYLOC_GEMM", DEFAULT_GEMM),
                    help="block GEMMs: x6 = exact 3-way bf16 split, six bf16 MFMA products, fp32 accumulate "
                         "(fp32-level accuracy); f32 = fp32 MFMA")
    ap.add_argument("--cpu-seconds", type=float, default=25.0)
    ap.add_argument("--no-modes", action="store_true", help="skip the short timings of the other two GEMM arithmetics")
    ap.add_argument("--mode-steps", type=int, default=0,
                    help="timed steps of each of the other GEMM arithmetics (0 = the same --steps as the headline mode)")
    ap.add_argument("--no-stages", action="store_true",
                    help="skip the `stages` block (k-means 5M x 1536, VLAD alone, one config-3 shard, ViT-L 518 two taps)")
    ap.add_argument("--power-steps", type=int, default=8,
                    help="extra untimed steps after the timed region over which socket power / shader clock are sampled (0 = off)")
    ap.add_argument("--power-period", type=float, default=0.05, help="seconds between power samples")
    ap.add_argument("--no-whole-jobs", action="store_true",
                    help="skip the two whole-job stages (configs[1] as one 11 000-image job, ~35 s; configs[2] whole on one GPU, "
                         "196.6 GB resident, ~15 s)")
    ap.add_argument("--workload", choices=["config2", "config3"], default="config2",
                    help="config2 (default): BASELINE.json configs[1], the bench line; config3: configs[2], retrieval of "
                         "10 000 queries against a database sharded 125 000 rows per GPU")
    ap.add_argument("--queries", type=int, default=10000, help="--workload config3: query VLADs of the whole job")
    ap.add_argument("--shard-rows", type=int, default=125000, help="--workload config3: database rows per GPU")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (top-k distances / indices, and the "
                         "query VLADs at N = 1) as DIR/<name>.npy, float32 / float64, at most 64 MB in all; the inputs are "
                         "seeded, so runs with the same arguments are comparable output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    os.environ["ANYLOC_GEMM"] = args.gemm
    if args.workload == "config3":
        return main_config3(args)

    world, rank, dev, dist = init_ranks(args)
    _lib.load()
    import utilities
    B, steps, warm = args.batch, args.steps, args.warmup
    total_steps = steps + warm

    # ---------------- setup (untimed): weights, vocabulary, database, query images ----------
    t_setup = time.time()
    sd = synth.synthetic_state_dict(MODEL, seed=0, device=str(dev))
    weights.register_state_dict(MODEL, sd)
    ext = utilities.DinoV2ExtractFeatures(MODEL, LAYER, FACET, device=str(dev))
    # distinct places: one block of B per step, at most ~1024 (longer runs cycle through the blocks)
    n_blocks = min(total_steps, max(1, 1024 // B))
    n_places = n_blocks * B
    db_img, qu_img, gt = synth.synthetic_places(n_places, n_places, HW, HW, seed=42 + rank, device=str(dev))
    vlad = utilities.VLAD(K_CLUSTERS, None, cache_dir=None)
    # vocabulary: k-means (HIP assign+update kernel) on the tokens of the first database images
    voc_tok = torch.cat([ext(db_img[s:s + B]) for s in range(0, min(n_places, 2 * B), B)])
    np.random.seed(42)
    vlad.fit(voc_tok.reshape(-1, voc_tok.shape[-1]))
    del voc_tok
    # database: 10k resident VLADs; the places the queries depict are real pipeline outputs
    db = synthetic_db(N_DB, K_CLUSTERS, 1536, dev, seed=100 + rank)
    for s in range(0, n_places, B):
        db[s:s + B] = vlad.generate_multi(ext(db_img[s:s + B]))
    del db_img
    shard_base = rank * N_DB
    torch.cuda.synchronize()
    t_setup = time.time() - t_setup

    # ---------------- one step of the hot path ---------------------------------------------
    results = []

    def step(i):
        blk = i % n_blocks
        imgs = qu_img[blk * B:(blk + 1) * B]
        tokens = ext(imgs)                                   # [B,529,1536] on device (ext: the current mode's extractor)
        q = vlad.generate_multi(tokens)                      # [B,49152]
        if dist is None:
            d, idx = retrieval.search(db, q, TOPK)           # normalise + top-k, device tensors
            results.append((d, idx, q))
        else:
            d, idx = retrieval.sharded_search(db, shard_base, q, TOPK, group=None, counts=[B] * world)
            if rank == 0:
                results.append((d, idx))

    for i in range(warm):
        step(i)
    # HIP events around EVERY launch cost the queue ~3 us each (450 per step): the timed region brackets only the launches
    # of the dominant kernel -- found by one fully bracketed, untimed step -- and the per-kernel table comes from two more
    # untimed steps after it (anyloc_profile_filter)
    ops.profile_enable(True)
    ops.profile_reset()
    step(0)
    torch.cuda.synchronize()
    ops.profile_enable(False)
    dom_tag = max(ops.profile_dump().items(), key=lambda kv: kv[1]["ms"])[0]
    results.clear()
    ops.profile_filter(dom_tag)
    ops.profile_enable(True)
    ops.profile_reset()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(warm, total_steps):
        step(i)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    t_end = time.perf_counter()
    elapsed = t_end - t0
    ops.profile_enable(False)
    prof_dom = ops.profile_dump()
    ops.profile_filter(None)
    elapsed = max_over_ranks(elapsed, dist, dev)
    images = steps * B * world
    value = images / elapsed
    headline = {
        "metric": "images/sec (DINOv2->VLAD->top-k), ViT-G/14 L31 value K=32", "value": round(value, 3),
        "unit": "images/s", "n_gpus": world, "steps": steps, "warmup": warm,
        "ms_per_step": round(elapsed / steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None,
        "dtype": {"x6": "f32 (GEMM operands as exact 3-way bf16 splits, 6 bf16 MFMA products, fp32 accumulate)",
                  "h3": "f32 (GEMM and attention operands as power-of-two-scaled 2-term fp16 splits = 22 bits, "
                        "3 fp16 MFMA products, fp32 accumulate; softmax, LayerNorm, residuals in fp32)",
                  "f32": "f32"}[args.gemm], "data": "synthetic",
        "config": {"workload": "BASELINE.json configs[1]: DINOv2 ViT-G/14 layer31 'value' K=32 VLAD, "
                               "322x322, top-20 vs 10k-row database per GPU", "batch_per_gpu": B, "gemm": args.gemm,
                   "images_per_step": B * world, "db_rows_per_gpu": N_DB, "vlad_dim": K_CLUSTERS * 1536,
                   "weights": "random-init, hub layout (no checkpoint available offline)",
                   "parallelism": f"dp{world}+db-shard{world}" if dist is not None else "single"},
        "setup_s": round(t_setup, 1),
    }
    if args.dump_outputs and rank == 0:      # the last timed step: its query VLADs (N = 1) and the (merged) top-k lists
        dump_outputs(args.dump_outputs, dict(zip(("topk_distances", "topk_indices", "query_vlads"), results[-1])))
    if not args.full:                        # a plain run ends here: the headline line, nothing else measured or checked
        if rank == 0:
            print(json.dumps(headline), flush=True)
        if dist is not None:
            dist.destroy_process_group()
        return
    rccl_legs, rccl_legs_all = {}, None
    if dist is not None:                     # one instrumented retrieval of a step's queries, every rank (collectives inside)
        q_probe = vlad.generate_multi(ext(qu_img[:B]))
        retrieval.sharded_search(db, shard_base, q_probe, TOPK, group=None, counts=[B] * world, timings=rccl_legs)
        del q_probe
        rccl_legs_all = [None] * world
        dist.all_gather_object(rccl_legs_all, rccl_legs)
    timed_results = list(results)            # (the untimed steps below and the `modes` block re-use and clear `results`)
    # Socket power / shader clock: sampled over EXTRA, untimed steps identical to the timed ones, right after them -- the
    # sampler reads the GPU's own hwmon nodes (an SMU query each), so it never runs while `value` is being measured
    sampler, power_timed = None, None
    if args.power_steps > 0:                 # (every rank runs the steps -- a sharded step holds collectives; rank 0 samples)
        if rank == 0:
            sampler = PowerSampler(dev.index or 0, period=args.power_period)
        torch.cuda.synchronize()
        if sampler is not None:
            sampler.resume()
        t_p0 = time.perf_counter()
        for i in range(args.power_steps):
            step(warm + i)
        torch.cuda.synchronize()
        t_p1 = time.perf_counter()
    if sampler is not None:
        sampler.pause()
        power_timed = sampler.window(t_p0, t_p1)
        power_timed["steps"] = args.power_steps
        power_timed["ms_per_step_while_sampling"] = round((t_p1 - t_p0) / args.power_steps * 1e3, 3)
        power_timed["note"] = ("sampled over extra untimed steps right after the timed region (same workload); "
                               "`ms_per_step_while_sampling` against `ms_per_step` shows what the sampling itself costs")
        results.clear()
    ops.profile_enable(True)
    ops.profile_reset()
    for i in range(2):
        step(warm + i)
    torch.cuda.synchronize()
    ops.profile_enable(False)
    prof = {k: {f: v[f] * (steps / 2.0) for f in ("calls", "ms", "flops", "bytes")} for k, v in ops.profile_dump().items()}
    prof[dom_tag] = prof_dom[dom_tag]        # the dominant kernel: its launches inside the timed region
    results.clear()

    if rank != 0:
        dist.destroy_process_group()
        return

    # Recall@1 of the timed queries (rank 0's share): query i depicts place i of its own rank
    if dist is None:
        idx_all = torch.cat([r[1] for r in timed_results]).cpu().numpy()
        gt_timed = np.empty(len(idx_all), dtype=object)
        for n, i in enumerate(range(warm, total_steps)):
            for j in range(B):
                gt_timed[n * B + j] = np.array([(i % n_blocks) * B + j])
        rec = retrieval.recalls_from_indices([1, 5, 10], idx_all, gt_timed)
    else:
        # merged lists are ordered rank-major within a step; rank r's query j of step i depicts global
        # database row r*N_DB + i*B + j (its own shard's place)
        idx_all = np.concatenate([r[1] for r in timed_results])
        gt_timed = np.empty(len(idx_all), dtype=object)
        n = 0
        for i in range(warm, total_steps):
            for r in range(world):
                for j in range(B):
                    gt_timed[n] = np.array([r * N_DB + (i % n_blocks) * B + j])
                    n += 1
        rec = retrieval.recalls_from_indices([1, 5, 10], idx_all, gt_timed)

    roofline = roofline_of(prof, args.gemm, value / world, steps)
    # socket power / shader clock over the timed region (hwmon samples of a host thread): the evidence behind `power_limited`
    roofline["power"] = power_timed

    out = dict(headline, recall=rec, roofline=roofline,
               rccl=rccl_record(dist, world, rccl_legs, elapsed / steps * 1e3, rccl_legs_all))

    # ---------------- CPU baseline + parity on a bounded sample (N=1 only) -----------------
    # ---------------- the other two GEMM arithmetics, timed briefly in the same run (N=1) -------
    if world == 1 and not args.no_modes:
        mode_steps = args.mode_steps or steps
        modes = {args.gemm: {"value": round(value, 3), "ms_per_step": round(elapsed / steps * 1e3, 3), "steps": steps,
                             "frac": roofline["frac"], "peak": roofline["peak"], "achieved": roofline["achieved"],
                             "end_to_end_frac": roofline["end_to_end"]["frac"]}}
        for mode in ("h3", "x6", "f32"):
            if mode == args.gemm:
                continue
            os.environ["ANYLOC_GEMM"] = mode
            ext_m = utilities.DinoV2ExtractFeatures(MODEL, LAYER, FACET, device=str(dev))
            ext_prev, ext = ext, ext_m
            try:
                step(0)
                results.clear()
                ops.profile_filter(dom_tag)
                ops.profile_enable(True)
                ops.profile_reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(mode_steps):
                    step(warm + i)
                torch.cuda.synchronize()
                el = time.perf_counter() - t0
                ops.profile_enable(False)
                pd = ops.profile_dump()
                ops.profile_filter(None)
                ops.profile_enable(True)
                ops.profile_reset()
                step(warm)
                torch.cuda.synchronize()
                ops.profile_enable(False)
                pm = {k: {f: v[f] * float(mode_steps) for f in ("calls", "ms", "flops", "bytes")} for k, v in ops.profile_dump().items()}
                if dom_tag in pd:
                    pm[dom_tag] = pd[dom_tag]
                r = roofline_of(pm, mode, mode_steps * B / el, mode_steps)
                modes[mode] = {"value": round(mode_steps * B / el, 3), "ms_per_step": round(el / mode_steps * 1e3, 3),
                               "steps": mode_steps, "frac": r["frac"], "peak": r["peak"], "achieved": r["achieved"],
                               "end_to_end_frac": r["end_to_end"]["frac"], "kernel": r["kernel"]}
            finally:
                ext = ext_prev
                del ext_m
                results.clear()
        os.environ["ANYLOC_GEMM"] = args.gemm
        out["modes"] = modes

    failed = None
    if dist is None:
        # identity of the retrieval of EVERY timed query with an exact (float64) flat search over the whole database
        rchk = retrieval_identity(timed_results, db, gt_timed)
        out["retrieval_check"] = rchk
        if not rchk["ok"]:
            failed = f"timed queries: retrieval differs from the float64 flat search ({rchk})"
        timed_results.clear()
    if world == 1 and not args.no_cpu_baseline:
        out.update(cpu_baseline_and_parity(sd, qu_img, vlad, db, ext, args.cpu_seconds, warm, B))
        failed = failed or parity_violation(out["parity"])
        out["parity"]["ok"] = parity_violation(out["parity"]) is None
        out["recall_note"] = ("`recall` is against the synthetic ground truth (which place a query image depicts); identity "
                              "with the reference's retrieval is `parity.top1_equal` / `parity.topk_index_mismatches` on the "
                              f"{out['parity']['images']} images the CPU oracle could process inside --cpu-seconds")
    if world == 1 and not args.no_stages:
        # the other BASELINE.json configurations and the HBM-bound kernels, timed by the same process (driver clock)
        check = not args.no_cpu_baseline
        b1 = stage_b1(ext, qu_img, sampler)
        # the scripts' DEFAULT image shape (configs.py:141 resize = [480, 640] -> 476 x 630 after the centre crop): T = 1531
        img_480 = synth.synthetic_places(1, 8, 476, 630, seed=77, device=str(dev))[1]
        b1_480 = stage_b1(ext, img_480, sampler, label="476x630 (the scripts' default resize [480, 640], centre-cropped)")
        del img_480
        sp = stage_script_path(ext, vlad, db, qu_img, gt)
        # the pipeline's own tokens of 256 query images for the VLAD stages (832 MB; freed by run_stages)
        n_real = min(256, qu_img.shape[0])
        real_tokens = torch.cat([ext(qu_img[s0:s0 + 64]) for s0 in range(0, n_real, 64)]) if n_real >= 61 else None
        del qu_img
        full_job = None
        if not args.no_whole_jobs:
            del ext                                              # (the job builds its own extractor from the registered weights)
            ext = None
            _lib.release_workspaces()
            torch.cuda.empty_cache()
            full_job = stage_config2_full_job(dev)
        weights.unregister_state_dict(MODEL)
        out["stages"] = run_stages(dev, vlad, check, real_tokens)
        del real_tokens
        out["stages"]["vitg_b1"] = b1
        out["stages"]["vitg_b1_480x640"] = b1_480
        out["stages"]["script_path_vitg"] = sp
        if full_job is not None:
            out["stages"]["config2_full_job"] = full_job
            del db, sd
            _lib.release_workspaces()
            torch.cuda.empty_cache()
            out["stages"]["config3_whole_db"] = stage_config3_whole_db(dev)
        bad = [k for k, v in out["stages"].items() if v.get("oracle_ok") is False]
        if bad and failed is None:
            failed = f"stage oracle spot-check failed: {bad}"
    # a compact record of the checks and of the exact-arithmetic mode INSIDE `roofline` (the driver's parsed copy keeps the
    # contract keys; `parity`, `modes`, `stages` are extra keys it may drop)
    summ = {}
    if "parity" in out:
        pr = out["parity"]
        summ["oracle"] = {"images": pr["images"], "token_max_abs_err": float(f"{pr['token_max_abs_err']:.3g}"),
                          "vlad_max_rel_err": None if pr["vlad_max_rel_err"] is None else float(f"{pr['vlad_max_rel_err']:.3g}"),
                          "label_mismatches": pr["label_mismatches"], "top1_equal": pr["top1_equal"],
                          "topk_index_mismatches": pr["topk_index_mismatches"], "ok": pr["ok"]}
    if "retrieval_check" in out:
        rc = out["retrieval_check"]
        summ["retrieval_vs_float64"] = {k: rc[k] for k in ("queries", "db_rows", "index_mismatches", "near_tie_swaps",
                                                            "recall_identical", "ok")}
    if "modes" in out and "f32" in out["modes"]:
        m = out["modes"]["f32"]
        summ["f32_mode"] = {"value": m["value"], "frac": m["frac"], "end_to_end_frac": m["end_to_end_frac"]}
    if "stages" in out:
        st = out["stages"]
        summ["stages"] = {k: (v.get("images_per_s") or v.get("ms") or v.get("ms_per_image") or v.get("seconds_per_retrieval") or v.get("skipped") or
                              v.get("ms_per_iteration") or v.get("kernel_ms"))
                          for k, v in st.items()}
    out["roofline"]["checks"] = summ
    out["roofline"].update(flat_evidence(out))
    print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()
    if failed:
        print(f"PARITY VIOLATION: {failed}", file=sys.stderr, flush=True)
        sys.exit(3)


def flat_evidence(out):
    """SCALAR copies of the run's evidence for `roofline` (round 6): a parsed copy of the line that keeps only the scalar
    members of the contract objects still carries the end-to-end fraction, the power record, the exact-fp32 mode, the parity
    summary and one figure per stage.  Every key is a plain number / bool (None when the run skipped that part)."""
    r = out["roofline"]
    flat = {}

    def put(key, v, nd=4):
        if isinstance(v, bool) or v is None:
            flat[key] = v
        elif isinstance(v, (int, float)):
            flat[key] = round(float(v), nd) if isinstance(v, float) else v
    put("e2e_frac", (r.get("end_to_end") or {}).get("frac"))
    pw = r.get("power") or {}
    put("power_w", pw.get("avg_w"), 1)
    put("power_cap_w", pw.get("cap_w"), 1)
    put("sclk_mhz", pw.get("sclk_mhz_avg"), 0)
    f32 = (out.get("modes") or {}).get("f32") or {}
    put("f32_mode_images_per_s", f32.get("value"), 2)
    put("f32_mode_frac", f32.get("frac"))
    put("f32_mode_e2e_frac", f32.get("end_to_end_frac"))
    x6 = (out.get("modes") or {}).get("x6") or {}
    put("x6_mode_images_per_s", x6.get("value"), 2)
    pr = out.get("parity") or {}
    put("parity_ok", pr.get("ok"))
    put("parity_images", pr.get("images"))
    put("parity_token_max_abs_err", pr.get("token_max_abs_err"), 10)
    put("parity_vlad_rel_err", pr.get("vlad_max_rel_err"), 10)
    put("label_mismatches", pr.get("label_mismatches"))
    put("topk_index_mismatches", pr.get("topk_index_mismatches"))
    rc = out.get("retrieval_check") or {}
    put("retrieval_ok", rc.get("ok"))
    put("retrieval_queries", rc.get("queries"))
    put("retrieval_index_mismatches", rc.get("index_mismatches"))
    st = out.get("stages") or {}
    put("b1_ms", (st.get("vitg_b1") or {}).get("ms_per_image"), 3)
    put("b1_480x640_ms", (st.get("vitg_b1_480x640") or {}).get("ms_per_image"), 3)
    put("script_path_images_per_s", (st.get("script_path_vitg") or {}).get("images_per_s"), 1)
    legs = (st.get("script_path_vitg") or {}).get("legs_ms") or {}
    put("script_generate_multi_ms", legs.get("generate_multi_total"), 2)
    put("script_get_top_k_recall_ms", legs.get("get_top_k_recall_total"), 2)
    put("vlad61_frac", (st.get("vlad_61img_pipeline_tokens") or {}).get("frac"))
    put("vlad256_frac", (st.get("vlad_256img_pipeline_tokens") or {}).get("frac"))
    put("kmeans_frac", (st.get("kmeans_5Mx1536") or {}).get("frac"))
    put("config3_shard_frac", (st.get("config3_shard") or {}).get("frac"))
    put("config3_shard_ms", (st.get("config3_shard") or {}).get("ms"), 2)
    put("config3_shard_peak_tflops", (st.get("config3_shard") or {}).get("peak"), 1)
    put("config3_shard_ms_unscreened", (st.get("config3_shard") or {}).get("ms_unscreened"), 2)
    put("config3_shard_speedup_vs_unscreened", (st.get("config3_shard") or {}).get("speedup_vs_unscreened"), 3)
    put("config3_shard_queries_per_s", (st.get("config3_shard") or {}).get("queries_per_s"), 1)
    put("config3_whole_db_s", (st.get("config3_whole_db") or {}).get("seconds_per_retrieval"), 3)
    put("vitl_518_images_per_s", (st.get("vitl_518_2taps") or {}).get("images_per_s"), 1)
    put("config2_full_job_s", (st.get("config2_full_job") or {}).get("seconds"), 2)
    bad = [k for k, v in st.items() if isinstance(v, dict) and v.get("oracle_ok") is False]
    if st:
        flat["stages_oracle_ok"] = not bad
    km = r.get("kernels_ms_per_step") or {}
    put("attention_ms_per_step", km.get("attention"), 3)
    put("layernorm_ms_per_step", km.get("layernorm_h2"), 3)
    return flat


def retrieval_identity(results, db, gt_timed, tol=3e-6):
    """Top-k indices, distances and Recall@1/5/10 of ALL timed queries against an exact float64 flat search over the whole
    resident database (device float64 matmul of the L2-normalised operands: the checker, not the product).  Tie-aware: a
    differing index is accepted only where the float64 scores of the two candidates lie within ``tol`` of each other (the
    fp32 rounding of a score near 1); anything else is a mismatch and fails the run.  Reference: utilities.py:433-468."""
    idx = torch.cat([r[1] for r in results])
    dist = torch.cat([r[0] for r in results])
    q = torch.cat([r[2] for r in results])
    k = idx.shape[1]
    dbn = torch.nn.functional.normalize(db.double(), dim=1)
    mism = swaps = 0
    max_derr = 0.0
    ref_idx = []
    for s0 in range(0, q.shape[0], 256):
        qn = torch.nn.functional.normalize(q[s0:s0 + 256].double(), dim=1)
        sc = qn @ dbn.T                                             # [256, N] float64
        # exact ranking with faiss' tie rule (lower index first): stable sort of -score
        order = torch.sort(-sc, dim=1, stable=True)[1][:, :k]
        ref_idx.append(order)
        ours = idx[s0:s0 + 256]
        got = torch.gather(sc, 1, ours.clamp_min(0))
        want = torch.gather(sc, 1, order)
        diff = ours != order
        near = (got - want).abs() <= tol
        swaps += int((diff & near).sum())
        mism += int((diff & ~near).sum())
        max_derr = max(max_derr, float((dist[s0:s0 + 256].double() - got).abs().max()))
    ref_idx = torch.cat(ref_idx).cpu().numpy()
    rec_ref = retrieval.recalls_from_indices([1, 5, 10], ref_idx, gt_timed)
    rec_ours = retrieval.recalls_from_indices([1, 5, 10], idx.cpu().numpy(), gt_timed)
    ok = mism == 0 and rec_ref == rec_ours and max_derr <= tol
    return {"queries": int(q.shape[0]), "db_rows": int(db.shape[0]), "k": int(k), "index_mismatches": mism,
            "near_tie_swaps": swaps, "tie_tolerance": tol, "max_distance_err": max_derr, "recall": rec_ours,
            "recall_float64": rec_ref, "recall_identical": rec_ref == rec_ours, "ok": bool(ok),
            "checker": "device float64 matmul of the normalised operands + stable sort (ties -> lower index)"}


def parity_violation(p):
    """north_star bar on the bench's own oracle sample: tokens <= 2e-5, VLAD <= 1e-5, cluster ids identical except at
    oracle ties (< 1e-6 top-2 gap), top-1 identical, top-k indices identical for images without a tie flip."""
    if p["token_max_abs_err"] > 2e-5:
        return f"token error {p['token_max_abs_err']:.3e} > 2e-5"
    if p["vlad_max_rel_err"] is not None and p["vlad_max_rel_err"] > 1e-5:
        return f"VLAD relative error {p['vlad_max_rel_err']:.3e} > 1e-5"
    if p["label_mismatches"] and p["largest_oracle_gap_of_a_mismatch"] >= 1e-6:
        return f"cluster-id mismatch at an oracle gap of {p['largest_oracle_gap_of_a_mismatch']:.3e}"
    if not p["top1_equal"]:
        return "top-1 differs from the oracle"
    if p["topk_index_mismatches_in_clean_images"]:
        return f"{p['topk_index_mismatches_in_clean_images']} top-k indices differ in images without a tie flip"
    return None


def cpu_baseline_and_parity(sd, qu_img, vlad, db, ext, budget_s, warm, B):
    """Oracle (reference algorithm, torch CPU, all host threads) on the first timed query
    images: full 40-block forward at B=1 as the reference runs it (utilities.py:269), reference
    VLAD restatement, flat top-k against a 2000-row slice of the same database."""
    from oracle import dinov2_ref, faiss_flat, vlad_ref
    cores = os.cpu_count() or 1
    model = dinov2_ref.build(MODEL, {k: v.cpu() for k, v in sd.items()})
    # torch's CPU GEMMs at M=530 do not scale to every hardware thread: pick the fastest thread count
    # on ONE transformer block first (a few seconds), then time whole images with it
    probe = torch.randn(1, 530, 1536)
    best_t, threads = None, cores
    for nt in sorted({min(cores, n) for n in (16, 32, 64)}):
        torch.set_num_threads(nt)
        with torch.no_grad():
            model.blocks[0](probe)                    # warm-up (thread pool, allocator)
            dt = None
            for _ in range(3):                        # best of three: the host is shared, single runs are noisy
                t0 = time.perf_counter()
                model.blocks[0](probe)
                el = time.perf_counter() - t0
                dt = el if dt is None else min(dt, el)
        if best_t is None or dt < 0.95 * best_t:      # prefer fewer threads unless clearly faster
            best_t, threads = dt, nt
    torch.set_num_threads(threads)
    cores = threads
    centers = vlad.c_centers.cpu()
    db_slice = db[:2000].cpu()
    imgs = qu_img[:B].cpu()
    t_used, n_done = 0.0, 0
    toks, vl = [], []
    t_all0 = time.perf_counter()
    while n_done < len(imgs) and (n_done < 1 or t_used < budget_s):
        t0 = time.perf_counter()
        tk = dinov2_ref.extract_facet(model, imgs[n_done:n_done + 1], LAYER, FACET)[0]
        v, lab = vlad_ref.vlad_hard(tk, centers)
        toks.append(tk)
        vl.append(v)
        n_done += 1
        t_used += time.perf_counter() - t0
    vl = torch.stack(vl)
    t0 = time.perf_counter()
    d_ref, i_ref = faiss_flat.flat_search(torch.nn.functional.normalize(vl),
                                          torch.nn.functional.normalize(db_slice), TOPK)
    t_search = time.perf_counter() - t0
    # scale the search slice to the full 10k rows for the per-image rate
    per_img = t_used / n_done + (t_search / n_done) * (N_DB / 2000.0)
    # parity of the GPU path on the same images
    g_tok = ext(imgs[:n_done].to(db.device))
    # labels come from the SAME call that produces the descriptors (the product's VLAD path)
    g_vl, lab_g = ops.vlad(g_tok, vlad.c_centers.to(db.device), return_labels=True)
    g_d, g_i = retrieval.search(db[:2000], g_vl, TOPK)
    ref_tok = torch.stack(toks)
    tok_err = float((g_tok.cpu() - ref_tok).abs().max())
    lab_g = lab_g.cpu().reshape(n_done, -1)
    lab_r = vlad_ref.hard_labels(ref_tok.reshape(-1, g_tok.shape[-1]), centers).reshape(n_done, -1)
    flips = lab_g != lab_r
    # a flipped id is an fp32 tie: report the oracle's own top-2 cosine gap of those tokens
    gap = 0.0
    if flips.any():
        sc = vlad_ref.fpk_cosine_scores(ref_tok[flips], centers).topk(2, dim=1)[0]
        gap = float((sc[:, 0] - sc[:, 1]).max())
    clean = ~flips.any(dim=1)
    rel = (g_vl.cpu() - vl).norm(dim=1) / vl.norm(dim=1)
    return {
        "cpu_baseline": {"value": round(1.0 / per_img, 4), "unit": "images/s", "cores": cores, "kind": "port", "host_cpus": os.cpu_count(),
                         "sample": f"{n_done} query images end-to-end at B=1 (full 40-block ViT-G forward as the "
                                   f"reference runs it + VLAD) + top-{TOPK} of {n_done}x2000 slice scaled to 10k rows; "
                                   f"{t_used + t_search:.1f} s of CPU work"},
        "parity": {"images": n_done, "token_max_abs_err": tok_err,
                   "vlad_max_rel_err": float(rel[clean].max()) if clean.any() else None,
                   "label_mismatches": int(flips.sum()), "labels": int(lab_r.numel()),
                   "largest_oracle_gap_of_a_mismatch": gap, "images_with_a_mismatch": int((~clean).sum()),
                   "top1_equal": bool(torch.equal(g_i[:, 0].cpu(), i_ref[:, 0])),
                   "topk_index_mismatches": int((g_i.cpu() != i_ref).sum()),
                   # the same count restricted to images whose cluster ids all agree (a flipped fp32 tie moves one
                   # token's residual between two VLAD blocks, which can reorder that image's deep ranks)
                   "topk_index_mismatches_in_clean_images": int((g_i.cpu() != i_ref)[clean].sum())},
    }


# ---------------------------------------------------------------- stages ---------------------------------------------
KERNEL_MS_NOTE = ("kernel_ms / achieved / frac: the stage kernel's own HIP-event duration, the shorter of two profiled calls "
                  "(launch gaps and the other launches of the call excluded); achieved_wall: the same bytes over the wall time "
                  "of a whole call, averaged over the timed iterations")
PEAK_HBM_TBPS = 8.0                # MI355X_MICROARCH.md: HBM3E spec peak (6.3 TB/s achievable by a float4 copy)


def _timed(fn, iters, warm=1):
    """Wall time per call of ``fn`` (device drained on both sides, per-kernel profiler OFF: its event pairs cost
    launch-bound calls real time) and, from two more profiled calls, the per-kernel HIP-event durations."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        r = fn()
    torch.cuda.synchronize()
    el = (time.perf_counter() - t0) / iters
    best = {}
    for _ in range(2):                      # two profiled calls, per kernel the shorter one (a single call now and then catches a hiccup)
        ops.profile_enable(True)
        ops.profile_reset()
        fn()
        torch.cuda.synchronize()
        ops.profile_enable(False)
        for k, v in ops.profile_dump().items():
            best[k] = min(best.get(k, float("inf")), v["ms"])
    return el, r, {k: round(v, 4) for k, v in sorted(best.items(), key=lambda kv: -kv[1])}


def stage_b1(ext, qu_img, sampler=None, label="322x322"):
    """The way the reference's scripts call the extractor (scripts/dino_v2_vlad.py:169-183: one image per call): ViT-g/14
    at B = 1, tokens on the device: ~225 small launches whose own fill / k-step chain / drain is the time (dispatch
    timestamps: 98 % inside the kernels, 0.17 us between them -- profiles/r04_b1_kernel_trace_gaps.md).  ``qu_img`` [>=8,3,H,W]:
    322 x 322 (the bench shape) or 476 x 630 = the scripts' default ``resize=[480, 640]`` (configs.py:141) centre-cropped
    to multiples of 14 (scripts/dino_v2_vlad.py:173-176): 34 x 45 patches, T = 1531."""
    imgs = [qu_img[i:i + 1] for i in range(8)]
    n_patch = (qu_img.shape[-2] // 14) * (qu_img.shape[-1] // 14)
    state = {"i": 0}

    def one():
        state["i"] = (state["i"] + 1) % len(imgs)
        return ext(imgs[state["i"]])
    el, tok, kern = _timed(one, iters=40, warm=5)
    # the same image as image 0 of a batch gives bitwise the same tokens (per-row arithmetic does not depend on the batch);
    # elsewhere in a batch its rows fall into other GLOBAL 32-row groups of attention_h3's per-tile scales: the
    # same arithmetic on a differently grouped quantisation, equal to ~1e-7
    # one image per call runs the small-M plans (other tile shapes, split-K: another summation order over k than the same
    # image inside a batch); both meet the oracle bar and agree to ~1e-7
    batch = ext(qu_img[:8])
    first = float((ext(imgs[0]) - batch[0:1]).abs().max())
    other = float((ext(imgs[3]) - batch[3:4]).abs().max())
    fl = flops_per_image(n_patch=n_patch)
    res = {"workload": f"DinoV2ExtractFeatures.__call__ at B=1, ViT-G/14 L31 value, {label}, T = {n_patch + 1} "
                       "(the reference scripts' calling convention)",
           "ms_per_image": round(el * 1e3, 3), "images_per_s": round(1.0 / el, 1),
           "bound": "latency inside ~225 small launches (98 % of the time is inside kernels of a few hundred tiles each: fill, "
                    "per-k-step chain, drain; 0.17 us between dependent launches -- DESIGN.md 4.1d)",
           "achieved": round(fl / el / 1e12, 1), "unit": "TFLOP/s (algorithmic)",
           "frac_of_fp16_div3_peak": round(fl / el / 1e12 / (PEAK_BF16_MFMA_TFLOPS / 3), 4), "kernels_ms": kern,
           "oracle_ok": bool(max(first, other) <= 2e-6), "max_abs_diff_vs_batch_position_0": first,
           "max_abs_diff_vs_batch_position_3": other}
    if sampler is not None:                 # (a separate, untimed loop: the sampler idles while `el` is measured)
        sampler.resume()
        t_a = time.perf_counter()
        for _ in range(40):
            one()
        torch.cuda.synchronize()
        t_b = time.perf_counter()
        sampler.pause()
        res["power"] = sampler.window(t_a, t_b)
        res["power"]["ms_per_image_while_sampling"] = round((t_b - t_a) / 40 * 1e3, 3)
    return res


def stage_script_path(ext, vlad, db, qu_img, gt, n_img=256):
    """The reference scripts' own call pattern at the headline size, on the `utilities` surface, end to end:
    per image ``ext(img[None].to(device)).cpu()`` (scripts/dino_v2_vlad.py:164-188), then ``VLAD.generate_multi`` on the
    CPU tensor of all patch descriptors (:236-260), then ``get_top_k_recall`` on CPU tensors (:372) -- database VLADs
    included: the script holds them as a CPU tensor too.  Checked against the batched device path of the same images."""
    import utilities
    dev = db.device
    n_img = min(n_img, qu_img.shape[0])
    imgs_cpu = qu_img[:n_img].cpu()                       # the dataset's tensors live on the host
    db_cpu = db.cpu()
    gt_pos = np.empty(n_img, dtype=object)
    for i in range(n_img):
        gt_pos[i] = np.array([i])                         # query i depicts database place i (bench setup)

    cat_s = [0.0]

    def extract():
        patch_descs = []
        for i in range(n_img):
            img = imgs_cpu[i].to(dev)                     # as the script: one image, .to(device)
            ret = ext(img[None, ...])
            patch_descs.append(ret.cpu())
        c0 = time.perf_counter()
        full = torch.cat(patch_descs, dim=0)              # [n_img, 529, 1536] on the host: the script's own torch.cat,
        cat_s[0] = time.perf_counter() - c0               # 832 MB of host memcpy into fresh pages -- no device work
        return full

    extract()                                             # warm-up (allocator, pinned pages, clocks)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    full_qu = extract()
    t1 = time.perf_counter()
    qu_vlads = vlad.generate_multi(full_qu)
    t2 = time.perf_counter()
    dists, indices, recalls = utilities.get_top_k_recall([1, 5, 10, TOPK], db_cpu, qu_vlads, gt_pos)
    t3 = time.perf_counter()
    total = t3 - t0
    # breakdown of the per-image loop from an instrumented pass (a sync after every leg; not the timed pass)
    legs = {"h2d": 0.0, "forward": 0.0, "d2h": 0.0}
    for i in range(min(n_img, 64)):
        torch.cuda.synchronize(); a = time.perf_counter()
        img = imgs_cpu[i].to(dev); torch.cuda.synchronize(); b = time.perf_counter()
        ret = ext(img[None, ...]); torch.cuda.synchronize(); c = time.perf_counter()
        ret.cpu(); d = time.perf_counter()
        legs["h2d"] += b - a; legs["forward"] += c - b; legs["d2h"] += d - c
    legs = {k: round(v / min(n_img, 64) * 1e3, 3) for k, v in legs.items()}
    # VLAD.generate_multi on the CPU tensor (reference contract utilities.py:892-926: CPU in -> CPU out), leg by leg, from an
    # instrumented pass of exactly what anyloc_amd/vlad.py:_generate_batch does: host -> device copy of the 832 MB of patch
    # descriptors, the fused kernel, the [n_img, 49152] result back; then the call itself a second time (device buffers of
    # the first call are back in the allocator's pool: what is left is the copy)
    gm = {}
    torch.cuda.synchronize(); a = time.perf_counter()
    x_dev = ops._f32c(full_qu, dev); torch.cuda.synchronize(); b = time.perf_counter()
    v_dev = ops.vlad(x_dev, vlad._centers_dev()); torch.cuda.synchronize(); c = time.perf_counter()
    v_host = ops.to_home(v_dev, full_qu.device); d = time.perf_counter()
    gm.update({"h2d_ms": round((b - a) * 1e3, 2), "h2d_gb_per_s": round(full_qu.numel() * 4 / (b - a) / 1e9, 1),
               "kernel_call_ms": round((c - b) * 1e3, 2), "d2h_ms": round((d - c) * 1e3, 2),
               "bytes_in": int(full_qu.numel() * 4), "bytes_out": int(v_host.numel() * 4)})
    del x_dev, v_dev
    a = time.perf_counter()
    again = vlad.generate_multi(full_qu)
    gm["second_call_total_ms"] = round((time.perf_counter() - a) * 1e3, 2)
    gm["second_call_equal"] = bool(torch.equal(again, qu_vlads))
    del again, v_host
    # the same images through the batched device path (what the headline line times).  One image per call runs other GEMM
    # plans than a batch (another summation order over k): tokens agree to ~1e-7, which may flip the cluster id of a token
    # whose two best centres are tied to fp32 rounding -- such a flip (float64 gap of the two centres' cosines < 1e-6) is
    # not an error; VLADs are compared on the images without one
    tok_b = torch.cat([ext(qu_img[s:s + 32]) for s in range(0, n_img, 32)])
    tok_s = full_qu.to(dev)
    tok_err = float((tok_b - tok_s).abs().max())
    cdev = vlad.c_centers.to(dev)
    vl_b, lab_b = ops.vlad(tok_b, cdev, return_labels=True)
    vl_s, lab_s = ops.vlad(tok_s, cdev, return_labels=True)
    flips = (lab_b != lab_s).reshape(n_img, -1)
    gap = 0.0
    if bool(flips.any()):
        t64 = torch.nn.functional.normalize(tok_s.reshape(-1, tok_s.shape[-1])[flips.reshape(-1)].double(), dim=1)
        sc = t64 @ torch.nn.functional.normalize(cdev.double(), dim=1).T
        la, lb = lab_b.reshape(-1)[flips.reshape(-1)], lab_s.reshape(-1)[flips.reshape(-1)]
        gap = float((sc.gather(1, la[:, None]) - sc.gather(1, lb[:, None])).abs().max())
    clean = ~flips.any(dim=1)
    rel = float(((vl_b - vl_s).norm(dim=1) / vl_s.norm(dim=1))[clean].max()) if bool(clean.any()) else 0.0
    same_as_direct = bool(torch.equal(vl_s.cpu(), qu_vlads))            # generate_multi(CPU tensor) == the device call
    d_b, i_b = retrieval.search(db, vl_s, TOPK)
    top1_same = int((i_b[:, 0].cpu() == indices[:, 0]).sum())
    ok = tok_err <= 2e-6 and rel <= 1e-5 and gap < 1e-6 and top1_same == n_img and same_as_direct
    return {"workload": f"reference script call pattern, ViT-G/14 L31 value 322x322 K=32: {n_img} images one per call "
                        "(.to(device) -> extractor -> .cpu()), VLAD.generate_multi on the CPU tensor, get_top_k_recall of CPU "
                        f"tensors against the {db.shape[0]}-row database (host -> device copy of the database included)",
            "images_per_s": round(n_img / total, 1), "ms_per_image": round(total / n_img * 1e3, 3),
            "legs_ms": {"extract_loop_per_image": round((t1 - t0) / n_img * 1e3, 3),
                        "of_which_host_concat_per_image": round(cat_s[0] / n_img * 1e3, 3),
                        "generate_multi_total": round((t2 - t1) * 1e3, 2), "get_top_k_recall_total": round((t3 - t2) * 1e3, 2),
                        "per_image_instrumented": legs, "generate_multi_legs": gm},
            "recall": {str(k): v for k, v in recalls.items()},
            "vs_batched_device_path": {"token_max_abs_diff": tok_err, "label_flips": int(flips.sum()),
                                       "largest_float64_gap_of_a_flip": gap, "vlad_max_rel_diff_in_images_without_a_flip": rel,
                                       "cpu_tensor_path_bitwise_equals_device_call": same_as_direct,
                                       "top1_identical_to_device_search": top1_same, "of": n_img},
            "oracle_ok": bool(ok)}


def stage_kmeans(dev, check):
    """BASELINE.json configs[3]: one k-means iteration (assign + update, anyloc_kmeans_step) over 5 M x 1536 cached patch
    features, K = 32; HBM-bound: 30.72 GB read once per iteration.  Rows = 32 von-Mises-like modes + noise."""
    n, d, k = 5_000_000, 1536, 32
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    modes = torch.nn.functional.normalize(torch.randn(k, d, generator=g, device=dev), dim=1)
    x = torch.empty(n, d, dtype=torch.float32, device=dev)
    for s in range(0, n, 250_000):
        e = min(n, s + 250_000)
        pick = torch.randint(0, k, (e - s,), generator=g, device=dev)
        x[s:e] = torch.nn.functional.normalize(modes[pick] + (0.6 / d ** 0.5) * torch.randn(e - s, d, generator=g, device=dev), dim=1)
    np.random.seed(42)
    init = x[torch.as_tensor(np.random.choice(n, size=[k], replace=False), device=dev)].clone()
    # iteration 1 assigns against the drawn rows (several of them from the same mode: many near-ties); the later iterations
    # of the fit against settled centroids -- both are timed, the fit spends its time in the second kind
    el1, (sums, counts, _), kern1 = _timed(lambda: ops.kmeans_step(x, init, "cosine", False), iters=3)
    c = init
    for _ in range(3):
        sums, counts, _ = ops.kmeans_step(x, c, "cosine", False)
        c = torch.where(counts[:, None] > 0, sums / counts[:, None], torch.zeros_like(sums))
    el, (sums, counts, _), kern = _timed(lambda: ops.kmeans_step(x, c, "cosine", False), iters=5)
    k_ms = sum(kern.values())
    res = {"workload": "BASELINE.json configs[3]: k-means assign+update step, 5M x 1536 fp32 rows, K=32 (cosine)",
           "ms_per_iteration": round(el * 1e3, 3), "ms_first_iteration": round(el1 * 1e3, 3), "kernel_ms": round(k_ms, 3),
           "bound": "hbm", "algorithmic_bytes": n * d * 4,
           "achieved": round(n * d * 4 / (k_ms * 1e-3) / 1e12, 3), "peak": PEAK_HBM_TBPS, "unit": "TB/s",
           "frac": round(n * d * 4 / (k_ms * 1e-3) / 1e12 / PEAK_HBM_TBPS, 4),
           "achieved_wall": round(n * d * 4 / el / 1e12, 3), "kernel_ms_note": KERNEL_MS_NOTE, "kernels_ms": kern, "kernels_ms_first_iteration": kern1,
           "rows_counted": float(counts.sum()), "oracle_ok": None}
    # the whole fit through the class the reference touches (fpk surface: init rows from NumPy's global RNG, <= 100 iterations,
    # tol 1e-4; anyloc_amd/kmeans.py): iterations to converge and wall time
    from anyloc_amd import kmeans as hk
    np.random.seed(42)
    km = hk.KMeans(k, mode="cosine")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    km.fit(x)
    torch.cuda.synchronize()
    res["fit"] = {"iterations": int(km.n_iter_), "seconds": round(time.perf_counter() - t0, 3), "max_iter": km.max_iter, "tol": km.tol,
                  "modes_recovered": int((torch.nn.functional.normalize(km.centroids, dim=1) @ modes.T).max(0)[0].gt(0.99).sum())}
    if check:
        # the whole fit on the first 200 000 rows against the fpk restatement run on the host from the same drawn rows:
        # same number of iterations, same centroids
        from oracle import vlad_ref as _vr
        m2 = 200000
        draw = np.random.RandomState(5).choice(m2, size=[k], replace=False)
        g_fit = hk.KMeans(k, mode="cosine")
        g_fit.fit(x[:m2], centroids=x[:m2][torch.as_tensor(draw, device=dev)])
        c_ref, it_ref = _vr.kmeans_fit(x[:m2].cpu(), k, norm_descs=False, mode="cosine", init_idx=draw)
        cerr = float((g_fit.centroids.cpu() - c_ref).abs().max())
        res["fit"].update({"oracle_rows": m2, "oracle_iterations": int(it_ref), "subset_iterations": int(g_fit.n_iter_),
                           "oracle_centroid_max_abs_diff": cerr, "oracle_ok": bool(int(it_ref) == int(g_fit.n_iter_) and cerr < 1e-5)})
        # the same kernel on the first 20 000 rows against the fpk restatement (labels by cosine arg-max, sums of the rows)
        from oracle import vlad_ref
        m = 20000
        s_g, c_g, l_g = ops.kmeans_step(x[:m], init, "cosine", True)
        xc, cc = x[:m].cpu(), init.cpu()
        sc = vlad_ref.fpk_cosine_scores(xc, cc)
        l_r = sc.argmax(1)
        top2 = sc.topk(2, dim=1)[0]
        flips = l_g.cpu() != l_r
        tie_only = bool(((top2[:, 0] - top2[:, 1])[flips] < 1e-6).all()) if flips.any() else True
        s_r = torch.zeros(k, d, dtype=torch.float64).index_add_(0, l_g.cpu(), xc.double())
        err = float((s_g.cpu().double() - s_r).abs().max() / s_r.abs().max())
        res.update({"oracle_ok": bool(tie_only and err < 1e-5 and float(c_g.sum()) == m and res["fit"]["oracle_ok"]), "oracle_rows": m,
                    "oracle_label_flips": int(flips.sum()), "oracle_sums_rel_err": err})
    del x
    torch.cuda.empty_cache()
    return res


def stage_vlad(dev, vlad, n_img, check, toks=None):
    """The fused hard-assignment VLAD kernel alone (anyloc_vlad_hard) on n_img images of 529 x 1536 tokens, K = 32 (the bench
    vocabulary); HBM-bound: (N D + 2 K D) 4 B = 3.64 MB per image.  ``toks`` None: synthetic descriptor-like tokens
    around 32 random modes that are NOT the vocabulary's (every third row then has a close second centre: the screening kernel's
    worst case, rounds 2-4's stage); otherwise the tokens handed in -- the pipeline's own ViT-g tokens of the bench's query
    images, which the vocabulary was built on images like."""
    real = toks is not None
    if toks is None:
        toks = synth.clustered_tokens(n_img, 529, 1536, n_modes=32, seed=11, noise=0.6, device=str(dev))
    c = vlad.c_centers.to(dev)
    el, v, kern = _timed(lambda: ops.vlad(toks, c), iters=20, warm=2)
    per_img = (529 * 1536 + 2 * 32 * 1536) * 4
    k_ms = kern.get("vlad_fused", sum(kern.values()))      # the roofline is the kernel's; the call's wall time alongside
    res = {"workload": f"fused VLAD kernel, {n_img} images x 529 tokens x 1536, K=32, " +
                       ("the pipeline's own ViT-G/14 L31 tokens of the bench's query images" if real else
                        "synthetic tokens around 32 modes unrelated to the vocabulary"), "kernel_ms": round(k_ms, 4),
           "call_kernels_ms": round(sum(kern.values()), 4),      # + the centre preparation launch (normalised centres, byte table)
           "call_wall_ms": round(el * 1e3, 4), "bound": "hbm", "algorithmic_bytes": per_img * n_img,
           "achieved": round(per_img * n_img / (k_ms * 1e-3) / 1e12, 3), "peak": PEAK_HBM_TBPS, "unit": "TB/s",
           "frac": round(per_img * n_img / (k_ms * 1e-3) / 1e12 / PEAK_HBM_TBPS, 4),
           "achieved_wall": round(per_img * n_img / el / 1e12, 3),
           "kernel_ms_note": KERNEL_MS_NOTE, "kernels_ms": kern, "oracle_ok": None}
    if check:
        from oracle import vlad_ref
        worst = 0.0
        for j in (0, n_img // 2, n_img - 1):
            v_ref = vlad_ref.vlad_hard(toks[j].cpu(), c.cpu())[0]
            worst = max(worst, float((v[j].cpu() - v_ref).norm() / v_ref.norm()))
        res.update({"oracle_ok": worst <= 1e-5, "oracle_vlad_rel_err": worst})
    return res


def stage_config3_shard(dev, check):
    """BASELINE.json configs[2], the share of ONE GPU of the eight: 10 000 query VLADs against a 125 000-row shard
    (24.6 GB) of the 1 M x 49 152 database, cosine top-20 with the database normalised inside the search."""
    nq, ndb, dv = 10000, 125000, K_CLUSTERS * 1536
    db = synthetic_db(ndb, K_CLUSTERS, 1536, dev, seed=100)
    qu = synthetic_db(nq, K_CLUSTERS, 1536, dev, seed=500)
    rows = torch.arange(64, device=dev) * 17 + 5
    qu[:64] = 0.9 * db[rows] + 0.1 * qu[:64]
    # one-shot: `get_top_k_recall`'s own order of work -- index.add + index.search per call (utilities.py:439-450): every call
    # quantises the shard into the score GEMM's operand images.  Resident shard (what configs[2] describes: the database stays in
    # HBM, queries arrive): retrieval.FlatIndex prepares those images ONCE (round 6) and a retrieval only scores and merges.
    el1, (d1, i1), kern1 = _timed(lambda: retrieval.search(db, qu, TOPK), iters=2, warm=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index = retrieval.FlatIndex(db, "cosine", planes=True)
    torch.cuda.synchronize()
    t_build = time.perf_counter() - t0
    el, (d, i), kern = _timed(lambda: index.search(qu, TOPK), iters=2, warm=1)
    same_lists = bool(torch.equal(i, i1) and torch.equal(d, d1))
    screened = "topk_screen_gemm" in kern
    # round 6: the default search is SCREENED (csrc/scores_screen.hip: leading-plane score panels under a proven bound + float64
    # re-scoring of the rows inside it); the three-product panels of rounds 3-5 timed next to it on the same index
    with ops.options(topk_screen=0):
        el_u, (d_u, i_u), kern_u = _timed(lambda: index.search(qu, TOPK), iters=1, warm=1)
    lists_differ = int((i_u != i).sum())
    dist_diff = float((d_u - d).abs().max())
    del index
    # float64 check of the screened lists: 32 queries against the whole shard (the products in row blocks: no float64 copy of it)
    sel = torch.arange(0, nq, nq // 32, device=dev)[:32]
    qn64 = torch.nn.functional.normalize(qu[sel].double())
    s64 = torch.empty(len(sel), ndb, dtype=torch.float64, device=dev)
    for r0 in range(0, ndb, 8192):
        s64[:, r0:r0 + 8192] = qn64 @ torch.nn.functional.normalize(db[r0:r0 + 8192].double()).t()
    o64 = torch.sort(s64, dim=1, descending=True, stable=True)
    got64 = torch.gather(s64, 1, i[sel])
    f64_mism = i[sel] != o64.indices[:, :TOPK]
    f64_ok = bool((not f64_mism.any()) or float((got64[f64_mism] - o64.values[:, :TOPK][f64_mism]).abs().max()) <= 3e-6)
    f64_err = float((d[sel].double() - got64).abs().max())
    del s64, o64, qn64
    flops = 2.0 * nq * ndb * dv
    planted = bool((i[:64, 0] == rows).all()) and same_lists
    peak = PEAK_BF16_MFMA_TFLOPS if screened else PEAK_BF16_MFMA_TFLOPS / 3
    res = {"workload": "BASELINE.json configs[2], one shard: 10k queries x 125k rows x 49152-d, top-20 (cosine, normalise inside); "
                       "`ms` / `frac`: a retrieval against the RESIDENT shard (operand images prepared once: retrieval.FlatIndex = "
                       "faiss index.add), `ms_one_shot`: index.add + search in one call, as get_top_k_recall does; `ms_unscreened`: the "
                       "three-product score panels of rounds 3-5 on the same index (option topk_screen = 0)",
           "ms": round(el * 1e3, 2), "ms_one_shot": round(el1 * 1e3, 2), "index_build_ms": round(t_build * 1e3, 2),
           "ms_unscreened": round(el_u * 1e3, 2), "speedup_vs_unscreened": round(el_u / el, 3), "screened": screened,
           "frac_unscreened_of_peak_over_3": round(flops / el_u / 1e12 / (PEAK_BF16_MFMA_TFLOPS / 3), 4),
           "screened_vs_unscreened": {"indices_that_differ": lists_differ, "of": int(i.numel()), "max_abs_distance_difference": dist_diff},
           "float64_check": {"queries": int(len(sel)), "ok": f64_ok, "index_mismatches": int(f64_mism.sum()), "max_abs_distance_error": f64_err},
           "kernels_ms_one_shot": kern1, "kernels_ms_unscreened": kern_u,
           "resident_lists_equal_one_shot": same_lists,
           "queries_per_s": round(nq / el, 1), "bound": "mfma", "achieved": round(flops / el / 1e12, 2),
           "unit": "TFLOP/s (algorithmic, fp32-equivalent)", "peak": round(peak, 1),
           "frac": round(flops / el / 1e12 / peak, 4),
           "peak_note": "screened search: ONE fp16 matrix-core product per k on the leading planes (dense 16-bit peak 2500) + an exact "
                        "re-scoring of the rows inside the bound; `frac` = algorithmic flops / time / 2500.  Rounds 3-5 (`ms_unscreened`): "
                        "three products per k, priced against 2500 / 3 = 833.3 (`frac_unscreened_of_peak_over_3`); "
                        "`vs_fp32_mfma_peak` = achieved / 157.3 (the roofline of the round-2 fp32-MFMA panels)",
           "vs_fp32_mfma_peak": round(flops / el / 1e12 / PEAK_FP32_MFMA_TFLOPS, 4),
           "kernels_ms": kern, "planted_neighbours_found": planted, "oracle_ok": bool(planted and f64_ok) if screened else None}
    if check:
        # the many-query panel path on a slice the CPU can score: 96 queries x 3000 rows vs the flat-index restatement
        from oracle import faiss_flat
        qs, dbs = qu[:96], db[:3000]
        d_g, i_g = retrieval.search(dbs, qs, TOPK)
        d_r, i_r = faiss_flat.flat_search(torch.nn.functional.normalize(qs.cpu()), torch.nn.functional.normalize(dbs.cpu()), TOPK)
        same = bool(torch.equal(i_g.cpu(), i_r))
        derr = float((d_g.cpu() - d_r).abs().max())
        res.update({"oracle_ok": bool(planted and same and derr <= 3e-6 and f64_ok), "oracle_indices_equal": same, "oracle_dist_err": derr})
    del db, qu
    torch.cuda.empty_cache()
    return res


def stage_vitl(dev, check, B=23):
    """BASELINE.json configs[4]: ViT-L/14 518 x 518 (1369 tokens), taps at layers 20 and 23 ('value') concatenated to
    2048-d, K = 64 VLAD (131 072-d): 64 database + 16 query images end to end (extract_multi -> VLAD -> top-20).
    Batches of 23 images = 31 510 token rows = 247 row tiles of 128: the 247 x {4, 12, 16} tile grids of the D = 1024 GEMMs fill
    96.5 % of whole rounds of the 512 resident workgroups (what B = 61 is for ViT-g); batches of 16 leave the two N = 1024
    GEMMs at 688 tiles = 1.34 rounds (profiles/r04_vitl_batch.log; batches of 8: 309 images/s, of 16: 339)."""
    import utilities
    name, layers, K, hw = "dinov2_vitl14", [20, 23], 64, 518
    sd = synth.synthetic_state_dict(name, seed=0, device=str(dev))
    weights.register_state_dict(name, sd)
    try:
        ext = utilities.DinoV2ExtractFeatures(name, 23, "value", device=str(dev))
        db_img, qu_img, gt = synth.synthetic_places(64, 16, hw, hw, seed=5, device=str(dev))
        toks = torch.cat([ext.extract_multi(db_img[s:s + B], layers) for s in range(0, 64, B)])
        vl = utilities.VLAD(K, None, cache_dir=None)
        np.random.seed(42)
        vl.fit(toks.reshape(-1, toks.shape[-1]))
        del toks

        all_img = torch.cat([db_img, qu_img])

        def run():
            v = torch.cat([vl.generate_multi(ext.extract_multi(all_img[s:s + B], layers)) for s in range(0, 80, B)])
            return retrieval.search(v[:64], v[64:], TOPK)
        el, (dist_, idx), kern = _timed(run, iters=2, warm=1)
        rec = retrieval.recalls_from_indices([1, 5, 10], idx.cpu().numpy(), gt)
        T = 1370
        f_block = 2 * T * 1024 * 3072 + 4 * T * T * 1024 + 2 * T * 1024 * 1024 + 16 * T * 1024 * 1024
        f_img = 2 * 1369 * 588 * 1024 + 23 * f_block + 2 * T * 1024 * 1024 + 2 * T * 1024 * 3072
        res = {"workload": f"BASELINE.json configs[4]: ViT-L/14 518x518, taps L20+L23 'value' -> 2048-d, K=64 VLAD (131072-d), 64 db + 16 qu in batches of {B}",
               "images_per_s": round(80 / el, 2), "ms": round(el * 1e3, 2), "bound": "mfma",
               "achieved": round(80 * f_img / el / 1e12, 1), "unit": "TFLOP/s (algorithmic, fp32-equivalent)",
               "peak": round(PEAK_BF16_MFMA_TFLOPS / 3, 1), "frac": round(80 * f_img / el / 1e12 / (PEAK_BF16_MFMA_TFLOPS / 3), 4),
               "recall": rec, "kernels_ms": kern, "oracle_ok": None}
        if check:
            # one image through the CPU oracle at full depth (24 blocks run, taps at 20 and 23), tokens of both taps
            from oracle import dinov2_ref
            model = dinov2_ref.build(name, {k: v.cpu() for k, v in sd.items()})
            img = qu_img[:1].cpu()
            ref = torch.cat([dinov2_ref.extract_facet(model, img, l, "value") for l in layers], dim=-1)
            ref = torch.nn.functional.normalize(ref, dim=-1)
            got = ext.extract_multi(qu_img[:1], layers).cpu()
            err = float((got - ref).abs().max())
            res.update({"oracle_ok": err <= 2e-5, "oracle_token_max_abs_err": err})
    finally:
        weights.unregister_state_dict(name)
    torch.cuda.empty_cache()
    return res


def stage_config2_full_job(dev, n_db=10000, n_qu=1000, B=61):
    """BASELINE.json configs[1] as ONE complete job through the reference's class surface (`utilities`), on the driver's clock:
    10 000 database + 1 000 query images of 322 x 322 (synthetic places, generated on the device) -> DINOv2 ViT-G/14 layer-31
    `value` tokens -> vocabulary (`VLAD.fit` on the tokens of every 20th database image) -> K = 32 VLADs of all 11 000 images
    -> `get_top_k_recall` of the 1 000 x 10 000 x 49 152 search (what scripts/dino_v2_vlad.py:125-303 does, batches of 61
    instead of one image per call).  Checks: every VLAD unit-norm; indices, distances and recalls of all 1 000 retrievals
    identical to an exact float64 flat search over the job's own VLADs."""
    import utilities
    legs = {}

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        legs[name] = round(time.perf_counter() - t0, 3)
        return out
    db_img, qu_img, gt = timed("synthesise_images_s", lambda: synth.synthetic_places(n_db, n_qu, HW, HW, seed=42, device=str(dev)))
    ext = utilities.DinoV2ExtractFeatures(MODEL, LAYER, FACET, device=str(dev))
    vl = utilities.VLAD(K_CLUSTERS, desc_dim=None, cache_dir=None)

    def vocabulary():
        sub = db_img[::20]
        toks = torch.cat([ext(sub[i:i + B]) for i in range(0, len(sub), B)])
        np.random.seed(42)
        vl.fit(toks.reshape(-1, toks.shape[-1]))
        return int(toks.shape[0] * toks.shape[1])

    def describe(imgs):
        out = torch.empty(len(imgs), K_CLUSTERS * 1536, dtype=torch.float32, device=dev)
        for i in range(0, len(imgs), B):
            out[i:i + B] = vl.generate_multi(ext(imgs[i:i + B]))
        return out
    n_tok = timed("vocabulary_s", vocabulary)
    db_v = timed("database_vlads_s", lambda: describe(db_img))
    qu_v = timed("query_vlads_s", lambda: describe(qu_img))
    dists, idx, recalls = timed("get_top_k_recall_s", lambda: utilities.get_top_k_recall([1, 5, 10, TOPK], db_v, qu_v, gt))
    descr = legs["database_vlads_s"] + legs["query_vlads_s"]
    job = descr + legs["vocabulary_s"] + legs["get_top_k_recall_s"]
    unit = bool(torch.allclose(db_v.norm(dim=1), torch.ones(n_db, device=dev), atol=1e-4))
    # every one of the job's retrievals against an exact float64 flat search over its own VLADs (indices, distances, recalls)
    t_idx = torch.as_tensor(np.asarray(idx.cpu() if torch.is_tensor(idx) else idx), device=dev)
    t_dst = torch.as_tensor(np.asarray(dists.cpu() if torch.is_tensor(dists) else dists), device=dev)
    rchk = retrieval_identity([(t_dst, t_idx, qu_v)], db_v, gt)
    res = {"workload": f"BASELINE.json configs[1] as one job: {n_db} database + {n_qu} query images 322x322 -> ViT-G/14 L31 value -> "
                       f"K=32 VLAD -> top-{TOPK} of {n_qu} x {n_db} x {K_CLUSTERS * 1536} (utilities.DinoV2ExtractFeatures / VLAD / "
                       f"get_top_k_recall, batches of {B})",
           "seconds": round(job, 2), "legs_s": legs, "vocabulary_tokens": n_tok, "kmeans_iterations": int(vl.kmeans.n_iter_),
           "describe_images_per_s": round((n_db + n_qu) / descr, 1), "images_per_s": round((n_db + n_qu) / job, 1),
           "recalls": {str(k): float(v) for k, v in recalls.items()}, "vlads_unit_norm": unit,
           "recall_note": "random-init weights: Recall@k says how often a noisy, shifted query finds its own synthetic place, not how "
                          "good DINOv2 is; the check is identity with the float64 search",
           "retrieval_vs_float64": {k: rchk[k] for k in ("queries", "index_mismatches", "near_tie_swaps", "max_distance_err",
                                                         "recall_identical", "ok")},
           "oracle_ok": bool(unit and rchk["ok"])}
    del db_img, qu_img, db_v, qu_v, ext
    torch.cuda.empty_cache()
    return res


def stage_config3_whole_db(dev, nq=10000, ndb=1_000_000):
    """BASELINE.json configs[2] WHOLE on one GPU: 10 000 query VLADs against the full 1 M x 49 152 database (196.6 GB) resident
    in this GPU's HBM, cosine top-20 (what eight GPUs do on 125 000-row shards each; the sharded route is `--workload
    config3 --gpus N`).  Skipped with a note where the free HBM does not hold it."""
    dv = K_CLUSTERS * 1536
    need = ndb * dv * 4 + nq * dv * 4 + (12 << 30)               # database + queries + operand images / score panels / slack
    free, total = torch.cuda.mem_get_info(dev)
    if free < need:
        return {"workload": "BASELINE.json configs[2] whole on one GPU", "skipped": f"free HBM {free / 2**30:.0f} GiB < {need / 2**30:.0f} GiB",
                "oracle_ok": None}
    t0 = time.perf_counter()
    db = synthetic_db(ndb, K_CLUSTERS, 1536, dev, seed=100)
    qu = synthetic_db(nq, K_CLUSTERS, 1536, dev, seed=500)
    rows = (torch.arange(64, device=dev) * 15013 + 5) % ndb
    qu[:64] = 0.9 * db[rows] + 0.1 * qu[:64]
    torch.cuda.synchronize()
    t_gen = time.perf_counter() - t0
    retrieval.search(db[:8192], qu[:64], TOPK)                   # warm-up of the kernels / workspaces on a small panel
    torch.cuda.synchronize()
    ops.profile_enable(True)                                     # (a handful of scopes per retrieval: which kernels scored it)
    ops.profile_reset()
    t0 = time.perf_counter()
    d, i = retrieval.search(db, qu, TOPK)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    ops.profile_enable(False)
    kern = {k: round(v["ms"], 2) for k, v in sorted(ops.profile_dump().items(), key=lambda kv: -kv[1]["ms"])}
    screened = "topk_screen_gemm" in kern and "topk_scores_gemm" not in kern
    peak = PEAK_BF16_MFMA_TFLOPS if screened else PEAK_BF16_MFMA_TFLOPS / 3
    planted = bool((i[:64, 0] == rows).all())
    flops = 2.0 * nq * ndb * dv
    res = {"workload": f"BASELINE.json configs[2] WHOLE on one GPU: {nq} queries x {ndb} rows x {dv}-d resident in HBM ({ndb * dv * 4 / 1e9:.1f} GB), top-{TOPK}",
           "seconds_per_retrieval": round(el, 3), "queries_per_s": round(nq / el, 1), "generate_db_s": round(t_gen, 1), "bound": "mfma",
           "achieved": round(flops / el / 1e12, 1), "unit": "TFLOP/s (algorithmic, fp32-equivalent)", "peak": round(peak, 1),
           "frac": round(flops / el / 1e12 / peak, 4), "screened": screened, "kernels_ms": kern,
           "peak_note": "screened search (one fp16 product per k + exact re-scoring): dense 16-bit peak 2500; unscreened: 2500 / 3",
           "planted_neighbours_found": planted, "oracle_ok": planted}
    del db, qu, d, i
    _lib.release_workspaces()
    torch.cuda.empty_cache()
    return res


def run_stages(dev, vlad, check, real_tokens=None):
    """`stages`: everything the north star names besides the headline line, timed in this process after it."""
    out = {}
    t0 = time.time()
    out["vlad_61img"] = stage_vlad(dev, vlad, 61, check)
    out["vlad_256img"] = stage_vlad(dev, vlad, 256, False)
    if real_tokens is not None:
        out["vlad_61img_pipeline_tokens"] = stage_vlad(dev, vlad, 61, check, real_tokens[:61])
        if real_tokens.shape[0] >= 256:
            out["vlad_256img_pipeline_tokens"] = stage_vlad(dev, vlad, 256, False, real_tokens[:256])
        del real_tokens
    _lib.release_workspaces()
    torch.cuda.empty_cache()
    out["kmeans_5Mx1536"] = stage_kmeans(dev, check)
    out["config3_shard"] = stage_config3_shard(dev, check)
    out["vitl_518_2taps"] = stage_vitl(dev, check)
    out["seconds"] = {"value": round(time.time() - t0, 1)}
    return out


if __name__ == "__main__":
    main()
