"""The reference's call patterns on the HIP path (``pytest -m gpu``):

* a hub-layout ``.pth`` on disk (a random-init ``transformers.Dinov2Model`` remapped to the facebookresearch key names) is found
  through ``ANYLOC_DINOV2_WEIGHTS`` and gives the tokens the HF model itself computes (reference ``utilities.py:239-242``:
  ``torch.hub.load`` + ``.eval().to(device)``);
* the host <-> device transfers, and the scripts' CPU-tensor call pattern through ``VLAD.generate_multi`` / ``get_top_k_recall``;
* the call sequence of ``scripts/dino_v2_vlad.py`` as bench.py's stage and as a driver under ``python -m anyloc_amd.run``.

The reference's own ``scripts/dino_v2_vlad.py`` is not run here: a GPU test reads nothing outside this tree.  The script runs
unmodified on the CPU oracle backend in tests/test_reference_scripts_cpu.py, its call sequence runs on the HIP path below
(tests/drivers/vlad_driver_standin.py), and tools/reference_scripts_on_hip.py runs the reference's scripts on the HIP path
wherever a reference tree is at hand."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _retrieval_refs import vlad_like_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def hf_to_hub(hf_sd, depth, swiglu):
    """transformers.Dinov2Model state dict -> facebookresearch/dinov2 key layout (the inverse of the remap in
    tests/test_oracle_dinov2_hf.py): fused qkv, ``ls*.gamma``, ``mlp.w12 / w3``."""
    sd = {"cls_token": hf_sd["embeddings.cls_token"], "mask_token": hf_sd["embeddings.mask_token"],
          "pos_embed": hf_sd["embeddings.position_embeddings"],
          "patch_embed.proj.weight": hf_sd["embeddings.patch_embeddings.projection.weight"],
          "patch_embed.proj.bias": hf_sd["embeddings.patch_embeddings.projection.bias"],
          "norm.weight": hf_sd["layernorm.weight"], "norm.bias": hf_sd["layernorm.bias"]}
    for i in range(depth):
        p, q = f"blocks.{i}.", f"encoder.layer.{i}."
        sd[p + "attn.qkv.weight"] = torch.cat([hf_sd[q + f"attention.attention.{n}.weight"] for n in ("query", "key", "value")])
        sd[p + "attn.qkv.bias"] = torch.cat([hf_sd[q + f"attention.attention.{n}.bias"] for n in ("query", "key", "value")])
        sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"] = hf_sd[q + "attention.output.dense.weight"], hf_sd[q + "attention.output.dense.bias"]
        for n in ("norm1", "norm2"):
            sd[p + n + ".weight"], sd[p + n + ".bias"] = hf_sd[q + n + ".weight"], hf_sd[q + n + ".bias"]
        sd[p + "ls1.gamma"], sd[p + "ls2.gamma"] = hf_sd[q + "layer_scale1.lambda1"], hf_sd[q + "layer_scale2.lambda1"]
        if swiglu:
            sd[p + "mlp.w12.weight"], sd[p + "mlp.w12.bias"] = hf_sd[q + "mlp.weights_in.weight"], hf_sd[q + "mlp.weights_in.bias"]
            sd[p + "mlp.w3.weight"], sd[p + "mlp.w3.bias"] = hf_sd[q + "mlp.weights_out.weight"], hf_sd[q + "mlp.weights_out.bias"]
        else:
            for f in ("fc1", "fc2"):
                sd[p + f"mlp.{f}.weight"], sd[p + f"mlp.{f}.bias"] = hf_sd[q + f"mlp.{f}.weight"], hf_sd[q + f"mlp.{f}.bias"]
    return {k: v.detach().clone().contiguous() for k, v in sd.items()}


def test_hub_layout_checkpoint_file_through_env(tmp_path, monkeypatch):
    transformers = pytest.importorskip("transformers")
    import utilities
    from anyloc_amd import weights
    from oracle import dinov2_ref
    name, layer = "dinov2_vits14", 9
    dim, depth, heads, ffn, hidden = dinov2_ref.ARCH[name]
    torch.manual_seed(5)
    cfg = transformers.Dinov2Config(hidden_size=dim, num_hidden_layers=depth, num_attention_heads=heads, mlp_ratio=4,
                                    image_size=518, patch_size=14, layerscale_value=1.0, use_swiglu_ffn=False,
                                    layer_norm_eps=1e-6, qkv_bias=True, hidden_act="gelu", attn_implementation="eager")
    hf = transformers.Dinov2Model(cfg).eval()
    with torch.no_grad():                                   # HF initialises biases to zero: give the file real ones
        for n_, p_ in hf.named_parameters():
            if n_.endswith(".bias"):
                p_.normal_(0.0, 0.02)
    path = tmp_path / f"{name}_pretrain.pth"                # the file name facebookresearch publishes
    torch.save(hf_to_hub(hf.state_dict(), depth, False), str(path))
    weights.unregister_state_dict()
    monkeypatch.setenv("ANYLOC_DINOV2_WEIGHTS", str(tmp_path))      # a directory holding <name>_pretrain.pth ...
    ext = utilities.DinoV2ExtractFeatures(name, layer, "value", device="cuda")
    monkeypatch.setenv("ANYLOC_DINOV2_WEIGHTS", str(path))          # ... or the file itself
    ext_file = utilities.DinoV2ExtractFeatures(name, layer, "value", device="cuda:0")
    g = torch.Generator().manual_seed(1)
    img = torch.randn(2, 3, 518, 518, generator=g)          # native grid: HF and the hub code use the same positional table
    got = ext(img.to("cuda")).cpu()
    assert torch.equal(got, ext_file(img.to("cuda")).cpu())
    with torch.no_grad():
        hs = hf(pixel_values=img, output_hidden_states=True).hidden_states[layer]
        lay = hf.encoder.layer[layer]
        v_hf = torch.nn.functional.normalize(lay.attention.attention.value(lay.norm1(hs))[:, 1:], dim=-1)
        model = dinov2_ref.build(name, torch.load(str(path)))
        v_or = dinov2_ref.extract_facet(model, img, layer, "value")
    assert got.shape == (2, 1369, dim)
    assert float((got - v_or).abs().max()) < 2e-5            # the restated hub model on the same file
    assert float((got - v_hf).abs().max()) < 1e-4            # the independent implementation the file came from


def test_host_device_transfers_round_trip():
    """ops.to_device / ops.to_host (the product's only host <-> device copies) move bytes unchanged: small and large tensors,
    non-contiguous sources, other dtypes, pinned sources."""
    from anyloc_amd import ops as staging
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(0)
    for shape, dtype in (((7, 13), torch.float32), ((3, 322, 322), torch.float32), ((40, 529, 1536), torch.float32),
                         ((9_000_001,), torch.int64), ((5, 3), torch.float64), ((0, 4), torch.float32)):
        t = (torch.randn(shape, generator=g) * 100).to(dtype)
        on = staging.to_device(t, dev)
        assert on.is_cuda and on.dtype == dtype and torch.equal(on.cpu(), t)
        back = staging.to_host(on)
        assert back.device.type == "cpu" and torch.equal(back, t)
    t = torch.randn(300, 400, generator=g)
    nc = t.t()[5:200:3]                                          # non-contiguous view
    assert torch.equal(staging.to_device(nc, dev).cpu(), nc)
    pinned = torch.randn(1000, 100, generator=g).pin_memory()
    assert torch.equal(staging.to_device(pinned, dev).cpu(), pinned)


def test_cpu_tensor_call_pattern_equals_the_device_path():
    """What scripts/dino_v2_vlad.py does (:236-260, :372): CPU patch descriptors -> VLAD.generate_multi -> CPU VLADs ->
    get_top_k_recall with a CPU database.  Bitwise the results of the same calls on device tensors."""
    import utilities
    g = torch.Generator().manual_seed(3)
    tok = torch.nn.functional.normalize(torch.randn(37, 529, 1536, generator=g), dim=-1)
    vlad = utilities.VLAD(32, 1536, cache_dir=None)
    np.random.seed(1)
    vlad.fit(tok[:8].reshape(-1, 1536))
    v_cpu = vlad.generate_multi(tok)
    v_dev = vlad.generate_multi(tok.to(DEV))
    assert v_cpu.device.type == "cpu" and v_dev.is_cuda and torch.equal(v_cpu, v_dev.cpu())
    vlad.HOST_CHUNK_BYTES = 10 * 529 * 1536 * 4                  # the chunked host path (pieces of 10 images): every piece runs with
    v_chunked = vlad.generate_multi(tok)                         # the whole batch's workgroups-per-image count -> the SAME bits
    assert torch.equal(v_chunked, v_cpu)
    db = vlad_like_rows(3000, 32, 1536, 9).cpu()
    db[5:42] = v_cpu
    gt = np.empty(37, dtype=object)
    for j in range(37):
        gt[j] = np.array([5 + j])
    d1, i1, r1 = utilities.get_top_k_recall([1, 5], db, v_cpu, gt)
    d2, i2, r2 = utilities.get_top_k_recall([1, 5], db.to(DEV), v_dev, gt)
    assert i1.device.type == "cpu" and torch.equal(i1, i2.cpu()) and torch.equal(d1, d2.cpu())
    assert r1 == r2 and r1[1] == 1.0


def test_reference_script_call_pattern_stage_on_a_small_model():
    """bench.py's `script_path_vitg` stage -- per image ``ext(img[None].to(device)).cpu()``, ``VLAD.generate_multi`` on the CPU
    tensor, ``get_top_k_recall`` on CPU tensors (scripts/dino_v2_vlad.py:164-188, :236-260, :372) -- on ViT-S/14 at 224 x 224:
    the stage's own check against the batched device path must hold (tokens, cluster ids, VLADs, top-1)."""
    import bench
    import utilities
    from anyloc_amd import synth, weights
    name = "dinov2_vits14"
    weights.register_state_dict(name, synth.synthetic_state_dict(name, 2, device=DEV, depth=10))
    try:
        ext = utilities.DinoV2ExtractFeatures(name, 9, "value", device=DEV)
        db_img, qu_img, gt = synth.synthetic_places(24, 24, 224, 224, seed=3, device=DEV)
        vlad = utilities.VLAD(8, None, cache_dir=None)
        tok = ext(db_img)
        np.random.seed(3)
        vlad.fit(tok.reshape(-1, tok.shape[-1]))
        db = torch.nn.functional.normalize(torch.randn(400, 8 * 384, generator=torch.Generator().manual_seed(1)), dim=1).to(DEV)
        db[:24] = vlad.generate_multi(tok)
        res = bench.stage_script_path(ext, vlad, db, qu_img, gt, n_img=24)
        assert res["oracle_ok"], res
        assert res["vs_batched_device_path"]["cpu_tensor_path_bitwise_equals_device_call"]
        assert res["images_per_s"] > 0
    finally:
        weights.unregister_state_dict(name)


def test_reference_call_pattern_driver_through_anyloc_amd_run(tmp_path):
    """``python -m anyloc_amd.run tests/drivers/vlad_driver_standin.py`` in a fresh interpreter on the GPU box: the reference
    driver's call sequence on the ``utilities`` surface (scripts/dino_v2_vlad.py:157-188, :195-260, :372-376) -- tyro CLI and
    torchvision transforms through the shims, one image per extractor call with ``.to(device)`` / ``.cpu()``, ``VLAD.fit`` +
    ``generate_multi`` with cache ids (``c_centers.pt``, ``_r/_l`` files), ``get_top_k_recall`` on CPU tensors -- twice: the
    second run restores the vocabulary and the VLADs from the cache and must print the same recalls and top-1 indices.
    (The reference's own script runs unmodified on the CPU oracle backend in tests/test_reference_scripts_cpu.py, and on the
    HIP path through tools/reference_scripts_on_hip.py wherever its tree exists.)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_synth_dataset
    make_synth_dataset.write(str(tmp_path / "data"), "st_lucia", n_db=6, n_qu=4, h=112, w=140)
    env = dict(os.environ, ANYLOC_SYNTHETIC_WEIGHTS="0", PYTHONPATH=ROOT)
    outs = []
    for _ in range(2):
        res = subprocess.run([sys.executable, "-m", "anyloc_amd.run", os.path.join(ROOT, "tests", "drivers", "vlad_driver_standin.py"),
                              "--data-dir", str(tmp_path / "data"), "--cache-dir", str(tmp_path / "cache"), "--num-clusters", "4"],
                             env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0 and "Traceback" not in res.stdout + res.stderr, (res.stdout[-2000:], res.stderr[-2000:])
        outs.append(res.stdout)
    for out in outs:
        assert "Database VLADs shape: torch.Size([6, 1536])" in out and "Query VLADs shape: torch.Size([4, 1536])" in out
        assert "device of the results: cpu cpu" in out
    pick = lambda out: [l for l in out.splitlines() if l.startswith("R@") or l.startswith("top-1")]
    assert pick(outs[0]) == pick(outs[1]) and len(pick(outs[0])) == 4
    assert "Using cached cluster centers" in outs[1] and "Using cached cluster centers" not in outs[0]
    rec = [float(l.split(":")[1]) for l in pick(outs[0])[:3]]
    assert 0.5 <= rec[0] <= rec[1] <= rec[2] <= 1.0, outs[0][-800:]    # query q depicts place q (random-weight ViT-S: mostly found)
    pts = [f for dp, _, fs in os.walk(tmp_path / "cache") for f in fs if f.endswith(".pt")]
    assert "c_centers.pt" in pts and any(f.endswith("_r.pt") for f in pts) and any(f.endswith("_l.pt") for f in pts)
