"""Round 6 (``pytest -m gpu``): the overlapped sharded step on the prepared flat index, the workspace of a caller's
workgroups-per-image count, the gather hazard of the one-pass VLAD kernel, the FFN-bound telemetry and the
LayerNorm lead role.  The tests of the prepared index itself are in tests/test_gpu_topk_panels.py."""
import os

import numpy as np
import pytest
import torch

from _ranks import run_ranks
from _retrieval_refs import _screened_without_fallback, check_lists, exact_scores64, profiled, spread_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _prepared_shards_job(rank, world, out_dir):
    from anyloc_amd import retrieval
    dev = torch.device("cuda", 0)
    dim = 1024
    db, qu = spread_rows(5001, dim, 5), spread_rows(256, dim, 6)
    bounds = [0, 2100, 5001]
    shard = retrieval.FlatIndex(db[bounds[rank]:bounds[rank + 1]].to(dev), "cosine", planes=True)
    q_loc = qu[128 * rank:128 * (rank + 1)].to(dev)
    d_ref, i_ref = retrieval.search(db.to(dev), qu.to(dev), 10)
    for overlap in (True, False, "auto"):
        d, i = retrieval.sharded_search(shard, bounds[rank], q_loc, 10, counts=[128, 128], overlap=overlap)
        if rank == 0:
            assert np.array_equal(i, i_ref.cpu().numpy()), overlap
            np.testing.assert_allclose(d, d_ref.cpu().numpy(), atol=2e-6)
    if rank == 0:
        open(os.path.join(out_dir, "ok"), "w").write("1")


def _screened_shards_job(rank, world, out_dir):
    """The same step at a shape the SCREENED search serves (forced: topk_screen = 1): every rank's shard search scores on the
    leading planes and re-scores its candidates; the merged lists are checked against a float64 search over the whole database."""
    from anyloc_amd import ops, retrieval
    dev = torch.device("cuda", 0)
    dim = 4096
    db, qu = spread_rows(36000, dim, 7), spread_rows(600, dim, 8)
    bounds = [0, 17000, 36000]
    with ops.options(topk_screen=1, topk_h3=1):
        shard = retrieval.FlatIndex(db[bounds[rank]:bounds[rank + 1]].to(dev), "cosine", planes=True)
        q_loc = qu[300 * rank:300 * (rank + 1)].to(dev)
        outs = [retrieval.sharded_search(shard, bounds[rank], q_loc, 20, counts=[300, 300], overlap=ov) for ov in (True, False)]
        _, prof = profiled(lambda: retrieval.sharded_search(shard, bounds[rank], q_loc, 20, counts=[300, 300], overlap=True))
    assert _screened_without_fallback(prof), sorted(prof)
    if rank == 0:
        s = exact_scores64(torch.nn.functional.normalize(qu.to(dev).double()), db.to(dev), "ip")
        for d, i in outs:
            check_lists(torch.as_tensor(d, device=dev), torch.as_tensor(i, device=dev), s, 20, "ip", "screened shards", cap=None)
        assert np.array_equal(outs[0][1], outs[1][1])
        open(os.path.join(out_dir, "ok_screened"), "w").write("1")


def test_overlapped_sharded_step_with_the_screened_shard_search(tmp_path):
    run_ranks(_screened_shards_job, 2, tmp_path)
    assert (tmp_path / "ok_screened").exists()


def test_overlapped_sharded_step_on_a_prepared_shard_two_ranks_one_gpu(tmp_path):
    """The overlapped sharded step (own queries searched while the others' travel, the rest afterwards) on prepared shards with
    the real kernels: two ranks share cuda:0 over gloo; the merged lists are those of one flat search, with and without overlap."""
    run_ranks(_prepared_shards_job, 2, tmp_path)
    assert (tmp_path / "ok").exists()


def test_vlad_workspace_covers_a_callers_parts_count():
    """``ops.vlad(parts=p)`` with p above the library's own count for the batch (round 5's advisor finding: the workspace was
    sized for the library's count): sized by ``anyloc_vlad_workspace_bytes_parts`` now; out-of-range counts are refused in Python."""
    from anyloc_amd import ops, synth
    toks = synth.clustered_tokens(300, 529, 1536, n_modes=32, seed=5, noise=0.6, device=DEV)
    c = 0.8 * synth.clustered_tokens(1, 32, 1536, n_modes=32, seed=3, device=DEV)[0]
    assert ops.vlad_auto_parts(300, 300 * 529, 1536, 32) == 1
    with ops.options(vlad_two_pass=1):
        ref = ops.vlad(toks, c)
    for p in (8, 3, 64):
        got = ops.vlad(toks, c, parts=p)
        assert float(((got - ref).norm(dim=1) / ref.norm(dim=1)).max()) <= 1e-5, p
    for bad in (-1, 65, 128):
        with pytest.raises(ValueError):
            ops.vlad(toks, c, parts=bad)


def test_gather_hazard_variants_of_the_one_pass_vlad_kernel():
    """in GPR-index mode the first indexed VALU behind ``s_set_gpr_idx_on`` needs wait states.  The shipped
    gather (``s_nop`` behind every mode switch) is bitwise reproducible under load in BOTH residual arithmetics; the variant
    kept for the record (one fma, no wait state: option vlad_gather_v = 1) is the form round 5 found irreproducible -- it is
    only reported here, not asserted (a hazard is not obliged to fire)."""
    from anyloc_amd import ops, synth
    c = 0.8 * synth.clustered_tokens(1, 32, 1536, n_modes=32, seed=3, device=DEV)[0]
    toks = synth.clustered_tokens(400, 529, 1536, n_modes=32, seed=11, noise=0.6, device=DEV)
    with ops.options(vlad_two_pass=1):
        ref = ops.vlad(toks, c)
    report = {}
    for gv in (0, 2, 1):
        with ops.options(vlad_gather_v=gv):
            first = ops.vlad(toks, c).clone()
            differ = sum(int((ops.vlad(toks, c) != first).any(dim=1).sum()) for _ in range(10))
            wrong = int((((first - ref).norm(dim=1) / ref.norm(dim=1)) > 1e-5).sum())
        report[gv] = (wrong, differ)
        if gv != 1:
            assert (wrong, differ) == (0, 0), report
    print("gather variants (wrong vs two-pass, differing over 10 repeats):", report)


def test_ffn_telemetry_on_the_swiglu_epilogues_against_the_image_itself():
    """The rows' maxima the w12 epilogue leaves (atomicMax per row and wave) against the fc2 operand image itself: the figure of
    every (block, image) equals 2^15 / (largest |value| of the leading fp16 plane over the image's rows), on the transposed
    SwiGLU epilogue of ViT-g (one image: the 192 x 128 small-M plan; three images: 64 x 128 tiles) and on the row-major one
    (option h3_swiglu_t = 0).  The last executed block's image is still in the workspace after the call: it is checked directly;
    the other blocks' figures must be of the same order (a bound is above the maximum, not wildly)."""
    import utilities
    from anyloc_amd import ops, synth, weights
    name = "dinov2_vitg14"
    weights.register_state_dict(name, synth.synthetic_state_dict(name, 3, device=DEV, depth=3))
    try:
        for swiglu_t in (1, 0):
            with ops.options(h3_swiglu_t=swiglu_t):
                ext = utilities.DinoV2ExtractFeatures(name, 2, "token", device=DEV)
            m = ext.dino_model
            for batch in (1, 3):
                img = torch.randn(batch, 3, 322, 322, generator=torch.Generator().manual_seed(40 + batch)).to(DEV)
                tok = ext(img).clone()
                fig = m._telemetry[:3 * batch].cpu().reshape(3, batch)
                assert bool((fig > 1.0).all()) and bool((fig < 2.0 ** 14).all()), (swiglu_t, batch, fig)
                # the same call again: the same figures (atomicMax is order-independent) and tokens
                assert torch.equal(ext(img), tok)
                assert torch.equal(m._telemetry[:3 * batch].cpu().reshape(3, batch), fig)
                # an image alone reports the figures it has inside the batch to within the batch-position rounding
                if batch == 3:
                    ext(img[1:2])
                    alone = m._telemetry[:3].cpu()
                    assert float((alone / fig[:, 1] - 1).abs().max()) < 1e-3, (alone, fig[:, 1])
    finally:
        weights.unregister_state_dict(name)


@pytest.mark.parametrize("facet,layer", [("value", 2), ("token", 2), ("token", 1)])
def test_layernorm_lead_role_gives_the_bits_of_the_separate_launch(facet, layer):
    """One image per call (option h3s_ln_lead, csrc/gemm_h3_kernel.hpp): LayerNorm 1 / 2 run as the first workgroups of the qkv /
    w12 GEMM's own launch -- rows stored write-through into that GEMM's operand image, one relaxed agent-scope ticket per row tile,
    a GEMM workgroup waits for its tile's count and stages A with sc1 loads.  Same per-row arithmetic as layernorm_h2: the tokens
    must equal, bit for bit, those of the seven-launch block, on every one of 40 repeats (a stale operand row -- the failure this
    hand-off could have -- shows as a differing run), with and without the FFN-bound telemetry, at 322 x 322 (530 rows) and
    224 x 224 (257 rows); a 476 x 630 image (1 531 rows: more GEMM workgroups than the lead role allows) takes the separate
    launch under either setting.  `layer` 1 of 3 blocks leaves the last block's output unused; "value" keeps the v tap."""
    import utilities
    from anyloc_amd import ops, synth, weights
    name = "dinov2_vitg14"
    weights.register_state_dict(name, synth.synthetic_state_dict(name, 6, device=DEV, depth=3))
    try:
        ext = utilities.DinoV2ExtractFeatures(name, layer, facet, device=DEV)
        for hw, check in (((322, 322), True), ((322, 322), False), ((224, 224), True), ((476, 630), True)):
            ext.dino_model.ffn_check = check
            img = torch.randn(1, 3, *hw, generator=torch.Generator().manual_seed(hw[1])).to(DEV)
            with ops.options(h3s_ln_lead=0):
                want = ext(img).clone()
            assert torch.isfinite(want).all()
            with ops.options(h3s_ln_lead=1):
                for rep in range(40):
                    assert torch.equal(ext(img), want), (hw, check, rep, "the lead-role forward differs from the separate launches")
    finally:
        weights.unregister_state_dict(name)


def test_layernorm_lead_role_under_load_on_the_full_depth_forward():
    """The same hand-off with the chip busy: 32-block ViT-g forwards of one image, another stream running batched GEMM work
    meanwhile (its workgroups take CUs away from the lead launch in an order the launch does not choose); 30 forwards, one set of
    bits."""
    import utilities
    from anyloc_amd import ops, synth, weights
    name = "dinov2_vitg14"
    weights.register_state_dict(name, synth.synthetic_state_dict(name, 7, device=DEV, depth=32))
    try:
        ext = utilities.DinoV2ExtractFeatures(name, 31, "value", device=DEV)
        img = torch.randn(1, 3, 322, 322, generator=torch.Generator().manual_seed(5)).to(DEV)
        with ops.options(h3s_ln_lead=0):
            want = ext(img).clone()
        side = torch.cuda.Stream()
        a = torch.randn(4096, 4096, device=DEV)
        with ops.options(h3s_ln_lead=1):
            for rep in range(30):
                with torch.cuda.stream(side):
                    for _ in range(4):
                        a @ a
                assert torch.equal(ext(img), want), rep
        torch.cuda.synchronize()
    finally:
        weights.unregister_state_dict(name)


@pytest.mark.parametrize("name,hw,batch,facet", [("dinov2_vitg14", (322, 322), 17, "token"), ("dinov2_vitg14", (322, 322), 24, "value"),
                                                 ("dinov2_vitl14", (518, 518), 7, "token")])
def test_batched_layernorm_lead_role_gives_the_bits_of_the_separate_launch(name, hw, batch, facet):
    """Batched calls (option h3_ln_lead, csrc/gemm_h3_kernel.hpp LNL = 2, csrc/tile_order.hpp LeadPlan): LayerNorm 1 / 2 run as
    lead workgroups of 16 rows interleaved, per XCD, with the tiles of the qkv / w12 (ViT-L: fc1, GELU epilogue) GEMM's own launch;
    rows stored write-through, one ticket per 128-row tile, a GEMM tile waits for its row's count.  Same per-row arithmetic and
    store order as layernorm_h2_kernel: the tokens must equal, bit for bit, those of the separate launches on each of 12 repeats
    (a stale or missing operand row shows as a differing run).  >= 64 tile rows are needed for the plan (17 images x 530 rows)."""
    import utilities
    from anyloc_amd import ops, synth, weights
    weights.register_state_dict(name, synth.synthetic_state_dict(name, 8, device=DEV, depth=3))
    try:
        ext = utilities.DinoV2ExtractFeatures(name, 2, facet, device=DEV)
        img = torch.randn(batch, 3, *hw, generator=torch.Generator().manual_seed(batch)).to(DEV)
        for check in (True, False):
            ext.dino_model.ffn_check = check
            with ops.options(h3_ln_lead=0):
                ops.profile_enable(True); ops.profile_reset()
                want = ext(img).clone()
                torch.cuda.synchronize()
                assert "layernorm_h2" in ops.profile_dump()
            with ops.options(h3_ln_lead=1):
                ops.profile_reset()
                got = ext(img).clone()
                torch.cuda.synchronize()
                prof = ops.profile_dump()
                ops.profile_enable(False)
                # the lead role took the LayerNorm launches in front of the fused GEMMs (what is left: the last block's LN1 when a q / k / v
                # facet is tapped there)
                assert prof.get("layernorm_h2", {"calls": 0})["calls"] <= 1, prof.get("layernorm_h2")
                assert torch.isfinite(want).all() and torch.equal(got, want)
                for rep in range(12):
                    assert torch.equal(ext(img), want), (check, rep, "the lead-role forward differs from the separate launches")
    finally:
        ops.profile_enable(False)
        weights.unregister_state_dict(name)
