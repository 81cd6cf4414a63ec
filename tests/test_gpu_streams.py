"""The stream contract, op by op (``pytest -m gpu``): "all work of a call is enqueued on the caller's stream" (include/anyloc_hip.h,
"Streams"; INTEGRATION.md, "Streams").  Every case runs one op on a side stream whose inputs arrive LATE -- behind a chain of
matrix products -- into NaN-filled tensors, with NaN in every block the allocator can hand out (tests/_stream_harness.py): a
launch on another stream, a blocking memset or copy on the null stream, a helper that drops the stream, or a workspace shared
between streams reads NaN and the bits differ from the default-stream result.

Every case is in exactly one of two literal lists.  ASYNC_OPS: the call must return while its inputs do not exist yet
(``pending``) -- the case is conclusive and the op really is asynchronous.  SYNCING_OPS: the op waits for its stream somewhere
(a host read-back); the poison check still covers everything it enqueued before that.  SYNCING_ENTRY_POINTS names the C entry
points that synchronise by themselves -- the list include/anyloc_hip.h and INTEGRATION.md give, and the allow-list of
tests/test_stream_contract_cpu.py; every other syncing op waits in the PYTHON host (INTEGRATION.md lists those).

Measured on an MI355X (host time of the call, delay in front of the inputs): LABNOTES.md, "Stream-order tests".
"""
import pytest
import torch

from _op_cases import (TAPS, VIT, _cache, _cases, _fwd, _images, _model, _state_dict, _tokens, _topk_data, _unit, _with)

pytestmark = pytest.mark.gpu

ASYNC_OPS = [
    "l2norm_7x384", "l2norm_5x10", "layernorm_11x384", "pool_average_ragged", "pool_max_ragged", "pool_gem_ragged",
    "preprocess_u8", "preprocess_u8_bicubic",
    "gemm_nt_wide", "gemm_nt_narrow", "gemm_nt_530x8192x1536", "gemm_h3_129x384x592", "gemm_h3_small_m", "gemm_x6",
    "attention_f32", "attention_x6", "attention_h3_2x257x6", "attention_h3_1x20x3", "attention_h3_ks1", "attention_h3_ks2",
    "vlad_hard_fused_parts3", "vlad_hard_two_pass", "vlad_soft", "vlad_soft_weights", "vlad_assigned_soft", "vlad_residuals",
    "kmeans_step_fused", "kmeans_step_two_pass", "kmeans_update",
    "pca_gram_rows", "pca_gram_cols", "pca_axes",
    "topk_f32_ip_norm", "topk_f32_ip_raw", "topk_f32_l2_norm", "topk_f32_l2_raw", "topk_ndb0", "topk_fewq_qdma1", "topk_fewq_qdma0",
    "topk_h3_forced", "topk_index_build", "topk_index_build_range", "topk_indexed_unscreened", "flatindex_search",
    "vit_fwd_h3_uniform", "vit_fwd_x6_uniform", "vit_fwd_f32_uniform", "vit_fwd_h3_vitb_split_k",
    "vit_fwd_h3_ragged", "vit_fwd_x6_ragged", "vit_fwd_f32_ragged",
    "vit_fwd_h3_reg", "vit_fwd_x6_reg", "vit_fwd_f32_reg",
]
SYNCING_OPS = [
    # the C entry point itself waits (SYNCING_ENTRY_POINTS)
    "topk_screened", "topk_screened_fallback", "topk_indexed_screened_rows", "topk_indexed_screened_planes", "vit_attach_h2_direct",
    # the Python host waits: a host read of a device value ("Streams")
    "vlad_assigned_labels", "kmeans_fit_predict", "pca_fit_transform",
    "vit_build_h3", "vit_build_x6", "vit_build_f32", "vit_fwd_h3_uniform_ffn_check", "vit_fwd_h3_ragged_ffn_check",
    "reference_surface",
]
# C entry points that synchronise by themselves: the screened search reads a flag back (anyloc_topk on screened shapes, the
# indexed searches likewise), anyloc_vit_attach_h2 drains the device at construction time
SYNCING_ENTRY_POINTS = ("anyloc_topk", "anyloc_topk_search_index", "anyloc_topk_search_index_rows", "anyloc_vit_attach_h2")

TWO_STREAM_ASYNC = ["vlad_fused_vs_two_pass", "kmeans_step_vs_topk_h3", "two_extractors_h3"]
TWO_STREAM_SYNCING = ["two_flat_indexes_screened"]


# ---- the cases: tests/_op_cases.py (shared with tests/test_gpu_history.py) --------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    return _cases()


def test_every_case_is_in_exactly_one_list(cases):
    assert len(set(ASYNC_OPS)) == len(ASYNC_OPS) and len(set(SYNCING_OPS)) == len(SYNCING_OPS)
    assert not set(ASYNC_OPS) & set(SYNCING_OPS)
    assert set(cases) == set(ASYNC_OPS) | set(SYNCING_OPS)


@pytest.mark.parametrize("name", ASYNC_OPS + SYNCING_OPS)
def test_op_on_a_side_stream_behind_a_delayed_producer(cases, name):
    import _stream_harness as H
    case = cases[name]
    if "tags" in case or "check" in case:                     # the shape takes the path the case is about
        tags = H.tags_of(case["op"], case["inputs"])
        present, absent = case.get("tags", ([], []))
        assert all(t in tags for t in present) and not any(t in tags for t in absent), (name, sorted(tags))
        assert case.get("check", lambda t: True)(tags), (name, tags)
    H.run_case(name, case["op"], case["inputs"], asynchronous=name in ASYNC_OPS, in_place=case.get("in_place", False))


def test_one_image_forward_takes_a_split_k_plan():
    """vit_fwd_h3_vitb_split_k is there for the split-K tickets the forward zeroes with a memset on its stream: the fc2 GEMM of
    ViT-B at the 257 token rows of one 224 x 224 image splits K."""
    import _plan_edges as P
    from anyloc_amd import _lib
    plans = P.block_plans(_lib.load(), "dinov2_vitb14", 257)
    assert plans["fc2"]["ksplit"] > 1, plans


# ---- two streams at once -----------------------------------------------------------------------------------------------------
def _distinct_workspaces(*tags):
    def check(s1, s2):
        from anyloc_amd import _lib
        dev = torch.cuda.current_device()
        for tag in tags:
            a, b = _lib._workspaces.get((dev, s1.cuda_stream, tag)), _lib._workspaces.get((dev, s2.cuda_stream, tag))
            if a is not None and b is not None:
                assert a.data_ptr() != b.data_ptr(), tag
        mine = [k for k in _lib._workspaces if k[1] in (s1.cuda_stream, s2.cuda_stream)]
        assert {k[1] for k in mine} == {s1.cuda_stream, s2.cuda_stream}, mine          # each stream brought its own buffers
        ptrs = [_lib._workspaces[k].data_ptr() for k in mine]
        assert len(set(ptrs)) == len(ptrs)
    return check


def _two_stream_cases():
    from anyloc_amd import ops, retrieval
    from anyloc_amd.extractor import HipDinoV2
    c = {}
    tok, cen = _tokens(3, 300, 384, 80), 0.8 * _unit(8, 384, seed=81)
    tok512, cen40 = _tokens(3, 300, 512, 82), 0.8 * _unit(40, 512, seed=83)
    c["vlad_fused_vs_two_pass"] = (_with(lambda t, k: ops.vlad(t, k, return_labels=True), vlad_parts=3), [tok, cen],
                                   lambda t, k: ops.vlad(t, k, return_labels=True), [tok512, cen40], _distinct_workspaces("vlad"))
    x = _tokens(1, 5003, 384, 90)[0]
    q70, d256 = _topk_data(70, 300, 256, 130)
    c["kmeans_step_vs_topk_h3"] = (lambda a, k: ops.kmeans_step(a, k, "cosine", True), [x, 0.9 * _unit(16, 384, seed=91)],
                                   _with(lambda q, d: ops.topk(q, d, 5, "ip", normalize_db=True), topk_h3=1, topk_screen=0), [q70, d256],
                                   _distinct_workspaces())
    dev = torch.device("cuda", torch.cuda.current_device())
    m1, m2 = _model("h3"), HipDinoV2(VIT, _state_dict(), dev, gemm="h3")
    _cache["second_h3"] = m2
    c["two_extractors_h3"] = (_fwd(m1, False), [_images(2, 224, 224, 160)], _fwd(m2, False), [_images(2, 126, 154, 161)],
                              _distinct_workspaces("vit"))
    q2, d2 = _topk_data(70, 300, 256, 170)
    i1, i2 = retrieval.FlatIndex(d256, "cosine", True, planes=True), retrieval.FlatIndex(d2, "cosine", True, planes=True)
    scr = dict(topk_h3=1, topk_screen=1)
    c["two_flat_indexes_screened"] = (_with(lambda q: i1.search(q, 5), **scr), [q70], _with(lambda q: i2.search(q, 5), **scr), [q2],
                                      _distinct_workspaces("topk"))
    torch.cuda.synchronize()
    return c


@pytest.fixture(scope="module")
def two_stream_cases():
    return _two_stream_cases()


@pytest.mark.parametrize("name", TWO_STREAM_ASYNC + TWO_STREAM_SYNCING)
def test_two_streams_at_once(two_stream_cases, name):
    import _stream_harness as H
    op_a, in_a, op_b, in_b, between = two_stream_cases[name]
    if name == "two_flat_indexes_screened":
        assert "topk_screen_gemm" in H.tags_of(op_a, in_a)
    H.run_two_streams(name, op_a, in_a, op_b, in_b, asynchronous=name in TWO_STREAM_ASYNC, between=between)


# ---- the object rule of INTEGRATION.md, "Streams" -----------------------------------------------------------------------------
def test_an_extractor_moves_between_streams_with_wait_stream():
    """An extractor holds per-object device state (the positional tables it cached, its telemetry buffer): one stream at a time,
    and the hand-over is the caller's ``wait_stream`` -- exactly that, with a table first made on one stream and read on the
    other, against the default-stream results."""
    import _stream_harness as H
    from anyloc_amd.extractor import HipDinoV2
    dev = torch.device("cuda", torch.cuda.current_device())
    ref, model = _model("h3"), HipDinoV2(VIT, _state_dict(), dev, gemm="h3")
    a, b = _images(2, 224, 224, 180), _images(1, 126, 154, 181)
    ref.ffn_check = model.ffn_check = True
    want_a, want_b = ref.forward_taps(a, TAPS), ref.forward_taps(b, TAPS)
    torch.cuda.synchronize()
    s1, s2 = H._streams()
    with torch.cuda.stream(s1):
        H._delay().enqueue(H.MIN_DELAY_MS, 0)
        got_a = model.forward_taps(a, TAPS)                   # caches the 224 x 224 table on s1
    s2.wait_stream(s1)
    with torch.cuda.stream(s2):
        H._delay().enqueue(H.MIN_DELAY_MS, 1)
        got_b = model.forward_taps(b, TAPS)                   # caches the 126 x 154 table on s2
        got_a2 = model.forward_taps(a, TAPS)                  # reads the table s1 made
    s1.wait_stream(s2)
    with torch.cuda.stream(s1):
        got_b2 = model.forward_taps(b, TAPS)                  # reads the table s2 made
    torch.cuda.synchronize()
    for got, want in ((got_a, want_a), (got_a2, want_a), (got_b, want_b), (got_b2, want_b)):
        assert H.same_bits(got, want)
