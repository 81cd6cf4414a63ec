"""Call history (``pytest -m gpu``): no op's result depends on what ran before it.  include/anyloc_hip.h ("Buffers"): a call
initialises every word of the workspace it depends on -- the workspace may hold anything at entry, another call's leftovers, another
shape's, garbage -- and the same holds for a ViT handle between two forwards and for the options after anyloc_reset_options.  The
words in question (tickets, row maxima, counts, flags) and the memset or store that initialises each: profiles/workspace_state_audit.md.

The bar is bit equality with the same call on a zero-filled workspace (tests/_history.py: ``baseline``), no tolerance.  Every case of
the catalogue (tests/_op_cases.py) runs
  a. on a workspace filled with each pattern of ``_history.PATTERNS``;
  b. as the victim behind each of DONORS, one per family that writes the workspace, on the same buffer;
  c. SEQUENCES: the same op at another shape or route first, every call against its own baseline;
  d. against a freshly built model after the handle and the Python model have a history;
  e. after an option was set, a donor ran under it and anyloc_reset_options was called; likewise around the profiler;
  f. on the real growing workspace of anyloc_amd/_lib.py across a reallocation, a release and a second stream.
tests/test_history_cpu.py plants the defects this module exists for in fake ops and requires the same harness to report them.

Measured on an MI355X (case counts, wall time): LABNOTES.md, "Call-history tests".
"""
import pytest
import torch

import _history as H
import _op_cases as O
import test_gpu_streams as S

pytestmark = pytest.mark.gpu

DEV = O.DEV
CATALOGUE = tuple(S.ASYNC_OPS + S.SYNCING_OPS)

# one per family that writes the workspace
DONORS = (
    "vit_fwd_h3_vitb_split_k", "vit_fwd_h3_ragged", "vit_fwd_h3_uniform_ffn_check", "vit_fwd_x6_uniform", "attention_h3_ks2",
    "vlad_hard_fused_parts3", "vlad_hard_two_pass", "vlad_soft", "kmeans_step_fused", "kmeans_step_two_pass",
    "topk_fewq_qdma1", "topk_h3_forced", "topk_screened", "topk_screened_fallback", "topk_indexed_screened_planes", "flatindex_search",
)

# cases of the sequences that the catalogue does not hold (built by _extra_cases)
EXTRA_CASES = (
    "fwd_h3_3x224_tap1", "fwd_h3_1x126x154_tap0", "fwd_h3_ragged3", "fwd_h3_3x224_tap1_telemetry_off",
    "fwd_vitg_2x224", "fwd_vitg_lead_1x322", "fwd_vitg_lead_1x224", "fwd_vitg_lead_1x476x630", "fwd_vitg_17x322", "fwd_vitg_batched_lead_17x322",
    "attention_h3_5x530x4",
    "vlad_hard_parts8", "vlad_hard_parts1", "vlad_hard_one_token",
    "kmeans_fused_40000", "kmeans_fused_15", "kmeans_two_pass_40000", "kmeans_two_pass_15",
    "topk4096_screened_k20", "topk4096_fewq3", "topk4096_screened_k5", "topk4096_fallback", "topk4096_screened_k5_no_wait", "topk4096_ndb0",
)
EXTRA_ELSEWHERE = ()          # extra cases that no sequence uses (none)

# c. the same op at another shape or route first; every call is compared with its own baseline
SEQUENCES = {
    # ViT-S/14, 2 blocks, h3, telemetry on unless said: the memset of tickets and row maxima is sized by rows, telemetry and last layer
    "forward_h3": ("fwd_h3_3x224_tap1", "fwd_h3_1x126x154_tap0", "fwd_h3_ragged3", "fwd_h3_3x224_tap1",
                   "fwd_h3_3x224_tap1_telemetry_off", "fwd_h3_3x224_tap1", "vit_fwd_h3_vitb_split_k"),
    # the shapes of test_layernorm_lead_role_gives_the_bits_of_the_separate_launch (one ViT-g image: option h3s_ln_lead) behind a
    # forward without the lead role, then the batched lead role (option h3_ln_lead: >= 64 tile rows of 128 = 17 images of 530 rows)
    "layernorm_lead": ("fwd_vitg_2x224", "fwd_vitg_lead_1x322", "fwd_vitg_2x224", "fwd_vitg_lead_1x224", "fwd_vitg_lead_1x476x630",
                       "fwd_vitg_lead_1x322", "fwd_vitg_17x322", "fwd_vitg_batched_lead_17x322", "fwd_vitg_lead_1x322"),
    "attention_h3": ("attention_h3_5x530x4", "attention_h3_1x20x3", "attention_h3_ks2", "attention_h3_ks1"),
    "vlad_hard": ("vlad_hard_parts8", "vlad_hard_parts1", "vlad_hard_fused_parts3", "vlad_hard_two_pass", "vlad_hard_one_token",
                  "vlad_hard_parts8"),
    "kmeans_step": ("kmeans_fused_40000", "kmeans_fused_15", "kmeans_step_fused", "kmeans_two_pass_40000", "kmeans_two_pass_15",
                    "kmeans_step_two_pass"),
    # one database of 300 rows x 4096 (the fallback case: 900 rows of it with 600 near-duplicates).  4096 columns because the
    # few-query path needs them: anyloc_topk_path(3, 300, 256) = 0 (fp32 panels), anyloc_topk_path(3, 300, 4096) = 1
    "topk": ("topk4096_screened_k20", "topk4096_fewq3", "topk4096_screened_k5", "topk4096_fallback", "topk4096_screened_k5",
             "topk4096_screened_k5_no_wait", "topk4096_screened_k5", "topk4096_ndb0"),
}

# e. option -> (the options set together: the named one at a legal non-default value, with the companions it needs to be legal;
#                the donor that runs under them; the victim that runs after anyloc_reset_options)
_H3S = dict(h3s_cfg=0, h3s_kb=1, h3s_ksplit=3, h3s_stages=6)          # (tests/test_gpu_vit.py: split-K forced on every block GEMM)
_FWD, _X6 = "vit_fwd_h3_uniform", "vit_fwd_x6_uniform"
OPTION_HISTORY = {
    "gemm_f32_cfg": (dict(gemm_f32_cfg=2), "vit_fwd_f32_uniform", "gemm_nt_wide"),
    "x6_cfg": (dict(x6_cfg=3), _X6, "gemm_x6"),
    "h3_cfg": (dict(h3_cfg=2), _FWD, "gemm_h3_129x384x592"),
    "h3_group_m": (dict(h3_group_m=3), _FWD, _FWD),
    "h3_tiny_max": (dict(h3_tiny_max=0, h3s_enable=0), _FWD, _FWD),
    "h3_deep_max": (dict(h3_deep_max=0, h3s_enable=0), _FWD, _FWD),
    "h3_deep2_max": (dict(h3_deep2_max=0, h3s_enable=0), _FWD, _FWD),
    "h3_epi_lds": (dict(h3_epi_lds=0), _FWD, _FWD),
    "ln_rows_per_wave": (dict(ln_rows_per_wave=2), _FWD, _FWD),
    "ln_small_rows": (dict(ln_small_rows=0), _FWD, _FWD),
    "ln_waves": (dict(ln_waves=4, ln_rows_per_wave=2), _FWD, _FWD),
    "ln_direct_rows": (dict(ln_direct_rows=0), _FWD, _FWD),
    "h3_fuse": (dict(h3_fuse=0), _FWD, "vit_fwd_h3_uniform_ffn_check"),
    "x6_fuse": (dict(x6_fuse=0), _X6, _X6),
    "h3_min_rows": (dict(h3_min_rows=100000), _FWD, _FWD),
    "x6_min_rows": (dict(x6_min_rows=5), "vit_fwd_x6_ragged", _X6),
    "attn_cfg": (dict(attn_cfg=1), "attention_f32", "attention_f32"),
    "attn_x6": (dict(attn_x6=1), "vit_fwd_f32_uniform", "vit_fwd_f32_uniform"),
    "vlad_parts": (dict(vlad_parts=8), "reference_surface", "vlad_hard_fused_parts3"),
    "vlad_two_pass": (dict(vlad_two_pass=1), "vlad_hard_fused_parts3", "vlad_hard_fused_parts3"),
    "vlad_fused_v": (dict(vlad_fused_v=1), "vlad_hard_fused_parts3", "vlad_hard_fused_parts3"),
    "kmeans_fused_v": (dict(kmeans_fused_v=1), "kmeans_step_fused", "kmeans_step_fused"),
    "kmeans_max_chunks": (dict(kmeans_max_chunks=1), "kmeans_step_fused", "kmeans_step_two_pass"),
    "h3_mfma16": (dict(h3_mfma16=1), "gemm_h3_small_m", "gemm_h3_small_m"),
    "h3_swiglu_t": (dict(h3_swiglu_t=0), "vit_build_h3", "vit_build_h3"),
    "h3_fast_silu": (dict(h3_fast_silu=0), _FWD, _FWD),
    "topk_fewq_x6": (dict(topk_fewq_x6=1), "topk_fewq_qdma1", "topk_fewq_qdma1"),
    "topk_h3": (dict(topk_h3=1), "topk_f32_ip_norm", "topk_f32_ip_norm"),
    "h3s_cfg": (_H3S, _FWD, _FWD),
    "h3s_ksplit": (_H3S, "vit_fwd_h3_uniform_ffn_check", "vit_fwd_h3_vitb_split_k"),
    "h3s_kb": (_H3S, "vit_fwd_h3_ragged", _FWD),
    "h3s_stages": (_H3S, _FWD, "vit_fwd_h3_ragged"),
    "h3s_mask": (dict(_H3S, h3s_mask=9), _FWD, _FWD),
    "h3s_enable": (dict(h3s_enable=0), "vit_fwd_h3_vitb_split_k", "vit_fwd_h3_vitb_split_k"),
    "h3_patch": (dict(h3_patch=0), _FWD, _FWD),
    "topk_fewq_qdma": (dict(topk_fewq_qdma=0), "topk_fewq_qdma0", "topk_fewq_qdma1"),
    "h3s_w12_tall": (dict(h3s_w12_tall=0), "vit_fwd_h3_vitb_split_k", "vit_fwd_h3_vitb_split_k"),
    "attn_h3_qg": (dict(attn_h3_qg=2), "attention_h3_2x257x6", "attention_h3_2x257x6"),
    "attn_h3_ks": (dict(attn_h3_ks=2), "attention_h3_2x257x6", "attention_h3_2x257x6"),
    "h3s_ln_lead": (dict(h3s_ln_lead=1), "vit_fwd_h3_vitb_split_k", "vit_fwd_h3_vitb_split_k"),
    "h3_ln_lead": (dict(h3_ln_lead=1), _FWD, _FWD),
    "topk_screen": (dict(topk_screen=1, topk_h3=1), "topk_f32_ip_norm", "topk_h3_forced"),
    "attn_h3_ragged_xcd": (dict(attn_h3_ragged_xcd=0), "vit_fwd_h3_ragged", "vit_fwd_h3_ragged"),
    "topk_rescore_cols": (dict(topk_rescore_cols=4096), "topk_screened", "topk_screened"),
}
# the variants of the hazard study are "not reproducible run to run" (csrc/vlad_fused.hip) and compiled for D = 1536 alone
OPTIONS_EXCLUDED = ("vlad_gather_v",)

from anyloc_amd import _lib as _real_lib  # noqa: E402

REAL_WORKSPACE = _real_lib.workspace
COUNTS = {}


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def _with_record(model, op):
    """``op`` of a forward with ``ffn_check``: its result and what the call left on the model -- the per-call looseness, the blocks
    switched to the exact quantiser and the re-runs of this call."""
    def run(*a):
        before = model.ffn_reruns
        out = op(*a)
        return out, model.ffn_looseness, set(model.ffn_exact_blocks), model.ffn_reruns - before
    return run


def _fwd_taps(model, ffn_check, taps, **options):
    def run(img):
        model.ffn_check = ffn_check
        return model.forward_taps(img, taps)
    return O._with(run, **options)


def _extra_cases(cat):
    from anyloc_amd import ops
    c = {}

    def case(name, op, inputs):
        assert name in EXTRA_CASES and name not in c and name not in cat, name
        c[name] = dict(op=op, inputs=inputs)

    # forward, ViT-S/14 with 2 blocks (the catalogue's model)
    m = O._model("h3")
    three = O._images(3, 224, 224, 200)
    case("fwd_h3_3x224_tap1", _with_record(m, O._fwd(m, True)), [three])
    case("fwd_h3_1x126x154_tap0", _with_record(m, _fwd_taps(m, True, [(0, "token")])), [O._images(1, 126, 154, 201)])
    rag = [O._images(1, 224, 224, 202)[0], O._images(1, 126, 154, 203)[0], O._images(1, 28, 28, 204)[0]]
    case("fwd_h3_ragged3", _with_record(m, O._fwd_ragged(m, True)), rag)
    case("fwd_h3_3x224_tap1_telemetry_off", O._fwd(m, False), [three])
    # LayerNorm lead role: ViT-g/14 with 2 blocks
    g = O._model("h3", "dinov2_vitg14")
    case("fwd_vitg_2x224", _with_record(g, O._fwd(g, True)), [O._images(2, 224, 224, 210)])
    for hw in ((322, 322), (224, 224), (476, 630)):
        name = f"fwd_vitg_lead_1x{hw[0]}" + ("" if hw[0] == hw[1] else f"x{hw[1]}")
        case(name, _with_record(g, O._fwd(g, True, h3s_ln_lead=1)), [O._images(1, hw[0], hw[1], 211 + hw[1])])
    many = O._images(17, 322, 322, 220)
    case("fwd_vitg_17x322", _with_record(g, O._fwd(g, True)), [many])
    case("fwd_vitg_batched_lead_17x322", _with_record(g, O._fwd(g, True, h3_ln_lead=1)), [many])
    # attention
    case("attention_h3_5x530x4", lambda x: ops.attention_h3(x, 4), [O._randn(5, 530, 3 * 256, seed=230)])
    # VLAD, the catalogue's tokens and centres
    tok, cen = cat["vlad_hard_fused_parts3"]["inputs"]
    for parts in (8, 1):
        case(f"vlad_hard_parts{parts}", O._with(lambda t, k: ops.vlad(t, k, return_labels=True), vlad_parts=parts), [tok, cen])
    case("vlad_hard_one_token", lambda t, k: ops.vlad(t, k, return_labels=True), [tok[:1, :1].contiguous(), cen])
    # k-means step, D = 384: K = 16 fused, K = 40 two-pass (the catalogue's 5003 rows and centres)
    x40k = O._tokens(1, 40000, 384, 240)[0]
    for kind, name in (("fused", "kmeans_step_fused"), ("two_pass", "kmeans_step_two_pass")):
        cen_k = cat[name]["inputs"][1]
        for n in (40000, 15):
            case(f"kmeans_{kind}_{n}", lambda a, k: ops.kmeans_step(a, k, "cosine", True), [x40k[:n].contiguous(), cen_k])
    # top-k on one database
    q70, db = O._topk_data(70, 300, 4096, 250)
    dup = O._topk_data(70, 900, 4096, 251)[1]
    dup[200:800] = (3.0 * q70[0]).expand(600, -1)
    scr = dict(topk_h3=1, topk_screen=1)

    def search(k, **kw):
        return O._with(lambda q, d: ops.topk(q, d, k, "ip", normalize_db=True, **kw), **scr)
    case("topk4096_screened_k20", search(20), [q70, db])
    case("topk4096_fewq3", lambda q, d: ops.topk(q, d, 7, "ip", normalize_db=True), [q70[:3].contiguous(), db])
    case("topk4096_screened_k5", search(5), [q70, db])
    case("topk4096_fallback", search(5), [q70, dup])
    case("topk4096_screened_k5_no_wait", search(5, no_wait=True), [q70, db])
    case("topk4096_ndb0", search(5), [q70, db[:0].clone()])
    torch.cuda.synchronize()
    return c


@pytest.fixture(scope="module")
def hist():
    mp = pytest.MonkeyPatch()
    ws = H.OwnedWorkspace(DEV).install(mp)
    try:
        cases = dict(O._cases())
        for name in ("vit_fwd_h3_uniform_ffn_check", "vit_fwd_h3_ragged_ffn_check"):
            cases[name] = dict(cases[name], op=_with_record(O._model("h3"), cases[name]["op"]))
        cases.update(_extra_cases(cases))
        torch.cuda.synchronize()
        yield H.History(ws, cases)
    finally:
        mp.undo()
        _forget_built_models()


def _forget_built_models():
    O._cache.get("built", []).clear()         # (vit_build_* keeps every model it builds alive: per call, not per session)


@pytest.fixture(autouse=True)
def _per_test():
    yield
    _forget_built_models()
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                 # a device fault is sticky: nothing more of this module may run on the card
        pytest.exit(f"the device reports an error after this test, the module stops here: {e}", returncode=3)


def _count(key, n=1):
    COUNTS[key] = COUNTS.get(key, 0) + n


def test_the_lists_name_cases_of_the_catalogue(hist):
    assert set(CATALOGUE) | set(EXTRA_CASES) == set(hist.cases)
    assert set(DONORS) <= set(CATALOGUE) and len(DONORS) == 16
    assert all(s in hist.cases for steps in SEQUENCES.values() for s in steps)
    assert {n for n, _ in H.NOT_BITWISE} <= set(CATALOGUE)
    # the routes the top-k sequence is about (host-only plan functions)
    lib = _real_lib.load()
    assert lib.anyloc_topk_path(3, 300, 4096) == 1 and lib.anyloc_topk_path(3, 300, 256) == 0
    tags = __import__("_stream_harness").tags_of
    c = hist.cases
    assert "topk_screen_gemm" in tags(c["topk4096_screened_k5"]["op"], c["topk4096_screened_k5"]["inputs"])
    fb = tags(c["topk4096_fallback"]["op"], c["topk4096_fallback"]["inputs"])
    assert "topk_screen_gemm" in fb and "topk_scores_gemm" in fb, sorted(fb)
    assert "topk_combine" in tags(c["topk4096_fewq3"]["op"], c["topk4096_fewq3"]["inputs"])
    # the lead roles took the LayerNorm launches
    plain = tags(c["fwd_vitg_17x322"]["op"], c["fwd_vitg_17x322"]["inputs"])["layernorm_h2"]
    lead = tags(c["fwd_vitg_batched_lead_17x322"]["op"], c["fwd_vitg_batched_lead_17x322"]["inputs"]).get("layernorm_h2", 0)
    assert lead < plain, (lead, plain)
    one = c["fwd_vitg_lead_1x322"]
    plain1 = tags(O._fwd(O._model("h3", "dinov2_vitg14"), True), one["inputs"])["layernorm_h2"]
    assert tags(one["op"], one["inputs"]).get("layernorm_h2", 0) < plain1
    assert tags(c["vlad_hard_parts8"]["op"], c["vlad_hard_parts8"]["inputs"]).get("vlad_fused", 0) >= 1


# ---- a. fill patterns -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", H.PATTERNS)
@pytest.mark.parametrize("name", CATALOGUE)
def test_case_on_a_filled_workspace(hist, name, pattern):
    hist.check_pattern(name, pattern, seed=CATALOGUE.index(name))
    _count("a. fill patterns")


# ---- b. other ops' leftovers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("donor", DONORS)
@pytest.mark.parametrize("victim", CATALOGUE)
def test_victim_behind_donor(hist, victim, donor):
    hist.check_behind(donor, victim)
    _count("b. donors")


# ---- c. the same op at another shape or route first ---------------------------------------------------------------------------------
@pytest.mark.parametrize("label", list(SEQUENCES))
def test_sequence_of_shapes_and_routes(hist, label):
    steps = list(SEQUENCES[label])
    hist.check_sequence(steps, label=label)
    # ... and behind hostile leftovers of the sequence's own largest call: every pattern in front of the whole sequence
    for pattern in H.PATTERNS[1:]:
        hist.ws.fill(pattern, seed=7)
        for n in steps:
            diff = hist.same(n, hist.run(n), hist.baseline(n))
            assert diff is None, f"{label}: {n} in the sequence started on {pattern!r} differs from its own baseline: {diff}"
    _count("c. sequences")
    _count("c. sequence calls", len(steps) * len(H.PATTERNS))


# ---- d. handle and model history ----------------------------------------------------------------------------------------------------
def _fresh_model():
    from anyloc_amd.extractor import HipDinoV2
    m = HipDinoV2(O.VIT, O._state_dict(), torch.device("cuda", torch.cuda.current_device()), gemm="h3")
    torch.cuda.synchronize()
    return m


def _record(model, img, taps=O.TAPS):
    model.ffn_check = True
    before = model.ffn_reruns
    out = model.forward_taps(img, taps)
    torch.cuda.synchronize()
    return H.frozen((out, model.ffn_looseness, set(model.ffn_exact_blocks), model.ffn_reruns - before))


def _same_as_fresh(used, img, what):
    got, want = _record(used, img), _record(_fresh_model(), img)
    diff = H.first_difference(got, want)
    assert diff is None, f"{what}: the used model differs from a freshly built one given the same call: {diff}"
    return got


def test_exact_switch_toggled_on_and_off_leaves_no_trace(hist):
    lib = _real_lib.load()
    used, img = _fresh_model(), O._images(2, 224, 224, 300)
    plain = _record(used, img)
    for l in (0, 1):
        _real_lib.check(lib.anyloc_vit_block_ffn_exact(used._handle, l, 1), "anyloc_vit_block_ffn_exact")
    exact = _record(used, img)
    # (both quantisers scale by a power of two: the tokens may keep their bits.  The telemetry tells them apart: a block on the
    # exact quantiser did not run fused and reports 0)
    assert not H.bits_equal(exact[1], plain[1]) and not exact[1].any(), "the exact switch is not observable: the toggle proves nothing"
    for l in (0, 1):
        _real_lib.check(lib.anyloc_vit_block_ffn_exact(used._handle, l, 0), "anyloc_vit_block_ffn_exact")
    assert H.first_difference(_same_as_fresh(used, img, "exact switch on, then off"), plain) is None


def test_a_clean_batch_behind_one_that_tripped_the_ffn_bound(hist, monkeypatch):
    """The trip: the second half of the recipe of test_vitg_reg_outlier_weights_and_ffn_rerun -- the threshold at 0, so that every
    image is run again with its blocks on the exact quantiser (switches set and cleared on the handle, re-runs counted on the
    model)."""
    from anyloc_amd import extractor as ex
    used, loud, clean = _fresh_model(), O._images(2, 224, 224, 301) * 4.0, O._images(3, 126, 154, 302)
    with monkeypatch.context() as mp:
        mp.setattr(ex, "FFN_LOOSENESS_MAX", 0.0)
        tripped = _record(used, loud)
    assert tripped[3] == 2 and tripped[2], tripped[2:]
    got = _same_as_fresh(used, clean, "a clean batch behind a tripping one")
    assert got[2] == frozenset() and got[3] == 0


def test_a_small_batch_behind_a_larger_one_shows_nothing_of_its_telemetry(hist):
    used = _fresh_model()
    big = _record(used, O._images(5, 224, 224, 303) * 8.0)
    assert used._telemetry.numel() == used.depth * 5
    got = _same_as_fresh(used, O._images(2, 224, 224, 304), "a batch of 2 behind a batch of 5")
    assert got[1].shape == big[1].shape and not H.bits_equal(got[1], big[1]), "both batches measure the same looseness: a leftover would not show"


def test_a_positional_table_from_the_cache_equals_the_first_one(hist):
    used, img = _fresh_model(), O._images(1, 126, 154, 305)
    miss = _record(used, img)
    assert H.first_difference(_record(used, img), miss) is None, "cache hit differs from the miss"
    used.ffn_check = False
    for i in range(20):
        used.forward_taps(O._images(1, 14 * (2 + i), 14 * (3 + i % 5), 306 + i), O.TAPS)
    assert len(used._pos_cache) >= 21
    assert H.first_difference(_same_as_fresh(used, img, "the table after 20 other sizes"), miss) is None


# ---- e. options and profiler history ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option", list(OPTION_HISTORY))
def test_option_set_donor_run_reset_then_victim(hist, option):
    from anyloc_amd import ops
    lib = _real_lib.load()
    values, donor, victim = OPTION_HISTORY[option]
    assert option in values
    want = hist.baseline(victim)
    hist.baseline(donor)                      # (sizes the buffers)
    defaults = {k: ops.get_option(k) for k in values}
    assert all(defaults[k] != v for k, v in values.items() if k == option), (option, defaults)
    try:
        for k, v in values.items():
            ops.set_option(k, v)
        hist.ws.fill("zero")
        hist.run(donor)
    finally:
        _real_lib.check(lib.anyloc_reset_options(), "anyloc_reset_options")
    assert {k: ops.get_option(k) for k in values} == defaults
    diff = hist.same(victim, hist.run(victim), want)
    assert diff is None, f"{victim} after {donor} ran under {values} and anyloc_reset_options differs from its baseline: {diff}"
    _count("e. options")


@pytest.mark.parametrize("donor", DONORS)
def test_profiler_on_around_a_donor_then_off(hist, donor):
    from anyloc_amd import ops
    victim = donor
    want = hist.baseline(victim)
    ops.profile_enable(True)
    ops.profile_reset()
    try:
        hist.ws.fill("zero")
        got_on = hist.run(donor)
    finally:
        ops.profile_enable(False)
        ops.profile_reset()
    assert hist.same(donor, got_on, want) is None, f"{donor} under the profiler differs from its baseline"
    diff = hist.same(victim, hist.run(victim), want)
    assert diff is None, f"{victim} after the profiler was on around {donor}: {diff}"
    _count("e. profiler")


# ---- f. host workspace life cycle (the real anyloc_amd._lib.workspace) -------------------------------------------------------------
LIFE_CYCLE = (("attention_h3_1x20x3", "attention_h3_5x530x4", "attn_h3"), ("fwd_h3_1x126x154_tap0", "fwd_h3_3x224_tap1", "vit"),
              ("vlad_hard_one_token", "vlad_hard_parts8", "vlad"), ("topk4096_fewq3", "topk4096_screened_k20", "topk"),
              ("kmeans_fused_15", "kmeans_fused_40000", "kmeans"))


def _buffer(tag, stream=None):
    stream = torch.cuda.current_stream().cuda_stream if stream is None else stream
    return _real_lib._workspaces.get((torch.cuda.current_device(), stream, tag))


@pytest.mark.parametrize("victim,donor,tag", LIFE_CYCLE, ids=[v for v, _, _ in LIFE_CYCLE])
@pytest.mark.parametrize("how", ["reallocated", "released", "second_stream"])
def test_real_workspace_life_cycle(hist, monkeypatch, victim, donor, tag, how):
    monkeypatch.setattr(_real_lib, "workspace", REAL_WORKSPACE)
    _real_lib.release_workspaces()
    torch.cuda.synchronize()
    first = hist.run(victim)
    small = _buffer(tag).numel()
    if how == "released":
        hist.run(donor)
        _real_lib.release_workspaces()
        again = hist.run(victim)
        assert _buffer(tag).numel() == small
    elif how == "reallocated":
        hist.run(donor)
        assert _buffer(tag).numel() > small, "the donor did not force a reallocation"
        again = hist.run(victim)
    else:
        hist.run(donor)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            again = hist.run(victim)
            assert _buffer(tag) is not None and _buffer(tag).data_ptr() != _buffer(tag, torch.cuda.default_stream().cuda_stream).data_ptr()
        torch.cuda.current_stream().wait_stream(side)
    diff = hist.same(victim, again, first)
    assert diff is None, f"{victim} ({how} behind {donor}) differs from its first run: {diff}"
    _real_lib.release_workspaces()
    _count("f. life cycle")


def test_counts():
    """(last: the case counts of LABNOTES.md, "Call-history tests")"""
    print("HISTORY", dict(catalogue=len(CATALOGUE), patterns=len(H.PATTERNS), donors=len(DONORS), extra_cases=len(EXTRA_CASES),
                          sequences={k: len(v) for k, v in SEQUENCES.items()}, options=len(OPTION_HISTORY), ran=COUNTS,
                          not_bitwise=H.NOT_BITWISE))
