"""The catalogue of ops (not a test module): one small case per entry point and route, ``_cases()`` -> name -> dict(op=, inputs=,
[tags=(present, absent)], [check=callable], [in_place=]).  tests/test_gpu_streams.py runs every case on a side stream behind a
delayed producer, tests/test_gpu_history.py behind other calls' leftovers in the workspace.  The shapes are the smallest that take
each route (ViT-S/14 with 2 blocks, 2 x 257 x 6 attention, 3 x 300 x 384 VLAD); models are built once per process (``_cache``).
"""
import ctypes as C

import numpy as np
import torch

DEV = "cuda"
VIT = "dinov2_vits14"
TAPS = [(1, "token")]
_cache = {}


def _randn(*shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV) * scale


def _unit(*shape, seed=0):
    return torch.nn.functional.normalize(_randn(*shape, seed=seed), dim=-1)


def _tokens(n_img, n_tok, dim, seed):
    from anyloc_amd import synth
    return synth.clustered_tokens(n_img, n_tok, dim, 12, seed=seed, device=DEV)


def _topk_data(nq, ndb, dim, seed):
    qu = _unit(nq, dim, seed=seed)
    db = _randn(ndb, dim, seed=seed + 1) * (0.3 + 2.0 * torch.rand(ndb, 1, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed + 2)))
    return qu, db


def _with(op, **options):
    """``op`` under library options (host-side switches read while the call enqueues)."""
    def run(*a):
        from anyloc_amd import ops
        with ops.options(**options):
            return op(*a)
    return run


def _state_dict(name=VIT):
    from anyloc_amd import synth
    return synth.synthetic_state_dict(name, 0, device=DEV, depth=2)


def _model(gemm, name=VIT):
    """One model per (arithmetic, architecture), built on the default stream and finished before any case uses it."""
    from anyloc_amd.extractor import HipDinoV2
    key = (gemm, name)
    if key not in _cache:
        _cache[key] = HipDinoV2(name, _state_dict(name), torch.device("cuda", torch.cuda.current_device()), gemm=gemm)
        torch.cuda.synchronize()
    return _cache[key]


def _images(b, h, w, seed):
    return _randn(b, 3, h, w, seed=seed)


def _fwd(model, ffn_check, **options):
    def run(img):
        model.ffn_check = ffn_check
        return model.forward_taps(img, TAPS)
    return _with(run, **options)


def _fwd_ragged(model, ffn_check, **options):
    def run(*imgs):
        model.ffn_check = ffn_check
        return model.forward_taps_ragged(list(imgs), TAPS)
    return _with(run, **options)


X6 = dict(x6_min_rows=0)          # (the split-bf16 forward is honoured from 1600 token rows up by default)


# ---- the cases: name -> () -> dict(op=, inputs=, [tags=(present, absent)], [check=callable], [in_place=]) -------------------------
def _cases():
    from anyloc_amd import _lib, ops, preprocess, retrieval
    from anyloc_amd.kmeans import KMeans
    from anyloc_amd.pca import PCA
    c = {}

    def case(name, op, inputs, **kw):
        assert name not in c, name
        c[name] = dict(op=op, inputs=inputs, **kw)

    # rows
    case("l2norm_7x384", ops.l2norm_rows, [_randn(7, 384, seed=1, scale=3.0)])
    case("l2norm_5x10", ops.l2norm_rows, [_randn(5, 10, seed=2, scale=3.0)])
    case("layernorm_11x384", ops.layernorm, [_randn(11, 384, seed=3), 1.0 + _randn(384, seed=4, scale=0.1), _randn(384, seed=5, scale=0.1)])
    ragged = [_randn(n, 384, seed=6 + n) for n in (37, 0, 300, 5)]
    case("pool_average_ragged", lambda *t: ops.pool(list(t), "average"), ragged)
    case("pool_max_ragged", lambda *t: ops.pool(list(t), "max"), [ragged[0], ragged[2], ragged[3]])
    case("pool_gem_ragged", lambda *t: ops.pool(list(t), "gem"), [ragged[0], ragged[2], ragged[3]])
    u8 = torch.randint(0, 256, (2, 126, 155, 3), dtype=torch.uint8, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    case("preprocess_u8", preprocess.images_to_input, [u8], tags=(["preprocess_u8"], ["resize_bicubic"]))
    case("preprocess_u8_bicubic", lambda x: preprocess.images_to_input(x, max_img_size=112), [u8],
         tags=(["preprocess_u8", "resize_bicubic"], []))

    # GEMMs
    def gemm(M, N, K, seed):
        return [_randn(M, K, seed=seed), _randn(N, K, seed=seed + 1), _randn(N, seed=seed + 2)]
    case("gemm_nt_wide", ops.gemm_nt, gemm(300, 256, 64, 10))
    case("gemm_nt_narrow", ops.gemm_nt, gemm(64, 17, 40, 20))
    case("gemm_nt_530x8192x1536", ops.gemm_nt, gemm(530, 8192, 1536, 30), tags=(["gemm_nt"], []))

    def gemm_h3(a, w, b):
        return ops.gemm_nt_h3(ops.split_h2(a), ops.split_h2(w), a.shape[0], w.shape[0], a.shape[1], b)
    case("gemm_h3_129x384x592", gemm_h3, gemm(129, 384, 592, 40), tags=(["split_h2", "gemm_h3"], []))
    case("gemm_h3_small_m", gemm_h3, gemm(129, 1536, 4096, 50), tags=(["split_h2", "gemm_h3"], []))
    case("gemm_x6", lambda a, w, b: ops.gemm_nt_x6(ops.split_x3(a), ops.split_x3(w), a.shape[0], w.shape[0], a.shape[1], b),
         gemm(130, 515, 112, 60), tags=(["split_x3", "gemm_x6"], []))

    # attention
    qkv = _randn(2, 257, 3 * 384, seed=70)
    case("attention_f32", _with(lambda x: ops.attention(x, 6), attn_x6=0), [qkv])
    case("attention_x6", _with(lambda x: ops.attention(x, 6), attn_x6=1), [qkv])
    case("attention_h3_2x257x6", lambda x: ops.attention_h3(x, 6), [qkv])
    case("attention_h3_1x20x3", lambda x: ops.attention_h3(x, 3), [_randn(1, 20, 3 * 192, seed=71)])
    case("attention_h3_ks1", _with(lambda x: ops.attention_h3(x, 6), attn_h3_ks=1), [qkv])
    case("attention_h3_ks2", _with(lambda x: ops.attention_h3(x, 6), attn_h3_ks=2), [qkv])

    # VLAD
    tok, cen = _tokens(3, 300, 384, 80), 0.8 * _unit(8, 384, seed=81)
    tok512, cen40 = _tokens(3, 300, 512, 82), 0.8 * _unit(40, 512, seed=83)
    case("vlad_hard_fused_parts3", _with(lambda t, k: ops.vlad(t, k, return_labels=True), vlad_parts=3), [tok, cen],
         tags=(["vlad_fused"], ["vlad_assign"]))
    case("vlad_hard_two_pass", lambda t, k: ops.vlad(t, k, return_labels=True), [tok512, cen40], tags=(["vlad_assign", "vlad_accumulate"], ["vlad_fused"]))
    case("vlad_soft", lambda t, k: ops.vlad(t, k, mode="soft", soft_temp=2.0), [tok, cen], tags=(["vlad_soft_accumulate"], []))
    case("vlad_soft_weights", lambda t, k: ops.vlad_soft_weights(t, k, 2.0), [tok[0], cen])
    labels = torch.randint(0, 8, (300,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(84))
    case("vlad_assigned_labels", lambda t, k, l: ops.vlad_assigned(t, k, labels=l), [tok[0], cen, labels])
    case("vlad_assigned_soft", lambda t, k, w: ops.vlad_assigned(t, k, soft=w), [tok[0], cen, torch.softmax(_randn(300, 8, seed=85), dim=1)])
    case("vlad_residuals", ops.vlad_residuals, [tok[0], cen], tags=(["vlad_residuals"], []))

    # k-means
    x = _tokens(1, 5003, 384, 90)[0]
    case("kmeans_step_fused", lambda a, k: ops.kmeans_step(a, k, "cosine", True), [x, 0.9 * _unit(16, 384, seed=91)],
         tags=([], ["kmeans_assign"]))
    case("kmeans_step_two_pass", lambda a, k: ops.kmeans_step(a, k, "cosine", True), [x, 0.9 * _unit(40, 384, seed=92)],
         tags=(["kmeans_assign", "kmeans_accumulate"], []))
    sums, counts, _ = ops.kmeans_step(x, 0.9 * _unit(16, 384, seed=91))
    case("kmeans_update", ops.kmeans_update, [sums, counts, 0.9 * _unit(16, 384, seed=91)], tags=(["kmeans_update"], []))
    x64 = _tokens(1, 2000, 64, 93)[0]

    def fit_predict(a, k):
        km = KMeans(8, max_iter=10, mode="cosine")
        lab = km.fit_predict(a, centroids=k)
        return lab, km.centroids
    case("kmeans_fit_predict", fit_predict, [x64, x64[:8].clone()])

    # PCA
    xp = _randn(70, 130, seed=100)
    mean64 = xp.double().mean(0)
    case("pca_gram_rows", lambda a, m: ops.pca_gram_f64(a, m, 0), [xp, mean64])
    case("pca_gram_cols", lambda a, m: ops.pca_gram_f64(a, m, 1), [xp, mean64])
    vec = torch.linalg.qr(_randn(70, 70, seed=101).double())[0]
    case("pca_axes", lambda v, a, m: ops.pca_axes_f64(v, 5, a, m), [vec, xp, mean64])
    case("pca_fit_transform", lambda a: PCA(8, sign_convention="u").fit_transform(a), [xp])

    # top-k, one case per scoring path
    lib = _lib.load()
    q9, d103 = _topk_data(9, 103, 64, 110)
    for metric in ("ip", "l2"):
        for norm in (True, False):
            case(f"topk_f32_{metric}_{'norm' if norm else 'raw'}",
                 (lambda m, n: lambda q, d: ops.topk(q, d, 12, m, normalize_db=n))(metric, norm), [q9, d103],
                 check=lambda tags: lib.anyloc_topk_path(9, 103, 64) == 0)
    case("topk_ndb0", lambda q, d: ops.topk(q, d, 12, "ip"), [q9, d103[:0].clone()])
    q5, d300 = _topk_data(5, 300, 4096, 120)
    for v in (1, 0):
        case(f"topk_fewq_qdma{v}", _with(lambda q, d: ops.topk(q, d, 7, "ip", normalize_db=True), topk_fewq_qdma=v), [q5, d300],
             tags=(["topk_combine"], []), check=lambda tags: lib.anyloc_topk_path(5, 300, 4096) == 1)
    q70, d256 = _topk_data(70, 300, 256, 130)

    def path_h3(tags):
        with ops.options(topk_h3=1):
            return lib.anyloc_topk_path(70, 300, 256) == 2
    case("topk_h3_forced", _with(lambda q, d: ops.topk(q, d, 5, "ip", normalize_db=True), topk_h3=1, topk_screen=0), [q70, d256],
         tags=(["topk_scores_gemm", "split_h2_wide"], ["topk_screen_gemm"]), check=path_h3)
    screened = _with(lambda q, d: ops.topk(q, d, 5, "ip", normalize_db=True), topk_h3=1, topk_screen=1)
    case("topk_screened", screened, [q70, d256], tags=(["topk_screen_gemm"], ["topk_scores_gemm"]))
    dup = _topk_data(70, 900, 256, 131)[1]
    dup[200:800] = (3.0 * q70[0]).expand(600, -1)         # > 512 candidates inside one query's bound: the unscreened re-run
    case("topk_screened_fallback", screened, [q70, dup], tags=(["topk_screen_gemm", "topk_scores_gemm"], []))
    panel = ops.topk_index_panel(256)
    big = _topk_data(70, panel + 300, 256, 132)[1]
    unscreened = dict(topk_h3=1, topk_screen=0)
    case("topk_index_build", _with(lambda q, d: ops.topk_indexed(q, ops.topk_index_build(d), d.shape[0], 5, normalize_db=True), **unscreened),
         [q70, d256], tags=(["split_h2_wide", "topk_scores_gemm"], ["topk_screen_gemm"]))

    def build_in_two(q, d):
        index = torch.empty(ops.topk_index_bytes(d.shape[0], 256), dtype=torch.uint8, device=d.device)
        ops.topk_index_build_range(index, d[panel:], panel, d.shape[0])
        ops.topk_index_build_range(index, d[:panel], 0, d.shape[0])
        return ops.topk_indexed(q, index, d.shape[0], 5, normalize_db=True)
    case("topk_index_build_range", _with(build_in_two, **unscreened), [q70, big])
    index = ops.topk_index_build(d256)
    case("topk_indexed_unscreened", _with(lambda q, i: ops.topk_indexed(q, i, 300, 5, normalize_db=True), **unscreened), [q70, index],
         tags=(["topk_scores_gemm"], ["topk_screen_gemm"]))
    case("topk_indexed_screened_rows", _with(lambda q, i, d: ops.topk_indexed(q, i, 300, 5, normalize_db=True, db=d), topk_h3=1, topk_screen=1),
         [q70, index, d256], tags=(["topk_screen_gemm", "topk_screen_rescore"], ["topk_scores_gemm"]))
    case("topk_indexed_screened_planes",
         _with(lambda q, i: ops.topk_indexed(q, i, 300, 5, normalize_db=True, rescore_planes=True), topk_h3=1, topk_screen=1),
         [q70, index], tags=(["topk_screen_gemm", "topk_screen_rescore_planes"], ["topk_scores_gemm"]))
    flat_index = retrieval.FlatIndex(d256, "cosine", True, planes=True)
    case("flatindex_search", lambda q: flat_index.search(q, 5), [q70])

    # ViT: forwards of finished models from a late image
    img, one = _images(2, 224, 224, 140), _images(1, 224, 224, 141)
    rag = [_images(1, 224, 224, 142)[0], _images(1, 126, 154, 143)[0]]
    for gemm_mode, opt in (("h3", {}), ("x6", X6), ("f32", {})):
        m, mr = _model(gemm_mode), _model(gemm_mode, VIT + "_reg")
        # which arithmetic ran shows in the LayerNorm that feeds the block GEMMs (they carry the same tags in every mode)
        arith = dict(h3=["layernorm_h2"], x6=["layernorm_x3"], f32=["layernorm"])[gemm_mode]
        other = [t for t in ("layernorm_h2", "layernorm_x3") if t not in arith]
        case(f"vit_fwd_{gemm_mode}_uniform", _fwd(m, False, **opt), [img], tags=(arith + ["vit_fc2_gemm", "attention"], other))
        case(f"vit_fwd_{gemm_mode}_ragged", _fwd_ragged(m, False, **opt), rag, tags=(arith + ["vit_fc2_gemm", "attention"], other))
        case(f"vit_fwd_{gemm_mode}_reg", _fwd(mr, False, **opt), [img], tags=(arith + ["vit_fc2_gemm", "attention"], other))
    h3 = _model("h3")
    # one ViT-B image: the fc2 GEMM splits K (test_one_image_forward_takes_a_split_k_plan), the forward zeroes its tickets with a
    # memset on its stream.  (anyloc_gemm_nt_h3 on its own has no workspace and never splits K.)
    case("vit_fwd_h3_vitb_split_k", _fwd(_model("h3", "dinov2_vitb14"), False), [one], tags=(["layernorm_h2", "vit_fc2_gemm"], []))
    case("vit_fwd_h3_uniform_ffn_check", _fwd(h3, True), [img], tags=(["layernorm_h2", "ffn_telemetry"], []))
    case("vit_fwd_h3_ragged_ffn_check", _fwd_ragged(h3, True), rag, tags=(["layernorm_h2", "ffn_telemetry"], []))

    # ViT: a model BUILT on the side stream from late weights, then one forward (the reference models of _model() stay alive)
    sd = _state_dict()
    keys = list(sd)
    built = _cache.setdefault("built", [])

    def build_and_forward(gemm_mode, opt):
        def run(*t):
            from anyloc_amd.extractor import HipDinoV2
            model = HipDinoV2(VIT, dict(zip(keys, t[:-1])), torch.device("cuda", torch.cuda.current_device()), gemm=gemm_mode)
            built.append(model)
            model.ffn_check = False
            return model.forward_taps(t[-1], TAPS)
        return _with(run, **opt)
    for gemm_mode, opt in (("h3", {}), ("x6", X6), ("f32", {})):
        case(f"vit_build_{gemm_mode}", build_and_forward(gemm_mode, opt), [sd[k] for k in keys] + [img])

    # anyloc_vit_attach_h2 itself, as a C caller reaches it: a FRESH handle (a re-attach frees the previous patch image first, and
    # hipFree waits for the device) whose patch weights arrive late on the side stream
    direct, create_args, h2_blocks = _model_with_h2_blocks()

    def attach_and_forward(patch_w):
        fresh = C.c_void_p()
        _lib.check(lib.anyloc_vit_create(C.byref(fresh), *create_args), "anyloc_vit_create")
        _lib.check(lib.anyloc_vit_attach_h2(fresh, h2_blocks), "anyloc_vit_attach_h2")
        old, direct._handle = direct._handle, fresh
        lib.anyloc_vit_destroy(old)
        direct.ffn_check = False
        return direct.forward_taps(img, TAPS)
    assert direct._keep[0].shape == (384, 3 * 14 * 14)           # the patch-embedding weights anyloc_vit_create was given
    case("vit_attach_h2_direct", attach_and_forward, [direct._keep[0]], in_place=True)

    # the reference's surface, CPU tensors in and out: the host-to-device and device-to-host legs of ops.to_device / to_host
    case("reference_surface", _reference_surface(), [_images(3, 224, 224, 150).cpu()])
    return c


def _model_with_h2_blocks():
    """An h3 model of its own, the arguments its construction gave anyloc_vit_create (after the handle) and the
    anyloc_vit_block_h2 array it handed to anyloc_vit_attach_h2."""
    from anyloc_amd import _lib
    from anyloc_amd.extractor import HipDinoV2
    lib = _lib.load()
    created, attached = [], []
    real_create, real_attach = lib.anyloc_vit_create, lib.anyloc_vit_attach_h2

    def spy_create(handle, *args):
        created.append(args)
        return real_create(handle, *args)

    def spy_attach(handle, blocks):
        attached.append(blocks)
        return real_attach(handle, blocks)
    lib.anyloc_vit_create, lib.anyloc_vit_attach_h2 = spy_create, spy_attach
    try:
        model = HipDinoV2(VIT, _state_dict(), torch.device("cuda", torch.cuda.current_device()), gemm="h3")
    finally:
        lib.anyloc_vit_create, lib.anyloc_vit_attach_h2 = real_create, real_attach
    torch.cuda.synchronize()
    assert len(created) == 1 and len(attached) == 1
    _cache["direct"] = (model, created[0], attached[0])
    return _cache["direct"]


def _reference_surface():
    from anyloc_amd import weights
    from anyloc_amd.extractor import DinoV2ExtractFeatures
    from anyloc_amd.kmeans import KMeans
    from anyloc_amd.retrieval import get_top_k_recall
    from anyloc_amd.vlad import VLAD
    weights.register_state_dict(VIT, {k: v.cpu() for k, v in _state_dict().items()})
    try:
        ext = DinoV2ExtractFeatures(VIT, 1, "value", device="cuda")
    finally:
        weights.unregister_state_dict(VIT)
    torch.cuda.synchronize()
    centers = 0.8 * _unit(8, 384, seed=151).cpu()
    vlad = VLAD(8, 384, cache_dir=None)
    vlad.c_centers = centers
    vlad.kmeans = KMeans(8, mode="cosine")
    vlad.kmeans.centroids = centers
    gt = np.empty(1, dtype=object)
    gt[0] = np.array([0])

    def run(imgs):
        toks = ext(imgs)
        v = vlad.generate_multi(toks)
        d, i, _ = get_top_k_recall([1, 2], v[:2], v[2:], gt)
        assert not toks.is_cuda and not v.is_cuda and not d.is_cuda
        return toks, v, d, i
    return run
