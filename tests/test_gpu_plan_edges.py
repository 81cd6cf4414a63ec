"""The fused two-term fp16 forward of all four DINOv2 sizes on either side of every row count at which the plan of one of its
GEMMs changes (csrc/gemm_h3s.hip: h3_plan), against the restated hub model on the CPU.  GPU box only.

The row counts come from tests/_plan_edges.py: M - 1 and M for every M of the model's edge list (derived from the library and
pinned by tests/test_h3_plan_cpu.py), the counts that fill every 64- / 128- / 192-row tile exactly and those that leave ONE
live row in the last tile of all three heights (k * 384 and k * 384 + 1), and the ln_direct_rows boundary of the LayerNorm.
A row count is reached with two images of different sizes in one ragged call; those with M - 1 = gh x gw also run as one
image through the uniform forward.  Every case first asks ``anyloc_h3_plan_describe`` whether it sits where it claims to.

First launches in any test (ViT-B/14 never ran on a GPU before; ViT-L/14 only at M >= 2740 and T = 36) -- (tile / ring depth,
split-K, epilogue):
  * fc1, EPI_GELU_H2: 128 x 128 / 6-deep (M <= 600), 64 x 128 four-wave / 3-deep (601 ... 1100), 64 x 64 two-wave / 3-deep
    (ViT-B, 1101 ... 1280), 128 x 128 / 3-deep above (ViT-L from 1101);
  * qkv, EPI_QKV_PLANES with 12 / 16 heads: 128 x 128 / 6-deep (M <= 600), 64 x 128 four-wave / 3-deep (601 ... 1100), 64 x 64
    two-wave / 3-deep (ViT-L 1101 ... 1280, ViT-B 1101 ... 1792), 128 x 128 / 3-deep above;
  * fc2, EPI_LS_RESID: 64 x 128 four-wave / 6-deep with the table's own split-K 2 (M <= 600) at K16 = 192 (ViT-B, exactly on the
    K16 >= 192 threshold: two ranges of 96 k-blocks) and K16 = 256 (ViT-L); unsplit 601 ... 1100; split-K 2 / 3-deep 1101 ... 1700;
    64 x 64 two-wave with two k-blocks per ring stage above;
  * proj, EPI_LS_RESID with N = 768 / 1024: 64 x 64 / 6-deep (M <= 600), 64 x 128 four-wave / 6-deep (601 ... 1700), 64 x 64
    two-wave with two k-blocks per ring stage above.
ViT-g adds the 192 x 128 w12 plan away from M = 530 (385 and 600, its two ends) and the tiny-GEMM rules below 385 rows
(M = 128 / 129 / 192 / 193: four, two and one k-block per ring stage on 64 x 64 tiles under EPI_SWIGLU_T_H2).
"""
import pytest
import torch
import torch.nn.functional as F

import _plan_edges as pe
from anyloc_amd import synth
from oracle import dinov2_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOKEN_ATOL = 2e-5        # unit-norm token rows against the oracle: the bar of test_gpu_vit / test_gpu_long_sequences / test_gpu_ragged
KORDER_ATOL = 2e-6       # another summation order over k: the bar of test_small_m_plans_agree_with_the_plain_kernels
TAPS = [(1, "token"), (1, "value")]
SEEDS = {"dinov2_vits14": 41, "dinov2_vitb14": 42, "dinov2_vitl14": 43, "dinov2_vitg14": 44}


class _Model:
    """One architecture with 2 synthetic blocks: the restated hub model, the HIP model per arithmetic, and the oracle's rows
    per list of image sizes (run once, one image per call, shared by every variant of a case)."""

    def __init__(self, name):
        self.name = name
        self.dim = synth.ARCH[name][0]
        self.sd = synth.synthetic_state_dict(name, SEEDS[name], depth=2)
        m = dinov2_ref.DinoVisionTransformer(name)
        m.blocks = m.blocks[:2]
        m.load_state_dict(self.sd, strict=True)
        self.ref_model = m.eval()
        self._hip, self._ref = {}, {}

    def hip(self, mode="h3"):
        from anyloc_amd.extractor import HipDinoV2
        if mode not in self._hip:
            self._hip[mode] = HipDinoV2(self.name, {k: v.to(DEV) for k, v in self.sd.items()}, torch.device(DEV), gemm=mode)
        return self._hip[mode]

    def _oracle_rows(self, img):
        """block-1 output and the v third of block 1's qkv, CLS dropped, each normalised: [N, 2 D] of one image"""
        grabbed = {}
        blk = self.ref_model.blocks[1]
        hooks = [blk.register_forward_hook(lambda m, i, o: grabbed.__setitem__("token", o)),
                 blk.attn.qkv.register_forward_hook(lambda m, i, o: grabbed.__setitem__("qkv", o))]
        try:
            with torch.no_grad():
                self.ref_model(img[None])
        finally:
            for h in hooks:
                h.remove()
        tok = grabbed["token"][0, 1:]
        val = grabbed["qkv"][0, 1:, 2 * self.dim:]
        return torch.cat([F.normalize(tok, dim=-1), F.normalize(val, dim=-1)], dim=-1)

    def case(self, sizes):
        """-> (images, oracle rows of all images [sum N_i, 2 D]); image-like input: smooth structure + noise"""
        key = tuple(sizes)
        if key not in self._ref:
            g = torch.Generator().manual_seed(sum(h * 7 + w for h, w in sizes))
            imgs = []
            for h, w in sizes:
                x = torch.randn(1, 3, h // 14, w // 14, generator=g)
                x = F.interpolate(x, size=(h, w), mode="bilinear", align_corners=False) + 0.3 * torch.randn(1, 3, h, w, generator=g)
                imgs.append(x[0])
            self._ref[key] = (imgs, torch.cat([self._oracle_rows(x) for x in imgs]))
        return self._ref[key]


@pytest.fixture(scope="module")
def zoo():
    models = {}

    def get(name):
        if name not in models:
            models[name] = _Model(name)
        return models[name]
    yield get
    models.clear()


@pytest.fixture(scope="module")
def lib():
    from anyloc_amd import _lib
    return _lib.load()


def _claims(lib, name, M):
    """What the case claims to hit, asked of the library under the options in force: on an edge the plans of M - 1 and M
    differ; at k * 384 + 1 the last row tile of every block GEMM holds one live row.  -> the plans at M."""
    plans = pe.block_plans(lib, name, M)
    for lo in (M - 1, M):
        if lo + 1 in pe.EDGES[name]:
            a, b = pe.block_plans(lib, name, lo), pe.block_plans(lib, name, lo + 1)
            assert any(pe.decision(a[k]) != pe.decision(b[k]) for k in pe.BLOCK), (name, lo + 1, "no plan changes here", a, b)
    if M in pe.ONE_LIVE_ROW:
        for k, p in plans.items():
            assert p["tile_rows"] in (64, 128, 192) and M - (p["tiles_m"] - 1) * p["tile_rows"] == 1, (name, M, k, p)
    if M in pe.TILE_FILL and M not in pe.ONE_LIVE_ROW:
        for k, p in plans.items():
            assert M == p["tiles_m"] * p["tile_rows"], (name, M, k, p)
    return plans


def _check_tokens(got, ref, what):
    """output shape, all finite, unit rows per tap, the oracle bar -> the max abs error"""
    got = got.cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    D = ref.shape[1] // 2
    for tap in (got[:, :D], got[:, D:]):
        assert float((tap.norm(dim=-1) - 1).abs().max()) < 1e-5, what
    err = float((got - ref).abs().max())
    print(f"[{what}] oracle err {err:.2e}")
    assert err <= TOKEN_ATOL, (what, err)
    return err


def _edge_case(lib, zoo, name, M, sizes, run):
    """assertions 1 - 5 of one (model, row count): ``run(model, images)`` -> [rows, 2 D] on the GPU"""
    from anyloc_amd import ops
    plans = _claims(lib, name, M)
    case = zoo(name)
    m = case.hip("h3")
    imgs, ref = case.case(sizes)
    x = [im.to(DEV) for im in imgs]
    got = run(m, x).clone()
    err = _check_tokens(got, ref, (name, M, sizes))
    assert torch.equal(run(m, x), got), (name, M, "two calls differ")              # split-K reduces in split order
    with ops.options(h3s_enable=0):
        plain = run(m, x).clone()
    diff = float((got - plain).abs().max())
    print(f"[{name} M={M} {sizes}] oracle err {err:.2e}, default vs h3s_enable=0 {diff:.2e}; "
          + ", ".join(f"{k} {p['tile_rows']}x{p['tile_cols']}/kb{p['kb']}/st{p['stages']}/ks{p['ksplit']}" for k, p in plans.items()))
    assert diff <= KORDER_ATOL, (name, M, diff)
    # the FFN ran fused (fc1 on its quantising epilogue, fc2 on the image it left): no block fell back to the exact quantiser
    assert m.ffn_exact_blocks == set() and m.ffn_reruns == 0, (name, M, m.ffn_exact_blocks)


def _ragged(m, x):
    return m.forward_taps_ragged(x, TAPS)[0]


def _uniform(m, x):
    assert len(x) == 1
    return m.forward_taps(x[0][None], TAPS)[0]


@pytest.mark.parametrize("name,M", [(n, M) for n in pe.MODELS for M in pe.row_counts(n)])
def test_forward_on_both_sides_of_every_plan_edge(lib, zoo, name, M):
    """Two images of different sizes with M token rows in one ragged call, 2 blocks, ``token`` and ``value`` of layer 1 (block 0
    runs fully fused: LN1 + qkv -> attention -> proj, LN2 + fc1 / w12 -> fc2; block 1 keeps fp32 q | k | v for the tap and runs its
    FFN fused): <= 2e-5 of the oracle run one image per call, <= 2e-6 of the round-3 kernels (option h3s_enable = 0: code
    against code, a second assertion), the same bits twice."""
    sizes = pe.image_sizes(M)
    assert pe.rows_of(sizes) == M
    _edge_case(lib, zoo, name, M, sizes, _ragged)


@pytest.mark.parametrize("name,M", [(n, M) for n in pe.MODELS for M in sorted(pe.ONE_IMAGE)])
def test_one_image_forward_at_the_edges(lib, zoo, name, M):
    """The row counts that are one near-square image (385 = 1 + 16 x 24 ... 1701 = 1 + 34 x 50) through the uniform forward --
    the reference's calling convention, the shape the plan table was measured for."""
    gh, gw = pe.ONE_IMAGE[M]
    _edge_case(lib, zoo, name, M, [(14 * gh, 14 * gw)], _uniform)


# ViT-g: the w12 launch carries LN2 while its 192 x 128 plan has at most 200 tiles (LN_LEAD_MAX_TILES, csrc/gemm_h3s.hip: a CU is
# left for every lead workgroup) -- three row tiles x 64 = 192 up to M = 576; from 577 rows on there are four x 64 = 256 and the
# LayerNorm stays a launch of its own.  Both sides of that edge run next to the listed row counts.
W12_LEAD_LAST = 576
LEAD_ROWS = [(n, M) for n in pe.MODELS[1:] for M in pe.row_counts(n) if M <= 600] + \
    [("dinov2_vitg14", W12_LEAD_LAST), ("dinov2_vitg14", W12_LEAD_LAST + 1)]


@pytest.mark.parametrize("name,M", LEAD_ROWS)
def test_layernorm_lead_role_at_the_edges(lib, zoo, name, M):
    """Option h3s_ln_lead = 1 at every listed row count of one image's range: LN1 travels with the qkv launch (ViT-g at 385 ...
    576 rows: LN2 with the w12 launch too; 577 ... 600: 256 tiles, more than the lead role allows), and the tokens are bit for
    bit those of the separate LayerNorm launches (the contract of
    test_layernorm_lead_role_gives_the_bits_of_the_separate_launch), on the GELU models and ragged batches as well."""
    from anyloc_amd import ops
    case = zoo(name)
    m = case.hip("h3")
    imgs, ref = case.case(pe.image_sizes(M))
    x = [im.to(DEV) for im in imgs]
    with ops.options(h3s_ln_lead=0):
        assert all(p["lead"] == 0 for p in pe.block_plans(lib, name, M).values())
        want = _ragged(m, x).clone()
    _check_tokens(want, ref, (name, M))
    with ops.options(h3s_ln_lead=1):
        plans = pe.block_plans(lib, name, M)
        assert plans["qkv"]["lead"] == 1, (name, M, plans["qkv"])
        if name == "dinov2_vitg14" and 385 <= M <= 600:
            w12 = plans["fc1"]
            assert (w12["tile_rows"], w12["tile_cols"]) == (192, 128), (M, w12)
            assert w12["lead"] == (1 if M <= W12_LEAD_LAST else 0), (M, w12)
            assert (w12["tiles_m"] * w12["tiles_n"] <= 200) == (M <= W12_LEAD_LAST), (M, w12)
        got = _ragged(m, x)
        assert torch.equal(got, want), (name, M, float((got - want).abs().max()))


@pytest.mark.parametrize("mode", ["x6", "f32"])
@pytest.mark.parametrize("name", ["dinov2_vitb14", "dinov2_vitl14"])
def test_vitb_vitl_one_image_in_the_other_arithmetics(zoo, name, mode):
    """ViT-B/14 and ViT-L/14 at the reference scripts' one 322 x 322 image (530 rows) on the split-bf16 kernels (option
    x6_min_rows = 0: below 1600 rows an x6 model would run the fp32-MFMA kernels) and on the fp32-MFMA kernels."""
    from anyloc_amd import ops
    case = zoo(name)
    imgs, ref = case.case([(322, 322)])
    with ops.options(x6_min_rows=0):
        got = case.hip(mode).forward_taps(imgs[0][None].to(DEV), TAPS)[0]
    _check_tokens(got, ref, (name, mode, "322x322"))


GEMM_M = (384, 385, 600, 601, 1100, 1101, 1700, 1701)
GEMM_NK = ((2048, 256), (2049, 256), (8191, 64), (8192, 64), (768, 3072), (768, 3056))


@pytest.fixture(scope="module")
def gemm_weights():
    """w, bias per (N, K), built as test_gemm_h3_random_shapes builds them, with the float64 copies the reference needs"""
    cache = {}

    def get(N, K):
        if (N, K) not in cache:
            g = torch.Generator().manual_seed(N * 7 + K)
            w = torch.randn(N, K, generator=g) * 0.05 * (0.1 + torch.rand(N, 1, generator=g))
            bias = torch.randn(N, generator=g)
            cache[(N, K)] = (w, bias)
        return cache[(N, K)]
    yield get
    cache.clear()


@pytest.mark.parametrize("M", GEMM_M)
@pytest.mark.parametrize("N,K", GEMM_NK)
def test_public_gemm_on_both_sides_of_the_width_thresholds(gemm_weights, N, K, M):
    """``anyloc_gemm_nt_h3`` (plain store, no split-K workspace) on either side of every row threshold of the plan table and of
    its width thresholds -- N <= 2048 (2048 / 2049), N < 8192 (8191 / 8192), K16 >= 192 (K = 3072 / 3056: K16 = 192 / 191) --
    which the random shapes of test_gemm_h3_random_shapes (k16 <= 130, n <= 2600) never reach; rows of very different magnitude;
    against float64 at that test's bar, 6e-7 of sum |a| |w| + |bias| elementwise."""
    from anyloc_amd import ops
    w, bias = gemm_weights(N, K)
    g = torch.Generator().manual_seed(M * 31 + N + K)
    a = torch.randn(M, K, generator=g) * torch.pow(10.0, torch.randint(-3, 4, (M, 1), generator=g).float())
    c = ops.gemm_nt_h3(ops.split_h2(a.to(DEV)), ops.split_h2(w.to(DEV)), M, N, K, bias.to(DEV)).cpu()
    assert c.shape == (M, N) and bool(torch.isfinite(c).all())
    ref = a.double() @ w.double().t() + bias.double()
    mag = a.double().abs() @ w.double().abs().t() + bias.double().abs()
    rel = float(((c.double() - ref).abs() / mag).max())
    print(f"[gemm_nt_h3 {M} x {N} x {K}] err / (|a| |w|^T + |bias|) {rel:.2e}")
    assert rel <= 6e-7, (M, N, K, rel)
