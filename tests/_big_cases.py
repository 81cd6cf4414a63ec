"""The case table of the addressing-limit tests, shared by tests/test_addressing_limits_cpu.py (which checks, without a GPU,
what the GPU module relies on) and tests/test_gpu_addressing.py (which runs the cases).

Inputs are a closed formula of (row, column): an integer hash mapped onto a small set of exactly representable floats,
evaluated with int64 tensors -- on the device in slabs for the whole tensor, on the CPU for any row alone.  Nothing of a
multi-GiB tensor ever has to travel to the host to get its float64 reference.

Token inputs (k-means, VLAD) lie on the lattice of multiples of 1 / 32 with |x| <= 1: a row is one of 32 base directions
(entries in [-0.75, 0.75)) plus noise in [-0.25, 0.25).  Every per-cluster sum of fewer than 2^18 such rows is EXACT in fp32
in any order (|sum| * 32 <= 2^23), so the bars of the families' tests, written for images of ~1 000 tokens, hold for 10^6
rows without being widened for fp32 growth; and a row's own direction beats every other by a margin of > 0.1 in both metrics (checked
in the CPU module), so no label sits on a near-tie and none needs excusing."""
import torch

B31, B32 = 1 << 31, 1 << 32
MODES = 32                     # base directions of the token inputs = clusters of the k-means / VLAD cases


def _i64(u):
    u &= (1 << 64) - 1
    return u - (1 << 64) if u >= (1 << 63) else u


_A, _B, _C = _i64(0x9E3779B97F4A7C15), _i64(0xBF58476D1CE4E5B9), _i64(0x94D049BB133111EB)


def hash_bits(rows, cols, seed):
    """int64 [R], int64 [C] -> int64 [R, C] of well-mixed bits (wrapping int64 arithmetic: the same on the CPU and the device)"""
    h = rows[:, None] * _A + cols[None, :] * _B + _i64(seed * 0x94D049BB133111EB + 0x2545F4914F6CDD1D)
    h = (h ^ (h >> 31)) * _B
    h = (h ^ (h >> 29)) * _C
    return h ^ (h >> 32)


def unit(rows, cols, seed):
    """float64 [R, C] in [-1, 1), multiples of 2^-23: exact in fp32"""
    return (hash_bits(rows, cols, seed) & 0xFFFFFF).double() / float(1 << 23) - 1.0


def positive(rows, cols, seed):
    """float64 in [0.5, 1): pooling inputs (no cancellation in mean(t^p), no negative base for a fractional power)"""
    return 0.75 + 0.25 * unit(rows, cols, seed)


def mode_of(rows):
    """the base direction of a token row"""
    return ((rows * 2654435761) >> 7) % MODES


def base_directions(D, seed, device="cpu"):
    """float64 [MODES, D], multiples of 1 / 32 in [-0.75, 0.75)"""
    h = hash_bits(torch.arange(MODES, device=device), torch.arange(D, device=device), seed + 1000)
    return ((h & 0xFFFFFF) % 48 - 24).double() / 32.0


def tokens(rows, cols, seed):
    """float64 [R, C]: base direction of the row + noise, multiples of 1 / 32 with |x| <= 1"""
    base = base_directions(int(cols.numel()), seed, rows.device)       # (cols is always the full arange(D) here)
    noise = ((hash_bits(rows, cols, seed) >> 24) % 16 - 8).double() / 32.0
    return base[mode_of(rows)][:, cols] + noise


def scaled(rows, cols, seed):
    """float64: unit values times 2^(row % 13 - 6) -- rows of very different magnitude (the splits scale per row), exact in fp32"""
    return unit(rows, cols, seed) * torch.pow(2.0, (rows % 13 - 6).double())[:, None]


def byte_values(rows, cols, seed):
    """float64 integers in [0, 255]: uint8 pixels"""
    return (hash_bits(rows, cols, seed) & 0xFF).double()


GENERATORS = {"unit": unit, "positive": positive, "tokens": tokens, "scaled": scaled, "bytes": byte_values}


def fill(rows, cols, gen, seed, device, scale=1.0, slab_elems=1 << 25, dtype=torch.float32):
    """the whole [rows, cols] tensor (fp32; uint8 for pixels) on ``device``, generated in slabs of about ``slab_elems`` elements"""
    out = torch.empty(rows, cols, dtype=dtype, device=device)
    c = torch.arange(cols, device=device)
    step = max(1, slab_elems // cols)
    for r0 in range(0, rows, step):
        r = torch.arange(r0, min(rows, r0 + step), device=device)
        out[r0:r0 + r.numel()] = (GENERATORS[gen](r, c, seed) * scale).to(dtype)
    return out


def rows_f64(row_idx, cols, gen, seed, scale=1.0):
    """the same values for the rows ``row_idx`` alone, on the CPU: float64 of the fp32 the device holds"""
    r = torch.as_tensor(row_idx, dtype=torch.int64)
    return (GENERATORS[gen](r, torch.arange(cols), seed) * scale).float().double()


# ---- boundaries and samples ------------------------------------------------------------------------------------------
def crossings(rows, stride_elems, elem_bytes):
    """{"2^31 B" | "2^32 B" | "2^31 el": the row that holds that flat byte offset / element index} of a [rows, stride] operand"""
    out = {}
    for name, flat in (("2^31 B", B31 // elem_bytes), ("2^32 B", B32 // elem_bytes), ("2^31 el", B31)):
        if flat < rows * stride_elems:
            out[name] = flat // stride_elems
    return out


def sample_rows(rows, boundary_rows, seed):
    """first and last 64 rows, 64 rows around every boundary row, 256 seeded random rows -> sorted unique list"""
    s = set(range(min(64, rows))) | set(range(max(0, rows - 64), rows))
    for b in boundary_rows:
        s |= set(range(max(0, b - 32), min(rows, b + 32)))
    g = torch.Generator().manual_seed(seed)
    s |= set(torch.randint(0, rows, (256,), generator=g).tolist())
    return sorted(s)


GIB = 1 << 30

# name -> rows (the index every operand shares), operands (name, row stride in elements, bytes per element), the crossings
# the case claims (operand -> names), the generator of its input, and the device bytes the test holds at once (inputs,
# outputs, workspace and the float64 slabs of its reference, rounded up)
CASES = {
    # anyloc_l2norm_rows / anyloc_layernorm / anyloc_pool_tokens: rows x 4092 floats, 16 368 bytes a row (no boundary on a row edge)
    "rows_4g": dict(rows=262500, cols=4092, gen="unit", seed=11, operands=[("x", 4092, 4), ("out", 4092, 4)],
                    crosses={"x": ["2^31 B", "2^32 B"], "out": ["2^31 B", "2^32 B"]}, device_bytes=12 * GIB),
    "pool_4g": dict(rows=262500, cols=4092, gen="positive", seed=12, operands=[("tokens", 4092, 4)],
                    crosses={"tokens": ["2^31 B", "2^32 B"]}, device_bytes=8 * GIB, n_tok=1369),
    # anyloc_kmeans_step / anyloc_vlad_hard at D = 384: one chunk / one image just past 2 GiB (1 398 102 rows)
    "tokens_2g": dict(rows=1398400, cols=384, gen="tokens", seed=13, operands=[("x", 384, 4), ("labels", 1, 8)],
                      crosses={"x": ["2^31 B"]}, device_bytes=8 * GIB),
    # the same past 2^31 ELEMENTS (8 GiB), default chunking; as a VLAD batch: 4085 images of 1369 tokens and one of 135
    "tokens_8g": dict(rows=5592500, cols=384, gen="tokens", seed=14, operands=[("x", 384, 4), ("labels", 1, 8)],
                      crosses={"x": ["2^31 B", "2^32 B", "2^31 el"]}, device_bytes=16 * GIB, n_tok=1369),
    # anyloc_gemm_nt: C [M, 1024] past 2^31 elements from K = 4; A [M, 1024] past 2^31 elements into 64 columns
    "gemm_c_8g": dict(rows=2097400, cols=4, gen="unit", seed=15, operands=[("A", 4, 4), ("C", 1024, 4)],
                      crosses={"C": ["2^31 B", "2^32 B", "2^31 el"]}, device_bytes=12 * GIB, N=1024),
    "gemm_a_8g": dict(rows=2097400, cols=1024, gen="unit", seed=16, operands=[("A", 1024, 4), ("C", 64, 4)],
                      crosses={"A": ["2^31 B", "2^32 B", "2^31 el"]}, device_bytes=10 * GIB, N=64),
    # anyloc_attention: 65 535 images of 171 tokens, one head -- qkv [rows, 192] past 2^31 elements, out [rows, 64] past 2^31 bytes
    # (attention inputs: uniform in [-2.6, 2.6), the standard deviation 1.5 of the family's own test, whose absolute bar was
    # set for logits of that size)
    "attn_8g": dict(rows=65535 * 171, cols=192, gen="unit", seed=17, scale=2.6, operands=[("qkv", 192, 4), ("out", 64, 4)],
                    crosses={"qkv": ["2^31 B", "2^32 B", "2^31 el"], "out": ["2^31 B"]}, device_bytes=14 * GIB, n_tok=171),
    # anyloc_attention: ONE image whose qkv rows end 32 768 bytes below 2 GiB (the next token count is refused)
    "attn_one_image": dict(rows=21845, cols=3 * 8192, gen="unit", seed=18, scale=2.6, operands=[("qkv", 3 * 8192, 4), ("out", 8192, 4)],
                           crosses={}, device_bytes=12 * GIB, heads=128),
    # anyloc_attention_h3: the most rows its q | k | v tile images hold (65 535 images of 128 tokens, one head: 262 140 groups of
    # 32 rows, 4 short of 2 GiB per image); qkv crosses 2^31 and 2^32 bytes
    "attn_h3_6g": dict(rows=65535 * 128, cols=192, gen="unit", seed=19, scale=2.6, operands=[("qkv", 192, 4), ("out", 64, 4)],
                       crosses={"qkv": ["2^31 B", "2^32 B"]}, device_bytes=20 * GIB, n_tok=128),
    # anyloc_preprocess_u8: 2731 images of 520 x 520 pixels, cropped to 518 x 518 -- the output (rows of 518 floats) past 2^31
    # elements, the uint8 input (rows of 1560 bytes, generated as [B * 520, 1560]) past 2^31 bytes
    "ingest_8g": dict(rows=2731 * 3 * 518, cols=518, gen="bytes", seed=23, operands=[("out", 518, 4)],
                      crosses={"out": ["2^31 B", "2^32 B", "2^31 el"]}, device_bytes=16 * GIB, batch=2731, hw=520, crop=518),
    # anyloc_resize_bicubic: 8300 planes of 64 x 64 upscaled to 512 x 508 -- the output (rows of 508 floats) past 2^31 elements
    "resize_8g": dict(rows=8300 * 512, cols=508, gen="unit", seed=24, operands=[("out", 508, 4)],
                      crosses={"out": ["2^31 B", "2^32 B", "2^31 el"]}, device_bytes=12 * GIB, planes=8300, hw=64, out_hw=(512, 508)),
    # anyloc_gemm_nt: the strided views of test_gemm_nt_widest_row_stride_*: 2 GiB between a tile's first and last row
    # (a VIEW of at most 256 rows, not a dense operand: no row of it is sampled, every row is compared)
    "gemm_view_2g": dict(rows=256, cols=64, gen="unit", seed=60, operands=[], crosses={}, device_bytes=4 * GIB),
    # anyloc_gemm_nt_h3 / _x6: the largest A image below 2 GiB at K = 1024 (4 and 6 bytes per element), and C past 2^31 elements
    "gemm_h3_image": dict(rows=524287, cols=1024, gen="scaled", seed=25, operands=[("A", 1024, 4), ("C", 64, 4)], crosses={},
                          device_bytes=8 * GIB, N=64),
    "gemm_x6_image": dict(rows=349525, cols=1024, gen="scaled", seed=26, operands=[("A", 1024, 4), ("C", 64, 4)], crosses={},
                          device_bytes=8 * GIB, N=64),
    "gemm_planes_c_8g": dict(rows=2097400, cols=64, gen="scaled", seed=27, operands=[("A", 64, 4), ("C", 1024, 4)],
                             crosses={"C": ["2^31 B", "2^32 B", "2^31 el"]}, device_bytes=12 * GIB, N=1024),
    # anyloc_pca_gram_f64 / _axes_f64: X [2056, 1 048 700] fp32 past 2^31 elements, and the same memory as [1 048 700, 2056]
    "pca_8g": dict(rows=2056, cols=1048700, gen="unit", seed=28, operands=[("X", 1048700, 4)],
                   crosses={"X": ["2^31 B", "2^32 B", "2^31 el"]}, device_bytes=14 * GIB),
    # anyloc_gemm_nt_f64: A [2056, 1 048 700] float64 past 2^31 elements (16 GiB), row-major and as the transpose of a view
    "f64_16g": dict(rows=2056, cols=1048700, gen="unit", seed=29, operands=[("A", 1048700, 8)],
                    crosses={"A": ["2^31 B", "2^32 B", "2^31 el"]}, device_bytes=24 * GIB),
    # anyloc_vlad_residuals: out [n, 32 * 384] past 2^31 elements
    "resid_8g": dict(rows=174800, cols=384, gen="tokens", seed=20, operands=[("x", 384, 4), ("out", 32 * 384, 4)],
                     crosses={"out": ["2^31 B", "2^32 B", "2^31 el"]}, device_bytes=10 * GIB),
    # anyloc_split_h2 / anyloc_split_x3: rows x 4096 past 2^31 elements (the plane images: 8 and 12 GiB)
    "split_8g": dict(rows=524400, cols=4096, gen="scaled", seed=21, operands=[("x", 4096, 4)],
                     crosses={"x": ["2^31 B", "2^32 B", "2^31 el"]}, device_bytes=24 * GIB),
    # anyloc_topk: a database of 262 400 rows x 4096 columns, past 2^32 bytes; rows 131 072 and 262 144 start exactly on 2^31 and
    # 2^32 bytes -- the best rows are planted there, just behind, and at both ends
    "topk_4g": dict(rows=262400, cols=4096, gen="unit", seed=22, scale=0.001, operands=[("db", 4096, 4)],
                    crosses={"db": ["2^31 B", "2^32 B"]}, device_bytes=12 * GIB, planted=[0, 131071, 131072, 131073, 262144, 262145, 262399]),
}


def case_boundary_rows(case):
    c = CASES[case]
    rows = set()
    for name, stride, eb in c["operands"]:
        rows |= set(crossings(c["rows"], stride, eb).values())
    return sorted(rows)


def case_sample(case):
    c = CASES[case]
    return sample_rows(c["rows"], case_boundary_rows(case), c["seed"])


def case_fill(case, device):
    c = CASES[case]
    return fill(c["rows"], c["cols"], c["gen"], c["seed"], device, c.get("scale", 1.0))


def case_rows_f64(case, row_idx):
    c = CASES[case]
    return rows_f64(row_idx, c["cols"], c["gen"], c["seed"], c.get("scale", 1.0))


def token_centers(D, seed):
    """the k-means / VLAD centres of a token case: its 32 base directions (fp32-exact) -> float32 [32, D]"""
    return base_directions(D, seed).float()


# ---- restated limits (include/anyloc_hip.h) --------------------------------------------------------------------------
def gemm_tile_span_ok(tile_rows, rows, ld, K):
    """anyloc_gemm_nt: (min(tile rows, rows) - 1) * ld * 4 + K * 4 < 2^31"""
    return (min(tile_rows, rows) - 1) * ld * 4 + K * 4 < B31


def gemm_last_ld(tile_rows, K):
    """the largest leading dimension (a multiple of 4) a full tile of ``tile_rows`` rows is served with"""
    return (B31 - 1 - K * 4) // (4 * (tile_rows - 1)) // 4 * 4


def attention_image_ok(tokens, dim):
    """anyloc_attention: tokens * 3 * dim * 4 < 2^31 per image"""
    return tokens * 3 * dim * 4 < B31


def fused_unit_rows(D):
    """k-means chunks and one-pass VLAD parts: fewer than 2^31 bytes of rows, whole 16-row tiles"""
    return (B31 - 1) // (4 * D) // 16 * 16


def vlad_rows_per_part(rows, parts):
    return -(-(-(-rows // 16)) // parts) * 16


def kmeans_chunks(n, D, max_chunks):
    """chunks of one anyloc_kmeans_step: max_chunks (>= 1024 rows each), more where a chunk would reach 2 GiB"""
    rows = max(1024, -(-n // max_chunks))
    rows = min(rows, fused_unit_rows(D))
    return -(-n // rows)


def attention_h3_rows_ok(rows, heads):
    """anyloc_attention_h3: heads * ceil(rows / 32) * 8192 < 2^31"""
    return heads * (-(-rows // 32)) * 8192 < B31
