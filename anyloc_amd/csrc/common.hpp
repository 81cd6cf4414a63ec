// Shared host/device helpers for libanyloc_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <type_traits>

#include "../../include/anyloc_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace anyloc {

// ---- error reporting (thread-local, never throws across the ABI) ----------
void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);

#define ANYLOC_CHECK_ARG(cond, ...)            \
  do {                                         \
    if (!(cond)) {                             \
      ::anyloc::set_error(__VA_ARGS__);        \
      return ANYLOC_ERR_INVALID_ARG;           \
    }                                          \
  } while (0)

#define ANYLOC_HIP(call)                                   \
  do {                                                     \
    hipError_t e__ = (call);                               \
    if (e__ != hipSuccess) return ::anyloc::hip_fail(e__, #call); \
  } while (0)

#define ANYLOC_TRY(call)        \
  do {                          \
    int s__ = (call);           \
    if (s__ != ANYLOC_OK) return s__; \
  } while (0)

// ---- per-kernel profiling with HIP events on the launch stream ------------
// A Scope brackets one kernel launch; when profiling is off it costs one branch.
struct ProfScope {
  int slot;
  hipStream_t stream;
  ProfScope(const char* name, hipStream_t s, double flops, double bytes);
  ~ProfScope();
};

bool profiling_enabled();

// ---- tuning options (anyloc_set_option / anyloc_get_option; include/anyloc_hip.h lists the names) ------------------
// Process-wide integers; never read from the environment on a call path: the one environment variable,
// ANYLOC_OPTIONS="name=value,...", is parsed once when the first option is looked up.
// Who reads what: an option is read by ONE plan function -- a function that decides how a call runs before its first HIP call --
// and by no template and no function that launches:
//   gemm_f32_plan (gemm_f32.hip)               gemm_f32_cfg
//   x6_plan (gemm_x6.hip)                      x6_cfg
//   h3_plan and its helpers (gemm_h3s.hip)     h3_cfg, h3_group_m (h3_group_m(): also gemm_screen's), h3_tiny_max, h3_deep_max, h3_deep2_max,
//                                              h3_epi_lds, h3_fast_silu, h3_mfma16, h3s_*, h3s_ln_lead, h3_ln_lead
//   ln_h2_plan (gemm_h3.hip)                   ln_rows_per_wave, ln_small_rows, ln_waves, ln_direct_rows
//   attn_f32_plan / attn_plan (attention.hip)  attn_cfg, attn_x6 / attn_h3_qg, attn_h3_ks, attn_h3_ragged_xcd
//   fused_plan (vlad_fused.hip)                vlad_fused_v, kmeans_fused_v, vlad_gather_v
//   the plan helpers of vlad.hip               vlad_parts, vlad_two_pass, kmeans_max_chunks
//   topk_plan (topk.hip)                       topk_h3, topk_screen, topk_rescore_cols, topk_fewq_x6, topk_fewq_qdma
//   vit_forward_launches' decision block       h3_fuse, x6_fuse, h3_min_rows, x6_min_rows, h3_patch
//   (h3_swiglu_t is read by the Python host when it builds the weight images)
enum Option {
  OPT_GEMM_F32_CFG,      // gemm_f32.hip tile configuration (micro-benchmarks); 0 = default
  OPT_X6_CFG,            // gemm_x6.hip tile configuration; 0 = default
  OPT_H3_CFG,            // gemm_h3.hip tile configuration; 0 = default (128x256, 3-deep ring)
  OPT_H3_GROUP_M,        // gemm_h3: tile rows per XCD scheduling group
  OPT_H3_TINY_MAX,       // gemm_h3: below this many 128x128 tiles run 64x64 two-wave tiles
  OPT_H3_DEEP_MAX,       // ... and below this many 64x64 tiles a ring stage holds four k-blocks
  OPT_H3_DEEP2_MAX,      // ... below this many, two
  OPT_H3_EPI_LDS,        // gemm_h3 LayerScale-residual epilogue: 1 = 16-byte accesses through LDS, 0 = dword read-modify-write
  OPT_LN_ROWS_PER_WAVE,  // layernorm_h2: 0 = by ln_small_rows; 1 / 2 / 4 = rows per wave at every size (A/B)
  OPT_LN_SMALL_ROWS,     // layernorm_h2: below this many rows one row per wave
  OPT_LN_WAVES,          // layernorm_h2 with two rows per wave: waves per block, 8 (16 rows: 512-byte store runs) or 4
  OPT_LN_DIRECT_ROWS,    // layernorm_h2: below this many rows one single-wave workgroup per row, no LDS tile (0 = never)
  OPT_H3_FUSE,           // h3 forward: 1 = q|k|v, attention output and FFN activation stay in fp16 planes; 0 = fp32 + quantiser passes
  OPT_X6_FUSE,           // x6 forward: the same for the bf16 plane images
  OPT_H3_MIN_ROWS,       // h3 forward: below this many token rows use the fp32-MFMA kernels
  OPT_X6_MIN_ROWS,       // x6 forward: the same
  OPT_ATTN_CFG,          // fp32-MFMA attention: workgroup shape (micro-benchmarks)
  OPT_ATTN_X6,           // anyloc_attention: 1 = split-bf16 products for every call, 0 = never, -1 = as the caller asks
  OPT_VLAD_PARTS,        // workgroups per image of the fused VLAD kernel (0 = chosen from the image count)
  OPT_VLAD_TWO_PASS,     // 1 = force the general two-pass VLAD path
  OPT_VLAD_FUSED_V,      // fused VLAD kernel: 0 = default choice, 1 = exact-score kernel, 3 / 4 = screening kernel with 4 / 8 waves
  OPT_KMEANS_FUSED_V,    // the same for the k-means step
  OPT_KMEANS_MAX_CHUNKS, // k-means: upper limit of row chunks (partial sums); 0 = two per CU
  OPT_H3_MFMA16,         // gemm_h3: 1 = large GEMMs on the 16x16x32 MFMA kernel (gemm_h3m.hip) where it has the epilogue
  OPT_H3_SWIGLU_T,       // Python host: build the SwiGLU fc1 image in the 16-channel block layout (transposed-accumulator epilogue)
  OPT_H3_FAST_SILU,      // fused SwiGLU epilogue of the h3 w12 GEMM: SiLU on v_exp_f32 + v_rcp_f32 instead of expf + IEEE division
  OPT_TOPK_FEWQ_X6,      // few-query retrieval scores: 2 = two fp16 planes under a running row scale (scores_h3.hip), 1 = three bf16
                         // planes (scores_x6.hip), 0 = fp32 MFMA
  OPT_TOPK_H3,           // retrieval score panels on the two-term fp16 GEMM: -1 = where it pays, 0 = never, 1 = wherever possible
  // small-M plans of the two-term fp16 GEMM (gemm_h3s.hip): overrides of the built-in plan table for sweeps / A-B runs
  OPT_H3S_CFG,           // tile configuration id (-1 = the plan table)
  OPT_H3S_KSPLIT,        // split-K factor (0 = the plan table)
  OPT_H3S_KB,            // k-blocks per ring stage: 1, 2 or 4 (0 = the plan table)
  OPT_H3S_STAGES,        // ring depth: 3 or 6 (0 = the plan table)
  OPT_H3S_MASK,          // which GEMMs the three overrides apply to: bit 0 qkv, 1 proj, 2 fc1 / w12, 3 fc2, 4 others
  OPT_H3S_ENABLE,        // 1 = small-M plans (default), 0 = the round-3 small-batch kernels (64x64 two-wave tiles, no split-K)
  OPT_H3_PATCH,          // fp16 mode: patch embedding on the two-term fp16 GEMM (1, default) or the fp32 MFMA GEMM (0)
  OPT_TOPK_FEWQ_QDMA,    // few-query scores on fp16 planes: 1 = queries pre-split once, DMA'd into LDS per slab; 0 = split per slab
  OPT_H3S_W12_TALL,      // small-M plan of the w12 / fc1 GEMM of one image: 1 = 192 x 128 tiles (one workgroup per CU), 0 = 128 x 128
  OPT_ATTN_H3_QG,        // attention_h3: 32-query groups per wave, 1 (four waves of 32 queries, default) or 2 (two waves of 64: A/B)
  OPT_ATTN_H3_KS,        // attention_h3: key splits across the waves of a workgroup, 0 = by grid size (2 when all workgroups are resident), 1, 2
  OPT_H3S_LN_LEAD,       // one image per call: LayerNorm as the lead role of its consumer GEMM's launch (LN1 + qkv, LN2 + w12); 0 = two launches
  OPT_H3_LN_LEAD,        // batched calls: LayerNorm as lead workgroups interleaved with its consumer GEMM's tiles (LN1 + qkv, LN2 + fc1 / w12); 0 = two launches
  OPT_VLAD_GATHER_V,     // one-pass VLAD kernel at D = 1536: variants of the register-indexed gather kept for the hazard study (0 = shipped)
  OPT_TOPK_SCREEN,       // many-query retrieval: score panels on the leading fp16 planes + exact re-scoring of the rows inside the bound (scores_screen.hip): -1 = where it pays, 0 = never, 1 = wherever possible
  OPT_ATTN_H3_RAGGED_XCD, // ragged attention_h3: 1 = (image, head) units dealt round-robin over the XCDs, 0 = the uniform kernel's contiguous ranges
  OPT_TOPK_RESCORE_COLS, // screened retrieval: columns per slice of the re-scoring kernels: 0 = 49 152 (rows up to that width in one slice, on the
                         // single-slice kernels), or a multiple of 4096 up to 49 152, which sends every width through the sliced kernels (tests)
  OPT_COUNT
};
int64_t option(Option o);

int launch_status(const char* what);

// A kernel that needs more than the default 64 KiB of dynamic LDS must be told so with hipFuncSetAttribute -- a property of
// the (kernel, DEVICE) pair: a process that drives several GPUs (device = "cuda:N", the sharded bench) has to set it on each.
// One DynLds per launch site (a static local: one per kernel instantiation) remembers the devices already done as a bit set;
// a failed call is reported and NOT remembered.
struct DynLds { std::atomic<unsigned long long> seen{0}; };
inline int ensure_dyn_lds(DynLds& st, const void* fn, int bytes) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return hip_fail(hipGetLastError(), "hipGetDevice");
  const unsigned long long bit = 1ull << (dev & 63);
  if (dev < 64 && (st.seen.load(std::memory_order_relaxed) & bit)) return ANYLOC_OK;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
  if (dev < 64) st.seen.fetch_or(bit, std::memory_order_relaxed);
  return ANYLOC_OK;
}

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// run-time value -> template argument: calls f(std::integral_constant<int, V>) with the smallest V of the ascending list that
// is >= v (the last one when none is) -- the smallest compiled variant that holds v
template <int V, int... Rest, class F>
auto with_constant(int v, F&& f) {
  if constexpr (sizeof...(Rest) == 0) {
    return f(std::integral_constant<int, V>{});
  } else {
    if (v <= V) return f(std::integral_constant<int, V>{});
    return with_constant<Rest...>(v, f);
  }
}

// bump allocator over the caller's workspace
struct Arena {
  char* base;
  size_t cap, off;
  Arena(void* p, size_t n) : base(static_cast<char*>(p)), cap(n), off(0) {}
  template <class T>
  T* take(size_t count) {
    size_t bytes = align_up(count * sizeof(T), 256);
    T* r = reinterpret_cast<T*>(base + off);
    off += bytes;
    return r;
  }
  bool ok() const { return off <= cap; }
};

// ---- device helpers --------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// torch's clamp_min (F.normalize's denominator, max(||x||, eps)): a NaN norm stays NaN, so a row that holds a NaN comes out
// all NaN, as the reference's does.  fmaxf(NaN, eps) is eps: the row's other elements would come out finite, x / eps.
__device__ __forceinline__ float clamp_min_nan(float v, float lo) { return v < lo ? lo : v; }

// A GATED launch (topk.hip, ANYLOC_TOPK_NO_WAIT): the host enqueues it without knowing whether it is needed; a device word written
// by an earlier kernel of the stream decides.  Asked at kernel entry, before any barrier or LDS use; the answer is the same for
// every lane of the launch.
__device__ __forceinline__ bool gate_closed(const int* gate) { return gate != nullptr && *gate == 0; }

// ---- exact three-way bf16 split (split-bf16 GEMM / attention): x = x1 + x2 + x3, round-to-nearest-even at every
// step, residuals exact in fp32.  Two values per call: v_cvt_pk_bf16_f32 rounds and packs a pair in one instruction;
// pk[plane] = (plane of a) | (plane of b) << 16.
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split_pair_x3(float a, float b, unsigned pk[3]) {
#pragma unroll
  for (int pl = 0; pl < 3; ++pl) {
    f32x2 v;
    v[0] = a; v[1] = b;
    const unsigned u = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
    pk[pl] = u;
    a -= __uint_as_float(u << 16);               // exact
    b -= __uint_as_float(u & 0xffff0000u);
  }
}

// ---- internal kernels shared between translation units ---------------------
enum GemmEpilogue {
  EPI_STORE = 0,      // C = acc (+ bias)
  EPI_GELU = 1,       // C = gelu_erf(acc + bias)
  EPI_LS_RESID = 2,   // C = resid + gamma * (acc + bias)        (C may alias resid)
  EPI_SWIGLU = 3,     // C[:, n/2] = silu(acc_gate + b) * (acc_val + b), rows pair-interleaved
  EPI_PATCH = 4,      // C[b*T + 1 + p, :] = acc + bias + pos[1 + p, :]
  // gemm_h3 only: the result leaves the kernel already quantised for its consumer (no fp32 round trip)
  EPI_QKV_PLANES = 5, // q | k | v written as per-head two-plane fp16 tiles + one 2^-e per (32-row group, head): attention_h3
  EPI_GELU_H2 = 6,    // gelu(acc + bias) written as the h2 image of the next GEMM, rows scaled by the caller's c_inv
  EPI_SWIGLU_H2 = 7,  // silu(gate) * value, the same
  // gemm_h3 only, weights in the 16-channel block layout (anyloc_vit_block_h2.fc1_layout = 1): the product is formed
  // transposed (weights as the MFMA A operand), a lane holds one token and 8 consecutive gate / value channels
  EPI_SWIGLU_T = 8,   // C[:, n/2] = silu(gate) * value as fp32
  EPI_SWIGLU_T_H2 = 9,// ... as the h2 image of the next GEMM, 16-byte chunks straight from the accumulators
  // gemm_h3 only, rotary models (DINOv3): EPI_QKV_PLANES with the q and k columns of the patch rows rotated (H3Problem::rope)
  // between descale + bias and the tile's maximum.  An epilogue of its own so that the kernels of EPI_QKV_PLANES stay the
  // code they were; it has the plans of EPI_QKV_PLANES (plan_epilogue)
  EPI_QKV_PLANES_ROPE = 10
};
// the epilogue whose plans (tile shape, ring, split-K, lead role) an epilogue runs on
constexpr int plan_epilogue(int epi) { return epi == EPI_QKV_PLANES_ROPE ? EPI_QKV_PLANES : epi; }

struct GemmProblem {
  const float* A; int64_t lda;
  const float* W; int64_t ldw;
  float* C; int64_t ldc;
  int64_t M, N, K;
  const float* bias;     // [N] or null
  const float* gamma;    // EPI_LS_RESID
  const float* resid;    // EPI_LS_RESID, leading dim ldc
  const float* pos;      // EPI_PATCH: [T, N]
  int patches;           // EPI_PATCH: patches per image (T = patches + 1)
  float* rowsq;          // optional: rowsq[m] = sum_k A[m,k]^2 (written by the n-block 0 column)
  const char* tag;       // profiling label
  // split-K (gemm_nt_splitk): K is the SLICE length, slice s contracts columns [s K, (s+1) K) of both operands (row
  // strides lda / ldw unchanged) into C + s * c_split_stride (and rowsq + s * M): the caller sums the slices
  int ksplit; int64_t c_split_stride;
};
int gemm_nt(const GemmProblem& p, int epilogue, hipStream_t stream);
// C_s[M, N<=64] = A[:, slice s] W[:, slice s]^T for s < ksplit in ONE launch (grid.y = slice) on 128 x 64 tiles, with the
// partial row sums of squares of A: few-query retrieval, where a plain GEMM would have too few tiles to stream HBM
int gemm_nt_splitk(const GemmProblem& p, hipStream_t stream);
// the same pass with both operands split on the fly into three bf16 planes (six bf16 MFMA products, fp32 accumulate):
// part[s][row][0..63] and rsq_part[s][row] for K slices s < ksplit of length kslice (scores_x6.hip)
int scores_fewq_x6(const float* db, int64_t ldd, int64_t rows, const float* queries, int64_t ldq, int64_t nq, int64_t kslice,
                   int ksplit, float* part, float* rsq_part, hipStream_t stream);
// the same pass on two fp16 planes under a running power-of-two row scale: three fp16 MFMA products (scores_h3.hip); qinv[nq] =
// 2^-e of the query rows (row_scales_h2)
size_t fewq_query_image_bytes(int64_t dim);
int fewq_query_image(const float* queries, int64_t ldq, int64_t nq, const float* qinv, int64_t dim, unsigned char* qimg,
                     hipStream_t stream);
int scores_fewq_h3(const float* db, int64_t ldd, int64_t rows, const float* queries, int64_t ldq, int64_t nq, const float* qinv,
                   const unsigned char* qimg, int64_t kslice, int ksplit, float* part, float* rsq_part, hipStream_t stream);

// split-bf16 GEMM on three-plane bf16 operand images (gemm_x6.hip)
struct X6Problem {
  const unsigned char* A3; int64_t RA;     // plane image of A [M, 16*K16], RA = rows the image was built with
  const unsigned char* W3; int64_t RW;     // plane image of W [N, 16*K16]
  float* C; int64_t ldc;
  unsigned char* C3; int64_t RC;            // optional (GELU / SwiGLU): write the result as a plane image with RC rows
  int64_t M, N;
  int K16;                                  // k-blocks of 16
  int64_t a_off, w_off;                     // byte offset of A3 / W3 inside its image (row sub-range of a larger image)
  const float* bias;
  const float* gamma;                       // EPI_LS_RESID
  const float* resid;                       // EPI_LS_RESID, leading dim ldc
  const char* tag;
};
size_t x3_bytes(int64_t rows, int64_t K);
int split_x3(const float* x, int64_t ldx, int64_t rows, int64_t K, void* x3, hipStream_t stream);
int gemm_x6(const X6Problem& p, int epilogue, hipStream_t stream);
int layernorm_x3(const float* x, const float* w, const float* b, int64_t rows, int dim, float eps, void* x3,
                 hipStream_t stream);

// Rotary positions (DINOv3): which rotation a token row of a forward gets.  table = fp32 rows of 64, cos[0..31] | sin[0..31]
// of one patch each (the angles of columns d and d + 32 of a head are equal), the same for every head and block.  Token row
// `row` is row t of image i; t < prefix (CLS and the registers) is not rotated, otherwise patch t - prefix of image i's table.
// meta == nullptr: a uniform batch, i = row / T, one table; otherwise the ragged table of the call (RAGGED_TOK gives i, and
// RAGGED_POS the first ROW of image i's table in the packed tables)
struct RopeRows {
  const float* table;
  const int64_t* meta; int n_img;
  int T, prefix;
};
// the image whose rows [off(i), off(i+1)) hold row r, off(i) = tok[i] - sub * i (strictly ascending for sub <= 1 + R)
__device__ __forceinline__ int ragged_image(const int64_t* __restrict__ tok, int n_img, int64_t r, int sub) {
  int lo = 0, hi = n_img - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tok[mid] - (int64_t)sub * mid <= r) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}
// -> the 64 floats of `row`'s rotation, or nullptr for a prefix row.  hint: an image at or before the row's (ragged: a walk
// from there instead of a search; 0 is always valid)
__device__ __forceinline__ const float* rope_row(const RopeRows& rp, int64_t row, int hint = 0) {
  if (!rp.meta) {
    const int t = (int)(row % rp.T) - rp.prefix;
    return t < 0 ? nullptr : rp.table + (int64_t)t * 64;
  }
  int i = hint;
  while (i + 1 < rp.n_img && rp.meta[i + 1] <= row) ++i;
  const int64_t t = row - rp.meta[i] - rp.prefix;
  return t < 0 ? nullptr : rp.table + (rp.meta[2 * (int64_t)(rp.n_img + 1) + i] + t) * 64;
}

// row-scaled two-term fp16 GEMM on two-plane operand images (gemm_h3.hip)
struct H3Problem {
  const unsigned char* A2; int64_t RA; const float* a_inv;   // image of A [M, 16*K16], rows of the image, 2^-e per row
  const unsigned char* W2; int64_t RW; const float* w_inv;   // image of W [N, 16*K16]
  float* C; int64_t ldc;
  int64_t M, N;
  int K16;
  int64_t a_off, w_off;                     // byte offset of A2 / W2 inside its image (row sub-range)
  const float* bias;
  const float* gamma;                       // EPI_LS_RESID
  const float* resid;                       // EPI_LS_RESID, leading dim ldc
  int accumulate;                           // EPI_STORE: C += A W^T (a long contraction cut into K chunks, one launch each)
  // the next three are the plan's (H3Plan): the launcher copies them here, whatever the caller left in them
  int fast_silu;                            // EPI_SWIGLU_H2 / _T / _T_H2: SiLU on v_exp_f32 / v_rcp_f32
  int epi_lds;                              // EPI_LS_RESID: transposed 16-byte epilogue through LDS
  int group_m;                              // tile-rows per XCD scheduling group
  // split-K (small-M plans, gemm_h3s.hip): ksplit > 1 cuts the contraction into ksplit ranges of kper k-blocks, one
  // workgroup each; partial accumulators meet in sk_part, the last arrival of a tile (sk_tickets, zero between launches)
  // sums them in split order and runs the epilogue.  Both buffers: h3_split_workspace().
  int ksplit, kper;
  float* sk_part; unsigned* sk_tickets;
  int kind;                                 // which block GEMM this is (H3_KIND_*: plan table / option h3s_mask); 0 = other
  const float* pos; int patches;            // EPI_PATCH: position table [patches + 1, N]; row b * patches + p -> C row b * (patches + 1) + 1 + p
  // EPI_QKV_PLANES: N = 3 * heads * 64; see QkvPlanes below
  unsigned char* qkv_planes; float* qkv_inv; int heads; int64_t groups;
  // EPI_QKV_PLANES_ROPE: the rotation table(s) of the call (RopeRows below)
  RopeRows rope;
  // EPI_GELU_H2 / EPI_SWIGLU_H2: output image (RC rows) quantised with the given per-row 2^-e (c_inv[row])
  unsigned char* C2; int64_t RC; const float* c_inv;
  // FFN-bound telemetry (optional): c_max[row] = bits of the largest scaled magnitude the row holds in the output image, merged by
  // atomicMax (one per row and wave: +0.09 ms per one-image ViT-g forward, lost in the noise of a batched one)
  unsigned* c_max;
  // LayerNorm LEAD role (small-M plans, gemm_h3s.hip; round 6): when ln_x is set, the first ln_wgs workgroups of the launch
  // normalise the rows of ln_x (one row per wave, the arithmetic of layernorm_h2) straight into THIS GEMM's operand image (A2 /
  // a_inv, and c_inv when ln_bound is set) with write-through stores and count the rows of every BM-row tile in ln_tickets; a
  // GEMM workgroup waits for its row tile's count before it stages A.  One launch instead of two for LN1 + qkv and LN2 + w12.
  const float* ln_x; const float* ln_w; const float* ln_b; float ln_eps; int ln_dim;
  float ln_bound[4]; int ln_has_bound;
  unsigned* ln_tickets; int ln_wgs;
  const char* tag;
  // EPI_STORE only (the retrieval's score panels): device word that decides whether the launch works at all -- nullptr = run;
  // *gate == 0: every workgroup returns at entry (gate_closed below).  Last member: no other field moves.
  const int* gate;
};

// Layout of the Q / K / V operand tiles attention_h3 consumes (written by gemm_h3's EPI_QKV_PLANES epilogue).
// Rows (tokens of all images, M = batch * T) are cut into GLOBAL groups of 32 rows (group g = rows 32g .. 32g+31,
// independent of image boundaries); every (part p in {q,k,v}, head h, group g) owns one power-of-two scale
//   inv[(p * heads + h) * groups + g] = 2^-e,  max |x| * 2^e in [2^14, 2^15)  over the 32 x 64 values of the tile,
// and two fp16 planes (x * 2^e = hi + lo) of 4 KiB each at byte offset (((p * heads + h) * groups + g) * 2 + plane) * 4096:
//   q, k:  [row 0..31][8 chunks of 8 d]   chunk c of row r sits at  r * 128 + ((c ^ ((r >> 1) & 7)) << 4)
//   v:     [d 0..63][4 chunks of 8 rows]  chunk (hh * 2 + s) of column d holds rows (j & 3) + 8 * (2 s + (j >> 2)) + 4 hh,
//          j = 0..7 -- the order the MFMA C/D registers of a 32-row block hold them -- at d * 64 + ((chunk ^ ((d >> 2) & 3)) << 4)
// Both images are what a wave reads conflict-free with ds_read_b128 after a linear global -> LDS DMA of the tile.
inline size_t qkv_planes_bytes(int64_t rows, int heads) { return (size_t)3 * heads * ((rows + 31) / 32) * 2 * 4096; }
inline size_t qkv_inv_count(int64_t rows, int heads) { return (size_t)3 * heads * ((rows + 31) / 32); }
size_t h2_bytes(int64_t rows, int64_t K);
int split_h2(const float* x, int64_t ldx, int64_t rows, int64_t K, void* h2, float* inv_scale, hipStream_t stream);
// rows of any width (K % 16 == 0; used above 4096 columns): also returns the rows' sums of squares when row_sumsq != nullptr
int split_h2_wide(const float* x, int64_t ldx, int64_t rows, int64_t K, void* h2, float* inv_scale, float* row_sumsq,
                  hipStream_t stream, const int* gate = nullptr);
// the first half of it alone: inv_scale[row] = 2^-e of the row-scaled split (and the rows' sums of squares when asked)
int row_scales_h2(const float* x, int64_t ldx, int64_t rows, int64_t K, float* inv_scale, float* row_sumsq, hipStream_t stream);
int split_h1_wide(const float* x, int64_t ldx, int64_t rows, int64_t K, void* h2, float* inv_scale, float* row_sumsq, float* resid_sq,
                  hipStream_t stream);
// bound (HOST array of 4 floats) != nullptr: also writes bound_inv[row] = 2^-e for an upper bound of the FFN hidden activation of that row
// (Cauchy-Schwarz: |fc1 output| <= ||ln(x)||_2 * max_j ||W_j||_2 + max |b|), bound = {gate_norm, gate_bias, val_norm, val_bias}
int layernorm_h2(const float* x, const float* w, const float* b, int64_t rows, int dim, float eps, void* h2,
                 float* inv_scale, hipStream_t stream, const float* bound = nullptr, float* bound_inv = nullptr);
// attention on the tiles of EPI_QKV_PLANES; writes the h2 image (+ per-row 2^-e) the projection GEMM reads.  tok_off == nullptr:
// n_img images of T rows each (rows = n_img * T); otherwise images of different lengths, tok_off = device [n_img + 1] row offsets,
// T the longest image, rows the total
int attention_h3(const unsigned char* planes, const float* inv, int64_t n_img, int T, const int64_t* tok_off, int64_t rows, int D,
                 int heads, unsigned char* out2, float* out_inv, hipStream_t stream);
// test / fallback producer of the same tiles from an fp32 [rows, 3D] buffer
int qkv_planes_from_f32(const float* qkv, int64_t rows, int D, int heads, unsigned char* planes, float* inv,
                        hipStream_t stream);
// FFN-bound telemetry: rowmax [nblocks][M] = bits of the largest scaled magnitude every row of a block's fc2 operand image holds
// (atomicMax by the fc1 / w12 epilogue, zero = block not run fused) -> out[l * groups + g] = max over the rows of group g
// (rows_per_group consecutive rows: an image, or all M) of 2^15 / rowmax; 0 for a block that left no maxima
int ffn_looseness(const unsigned* rowmax, int nblocks, int64_t M, int64_t rows_per_group, float* out, hipStream_t stream);
// small-M plans (gemm_h3s.hip): GEMMs of fewer than ~2 workgroups of 128 x 256 per CU -- one or a few images per call
enum { H3_KIND_OTHER = 0, H3_KIND_QKV = 1, H3_KIND_PROJ = 2, H3_KIND_FC1 = 3, H3_KIND_FC2 = 4 };
constexpr size_t H3_SPLIT_PART_BYTES = 48u << 20;      // partial accumulators of one split-K launch (<= 1024 workgroups x 32 KiB + slack)
constexpr size_t H3_SPLIT_TICKETS = 4096;               // tiles of one split-K launch
inline size_t h3_split_workspace_bytes() { return H3_SPLIT_PART_BYTES + H3_SPLIT_TICKETS * sizeof(unsigned) + 512; }
// How one GEMM runs: everything its launch needs that is not in the problem.  h3_plan (gemm_h3s.hip) is the one place that
// decides it, from the problem, the epilogue and the options, without a HIP call.
enum { H3_ROUTE_SMALL, H3_ROUTE_FIXED, H3_ROUTE_BATCHED };
struct H3Plan {
  int mfma16;            // first try the 16 x 16 x 32 MFMA kernel (gemm_h3m.hip); the rest is the launch of gemm_h3_kernel otherwise
  int route;             // the small-M plan table | the two fixed shapes of the epilogues without small-M plans | option h3_cfg's shapes
  int tile;              // id in kSmallTile (small-M plans) or kH3Tile (gemm_h3_kernel.hpp)
  int kb, stages;        // k-blocks per ring stage, ring depth
  int ksplit, kper;      // split-K: ranges of the contraction and k-blocks per range (1, K16: unsplit)
  int lead;              // LayerNorm lead role (H3Problem::ln_x): 0 = none, 1 = small-M, 2 = batched
  int tiles_m, tiles_n;
  unsigned grid;
  // what the kernel reads from its argument and the options decide: gemm_h3 copies them into H3Problem's fields of the same names
  int group_m;           // tile-rows per XCD scheduling group (option h3_group_m)
  int epi_lds;           // EPI_LS_RESID: 16-byte accesses through LDS (option h3_epi_lds, and C / resid aligned for them)
  int fast_silu;         // the SwiGLU epilogues that quantise or transpose (option h3_fast_silu)
};
// option h3_group_m as every kernel that orders its tiles by XCD groups takes it (gemm_h3_kernel, gemm_h3m_kernel, gemm_screen_kernel)
int h3_group_m();
// ln_in_front: the caller has a LayerNorm whose output is this GEMM's operand image and asks whether the launch can carry it
// as its lead role (plan.lead != 0: set H3Problem::ln_x ...; 0: the caller launches layernorm_h2 itself)
H3Plan h3_plan(const H3Problem& p, int epilogue, bool ln_in_front);
// plan == nullptr: planned here (with the lead role when p.ln_x is set: an error when the launch cannot carry it)
int gemm_h3(const H3Problem& p, int epilogue, hipStream_t stream, const H3Plan* plan = nullptr);
int gemm_h3_small(const H3Problem& p, int epilogue, const H3Plan& plan, hipStream_t stream);      // gemm_h3's launch of a small-M plan
int h3_lead_plan_check(int tiles_m, int tiles_n, int group_m, int64_t M, unsigned* grid);
// the same GEMM on v_mfma_f32_16x16x32_f16 (gemm_h3m.hip); ANYLOC_ERR_UNSUPPORTED for epilogues it does not have
int gemm_h3m(const H3Problem& p, int epilogue, hipStream_t stream);
// screened retrieval (scores_screen.hip)
float screen_accum(int k16_chunk, int chunks);
int screen_resid(const unsigned char* img, int64_t R, int K16, int64_t rows, const float* inv, const float* ss, float* rho,
                 unsigned* rho_max, hipStream_t stream);
int gemm_screen(const H3Problem& p, hipStream_t stream);
int screen_rho_max(const float* rho, int64_t n, unsigned* rho_max, hipStream_t stream);
int screen_rho_from_resid(const float* resid_sq, const float* inv, const float* ss, int64_t rows, float* rho, unsigned* rho_max,
                          hipStream_t stream);
int screen_margins(const float* qn, const float* rho_q, const unsigned* rho_max, const unsigned* ss_max, int64_t nq, int metric,
                   float accum, float* margin, hipStream_t stream);
int screen_compact(const float* scores, int64_t ld, int64_t ncols, int64_t nq, int k, int metric, const float* qn, const float* dn,
                   const float* dnorm, const float* thr, const float* margin, int cmax, int* cand, int* count, int* overflow,
                   int* over_q, hipStream_t stream);
// over_q[q] != 0 for the queries that overflowed in some range -> plan[0] = how many, plan[1] = 1 <= plan[0] <= side_cap,
// plan[2] = plan[0] > side_cap, plan[4 + j] = the j-th of them in ascending order (j < side_cap <= SCREEN_SIDE_Q; -1 beyond)
constexpr int SCREEN_SIDE_Q = 64;
constexpr int SCREEN_PLAN_INTS = 4 + SCREEN_SIDE_Q;
int screen_overflow_plan(const int* over_q, int64_t nq, int side_cap, int* plan, hipStream_t stream);
// re-scoring: `slice` = 0: the whole row in one slice, the query in registers (dim <= SCREEN_RESCORE_COLS); otherwise the columns
// per slice of the sliced kernels, a multiple of 4096 up to SCREEN_RESCORE_COLS (any dim; cmax <= SCREEN_CMAX)
constexpr int SCREEN_CMAX = 512;          // candidates per query and column range; more: the call re-runs unscreened
constexpr int64_t SCREEN_RESCORE_COLS = 2048 * 24;
bool screen_rescore_supported(int64_t dim);
int screen_rescore(const float* queries, const float* db, int64_t dim, int64_t slice, int64_t nq, int cmax, const int* cand,
                   const int* count, int metric, const float* qn, const float* dn, const float* dnorm, float* cand_v, hipStream_t stream);
// the same from the two planes of a prepared index (img + p * slot: the image of panel p; dinv: the 2^-e of ALL rows; the
// candidates are columns of the range that starts at database row s0; dn / dnorm already point at that range)
int screen_rescore_planes(const float* queries, const unsigned char* img, size_t slot, int64_t panel, int64_t ndb, int64_t s0,
                          const float* dinv, int64_t dim, int64_t slice, int64_t nq, int cmax, const int* cand, const int* count,
                          int metric, const float* qn, const float* dn, const float* dnorm, float* cand_v, hipStream_t stream);
int screen_select(const int* cand, const float* cand_v, const int* count, int cmax, int64_t col_base, int64_t nq, int k, float* run_v,
                  int64_t* run_i, int first, hipStream_t stream);

int l2norm_rows(const float* x, int64_t ldx, float* out, int64_t ldo, int64_t rows,
                int64_t dim, float eps, hipStream_t stream);
int layernorm(const float* x, float* y, const float* w, const float* b, int64_t rows, int dim,
              float eps, hipStream_t stream);
int im2col(const float* img, float* col, int64_t batch, int H, int W, int P, int kpad,
           hipStream_t stream);
int cls_rows(float* x, const float* cls, const float* pos, int64_t batch, int T, int dim,
             hipStream_t stream);
// the kept rows of every T-row image: skip leading rows, and gap more after row 0 (the register rows behind a kept CLS row)
int facet_rows(const float* src, int64_t lds_, int coff, float* out, int64_t ldo, int ooff,
               int64_t batch, int T, int skip, int gap, int rows_per_img, int dim, int normalize, float eps,
               hipStream_t stream);
// fp32 / split-bf16 attention on qkv [rows, 3D]; n_img, T, tok_off, rows as attention_h3's
int attention(const float* qkv, float* out, int64_t n_img, int T, const int64_t* tok_off, int64_t rows, int D, int heads,
              hipStream_t stream, unsigned char* out3 = nullptr,    // out3: write the result as a plane image instead
              bool x6 = false);                                      // x6: split-bf16 matrix products

// ragged batches (anyloc_vit_forward_ragged): the device table `meta` is int64 [RAGGED_ROWS][n_img + 1], row-major --
//   RAGGED_TOK: token-row offsets (T_i = 1 + R + N_i rows per image: CLS, R registers, patches), entry n_img = total rows
//   RAGGED_PIX: float offset of image i in the packed CHW input, RAGGED_POS: first row of image i's positional table in the
//   packed tables, RAGGED_H / RAGGED_W: the image size (last entry of these three unused)
//   (a rotary model has rotation tables instead: RAGGED_POS = first row of image i's [N_i, 64] table in the packed tables)
enum { RAGGED_TOK = 0, RAGGED_PIX = 1, RAGGED_POS = 2, RAGGED_H = 3, RAGGED_W = 4, RAGGED_ROWS = 5 };
static_assert(RAGGED_TOK == 0 && RAGGED_POS == 2, "rope_row reads rows 0 and 2 of the table");
int im2col_ragged(const float* img, float* col, const int64_t* meta, int n_img, int R, int64_t patch_rows, int P, int kpad,
                  hipStream_t stream);
// the token rows from the patch GEMM's output [P, D]: CLS + pos[0], R register rows, patch + pos rows.  meta == nullptr: a
// uniform batch of T-row images sharing the table pos; otherwise the ragged table (T unused)
// pos == nullptr (rotary models): no positional term anywhere
int embed_rows(float* x, const float* patch, const float* cls, const float* reg, int R, const float* pos, const int64_t* meta,
               int n_img, int T, int64_t rows, int dim, hipStream_t stream);
// the rotation of RopeRows in place on the q and k thirds of fp32 qkv [rows, 3 * heads * 64] (v and the prefix rows untouched)
int rope_rows(float* qkv, int64_t rows, int heads, const RopeRows& rp, hipStream_t stream);
int facet_rows_ragged(const float* src, int64_t lds_, int coff, float* out, int64_t ldo, int ooff, const int64_t* meta,
                      int n_img, int64_t out_rows, int skip, int gap, int dim, int normalize, float eps, hipStream_t stream);
// FFN-bound telemetry, one figure per (block, image) of a ragged batch
int ffn_looseness_ragged(const unsigned* rowmax, int nblocks, int64_t M, const int64_t* tok_off, int n_img, float* out,
                         hipStream_t stream);

// single-pass fused VLAD / k-means (vlad_fused.hip)
struct FusedArgs {
  const float* x;          // [total, D] tokens / rows
  const int64_t* offsets;  // VLAD: [units+1] token offsets (device); k-means: null
  int64_t chunk_rows;      // k-means: rows per unit
  int64_t total;           // total rows
  int D, K;
  const float* chat;       // [32, D] fpk-normalised centres (rows >= K are zero)
  const float* cbias;      // [32] additive score bias (euclidean mode) or zeros
  const float* centers;    // [K, D] raw centres (VLAD residual) or null
  float* out;              // VLAD: [units, K*D]; k-means: [units, K, D] partial sums
  unsigned* cnt_part;      // k-means: [units, K] label counts; VLAD: null
  int64_t* lab64;          // optional [total] labels
  int norm_descs, intra;
  int metric;              // 0 cosine (||chat_k|| = 1), 1 euclidean (chat = 2 c, cbias = -||c||^2): scales fused3's error bound
  int parts;               // VLAD: workgroups per image (1 = one each); > 1 needs the two buffers below
  float* part_buf;         // [units, parts, K, D] partial sums
  unsigned* part_tickets;  // [units] arrival counters (zeroed by the launcher)
};
bool fused_supported(int64_t D, int64_t K);
int vlad_fused(const FusedArgs& a, int64_t units, bool kmeans, hipStream_t stream);

}  // namespace anyloc
