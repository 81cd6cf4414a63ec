// DINOv2 ViT forward with early exit at the last tapped layer.
//
// replaces: DinoV2ExtractFeatures.__call__ (reference utilities.py:263-285):
// the torch.hub DINOv2 forward at :269, the forward-hook capture of
// blocks[L].attn.qkv / blocks[L] (:245-252, :258-261), CLS drop (:270-273),
// facet slice (:274-281) and F.normalize (:282-283).
//
// The reference runs all blocks, the final norm and the head and throws the
// result away; only the hooked tensor is used.  Here execution stops at the
// last tap, and when a q/k/v tap sits in the last executed block only that
// facet's third of the QKV projection is computed.
//
// Per block (every GEMM in the arithmetic of the call -- Arith below -- with a fused epilogue; shown for fp32):
//   y   = LN1(x)                                    layernorm
//   qkv = y Wqkv^T + b                              EPI_STORE
//   a   = softmax((q/8) k^T) v                      attention.hip
//   x  += ls1 * (a Wproj^T + b)                     EPI_LS_RESID (in place)
//   y   = LN2(x)
//   h   = gelu(y W1^T + b)  |  silu(y Wg^T+b)*(y Wv^T+b)    EPI_GELU | EPI_SWIGLU
//   x  += ls2 * (h W2^T + b)                        EPI_LS_RESID (in place)
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "common.hpp"

struct anyloc_vit {
  anyloc_vit_config cfg;
  const float* patch_w;
  const float* patch_b;
  const float* cls;
  const float* regs = nullptr;              // register tokens (device [n_reg, dim], caller-owned) or null
  int n_reg = 0;                            // R: token rows per image are CLS, R registers, patches
  int rope = 0;                             // 1: rotary positions (DINOv3) -- no positional table, q / k of the patch rows rotated
  float ln_eps = 1e-6f;                     // eps of every LayerNorm of the forward
  std::vector<anyloc_vit_block_weights> blocks;
  std::vector<anyloc_vit_block_x3> x3;      // optional: three-plane bf16 images of the four weight matrices
  std::vector<anyloc_vit_block_h2> h2;      // optional: two-plane fp16 images + row scales of the same matrices
  std::vector<char> ffn_exact;              // per block: 1 = quantise the FFN activation against the exact row maximum
  float* ffn_looseness = nullptr;           // telemetry target (device [depth] or [depth][batch]) or null
  int telemetry_per_image = 0;              // 1: one figure per (block, image) instead of one per block
  unsigned char* patch_w2 = nullptr;        // fp16 mode: two-plane image + row scales of patch_w, built (and owned) by
  float* patch_inv = nullptr;               // anyloc_vit_attach_h2
  void drop_patch_image() {
    if (patch_w2) (void)hipFree(patch_w2);
    if (patch_inv) (void)hipFree(patch_inv);
    patch_w2 = nullptr;
    patch_inv = nullptr;
  }
};

namespace anyloc {
namespace {

struct VitWs {
  float *x, *y, *qkv, *h;   // qkv doubles as the im2col buffer; attention output aliases y
  unsigned char* a3;        // split-bf16 mode: plane image of a D-wide activation operand (LN output, attention output)
  unsigned char* h3;        //                  plane image of the FFN hidden activation
  float *ainv, *hinv;       // fp16 mode: 2^-e per row of the images in a3 / h3
  float* qinv;              // fp16 mode, fused attention: 2^-e per (part, head, 32-row group) tile of q | k | v (in qkv)
  float* sk_part;           // fp16 mode, small-M plans: partial accumulators of a split-K launch (gemm_h3s.hip)
  unsigned* sk_tickets;     //                           arrival counters per tile, zero between launches
  unsigned* ln_tickets;     // fp16 mode, LayerNorm lead role (gemm_h3_kernel.hpp): [depth][2][ln_tk] rows done per 128-row tile of a lead launch
  size_t ln_tk;             //   words per launch: max(16, ceil(M / 128))
  unsigned* hmax;           // fp16 mode, FFN-bound telemetry: [depth][M] largest scaled magnitude per row (bits); tickets, lead
                            // tickets and these lie back to back so that ONE memset per forward clears them
  size_t bytes;
};

// M token rows, P patch rows (uniform: batch * T and batch * np; ragged: the sums over the images)
VitWs carve(void* ws, size_t cap, const anyloc_vit_config& c, int64_t M, int64_t P) {
  Arena a(ws, cap);
  VitWs w;
  w.x = a.take<float>(M * c.dim);
  w.y = a.take<float>(M * c.dim);
  // fp32 [M, 3D], or the im2col patches, or (fp16 mode) the q | k | v tiles of attention_h3: rows padded to 32
  const int64_t qkv_elems = std::max<int64_t>((M + 31) / 32 * 32 * 3 * c.dim, P * ((c.patch_k_pad + 15) / 16 * 16));
  w.qkv = a.take<float>(qkv_elems);
  w.h = a.take<float>(M * c.ffn_hidden);
  // (fp16 mode also quantises the gathered patches into a3: [batch * np, patch_k_pad rounded up to 16] as two fp16 planes)
  w.a3 = a.take<unsigned char>(std::max(x3_bytes(M, c.dim), h2_bytes(P, (c.patch_k_pad + 15) / 16 * 16)));
  w.h3 = a.take<unsigned char>(x3_bytes(M, c.ffn_hidden));
  w.ainv = a.take<float>(M);
  w.hinv = a.take<float>(M);
  w.qinv = a.take<float>(qkv_inv_count(M, c.heads));
  w.sk_part = a.take<float>(H3_SPLIT_PART_BYTES / sizeof(float));
  w.sk_tickets = a.take<unsigned>(H3_SPLIT_TICKETS);
  w.ln_tk = std::max<size_t>(16, (size_t)((M + 127) / 128));
  w.ln_tickets = a.take<unsigned>((size_t)c.depth * 2 * w.ln_tk);
  w.hmax = a.take<unsigned>((size_t)c.depth * M);
  w.bytes = a.off;
  return w;
}

// which kernels the GEMMs of a forward run on: fp32 MFMA (gemm_f32.hip), six bf16 products of three-plane images (gemm_x6.hip),
// three fp16 products of row-scaled two-plane images (gemm_h3.hip)
enum class Arith { F32, X6, H3 };

// an activation operand [M, K]: its fp32 rows and the place of its operand image (x6: three bf16 planes; h3: two fp16 planes
// and 2^-e per row in inv).  quantised: the producer wrote the image (the fp32 rows do not exist); otherwise the GEMM's
// arithmetic quantises the rows into it first
struct Act {
  const float* rows;
  unsigned char* img;
  float* inv;
  int64_t M, K;
  bool quantised;
};

// a weight matrix [rows, K] in the form each arithmetic reads (those the call does not use may be null)
struct Weights {
  const float* f32;
  const void* x3;
  const void* h2;
  const float* h2_inv;
  int64_t rows;
};

// One linear layer of the forward, C = epi(A W^T + bias): `describe` fills the problem of the call's arithmetic with what
// every such GEMM has, the call site sets by name what only this GEMM has, `run` launches it.
struct BlockGemm {
  Arith arith;
  Act a;
  GemmProblem f32;
  X6Problem x6;
  H3Problem h3;
  // h3, optional: the LayerNorm whose output IS the operand image (a.img / a.inv; with ln_bound, HOST [4], also the FFN bound
  // into h3.c_inv).  ln_tickets: zeroed words of this launch, one per 128-row tile (VitWs::ln_tk)
  const float *ln_x, *ln_w, *ln_b, *ln_bound;
  float ln_eps;
  unsigned* ln_tickets;
};

// N output columns from rows row0 .. row0 + N of wt.  kind (H3_KIND_*) other than OTHER also hands an h3 launch the split-K
// buffers: the small-M plans belong to the fused data flow; the unfused one (A/B runs, layers with a q / k / v tap) keeps
// the fixed tile shapes it was measured with
BlockGemm describe(Arith arith, const char* tag, const Act& a, const Weights& wt, int64_t row0, int64_t N, const float* bias,
                   float* C, int64_t ldc, int kind, const VitWs& ws) {
  BlockGemm g{};
  g.arith = arith;
  g.a = a;
  auto shared = [&](auto& p) {
    p.C = C; p.ldc = ldc;
    p.M = a.M; p.N = N;
    p.bias = bias;
    p.resid = C;
    p.tag = tag;
  };
  switch (arith) {
    case Arith::F32:
      shared(g.f32);
      g.f32.A = a.rows; g.f32.lda = a.K;
      g.f32.W = wt.f32 + row0 * a.K; g.f32.ldw = a.K;
      g.f32.K = a.K;
      break;
    case Arith::X6:
      shared(g.x6);
      g.x6.A3 = a.img; g.x6.RA = g.x6.RC = a.M;
      g.x6.W3 = static_cast<const unsigned char*>(wt.x3) + row0 * 32; g.x6.RW = wt.rows; g.x6.w_off = row0 * 32;
      g.x6.K16 = (int)((a.K + 15) / 16);
      break;
    case Arith::H3:
      shared(g.h3);
      g.h3.A2 = a.img; g.h3.RA = g.h3.RC = a.M; g.h3.a_inv = a.inv;
      g.h3.W2 = static_cast<const unsigned char*>(wt.h2) + row0 * 32; g.h3.RW = wt.rows; g.h3.w_off = row0 * 32;
      g.h3.w_inv = wt.h2_inv + row0;
      g.h3.K16 = (int)(a.K / 16);
      g.h3.groups = (a.M + 31) / 32;
      g.h3.kind = kind;
      if (kind != H3_KIND_OTHER) { g.h3.sk_part = ws.sk_part; g.h3.sk_tickets = ws.sk_tickets; }
      break;
  }
  return g;
}

// gamma: the LayerScale of EPI_LS_RESID (x += gamma * (A W^T + bias), in place)
int run(BlockGemm& g, int epi, hipStream_t stream, const float* gamma = nullptr) {
  const Act& a = g.a;
  switch (g.arith) {
    case Arith::F32:
      g.f32.gamma = gamma;
      return gemm_nt(g.f32, epi, stream);
    case Arith::X6:
      if (!a.quantised) ANYLOC_TRY(split_x3(a.rows, a.K, a.M, a.K, a.img, stream));
      g.x6.gamma = gamma;
      return gemm_x6(g.x6, epi, stream);
    case Arith::H3: {
      H3Problem& p = g.h3;
      if (!a.quantised) ANYLOC_TRY(split_h2(a.rows, a.K, a.M, a.K, a.img, a.inv, stream));
      p.gamma = gamma;
      const H3Plan plan = h3_plan(p, epi, g.ln_x != nullptr);
      if (plan.lead) {
        // the LayerNorm as the lead role of the GEMM's own launch (one image per call: LN1 + qkv, LN2 + w12) ...
        p.ln_x = g.ln_x; p.ln_w = g.ln_w; p.ln_b = g.ln_b; p.ln_eps = g.ln_eps; p.ln_dim = (int)a.K;
        p.ln_has_bound = g.ln_bound != nullptr;
        for (int i = 0; i < 4; ++i) p.ln_bound[i] = g.ln_bound ? g.ln_bound[i] : 0.0f;
        p.ln_tickets = g.ln_tickets;
      } else if (g.ln_x) {
        // ... or as a launch of its own in front of it: the same arithmetic, the same bits
        ANYLOC_TRY(layernorm_h2(g.ln_x, g.ln_w, g.ln_b, a.M, (int)a.K, g.ln_eps, a.img, a.inv, stream, g.ln_bound,
                                g.ln_bound ? const_cast<float*>(p.c_inv) : nullptr));
      }
      return gemm_h3(p, epi, stream, &plan);
    }
  }
  return ANYLOC_ERR_INVALID_ARG;
}

// the tap list of a forward; `who` is the entry point's name in the messages
int check_taps(const char* who, const anyloc_vit_config& c, int32_t n_taps, const int32_t* tap_layers, const int32_t* tap_facets) {
  ANYLOC_CHECK_ARG(n_taps >= 1 && n_taps <= 64, "%s: n_taps %d", who, n_taps);
  for (int t = 0; t < n_taps; ++t) {
    ANYLOC_CHECK_ARG(tap_layers[t] >= 0 && tap_layers[t] < c.depth, "%s: tap layer %d outside [0,%d)", who, tap_layers[t], c.depth);
    ANYLOC_CHECK_ARG(tap_facets[t] >= 0 && tap_facets[t] <= 3, "%s: facet %d", who, tap_facets[t]);
    ANYLOC_CHECK_ARG(t == 0 || tap_layers[t] >= tap_layers[t - 1], "%s: tap layers must ascend", who);
  }
  return ANYLOC_OK;
}

}  // namespace
}  // namespace anyloc

using namespace anyloc;

extern "C" {

int anyloc_layernorm(const float* x, float* y, const float* weight, const float* bias, int64_t rows, int64_t dim,
                     float eps, void* stream) {
  ANYLOC_CHECK_ARG(x && y && weight && bias && rows > 0 && dim > 0, "layernorm: bad args");
  ANYLOC_CHECK_ARG(rows < (1ll << 31) && dim < (1ll << 31), "layernorm: rows %lld and dim %lld must both be below 2^31", (long long)rows,
                   (long long)dim);
  return layernorm(x, y, weight, bias, rows, (int)dim, eps, static_cast<hipStream_t>(stream));
}

int anyloc_attention(const float* qkv, float* out, int64_t batch, int64_t tokens, int64_t dim, int64_t heads,
                     void* stream) {
  ANYLOC_CHECK_ARG(qkv && out, "attention: null pointer");
  ANYLOC_CHECK_ARG(batch > 0 && batch < 65536, "attention: batch %lld outside [1, 65535]", (long long)batch);
  ANYLOC_CHECK_ARG(tokens > 0 && tokens < (1ll << 31) && dim > 0 && dim < (1ll << 31) && heads > 0 && heads < (1ll << 31),
                   "attention: tokens %lld, dim %lld and heads %lld must be positive and below 2^31", (long long)tokens, (long long)dim,
                   (long long)heads);
  return attention(qkv, out, batch, (int)tokens, nullptr, batch * tokens, (int)dim, (int)heads, static_cast<hipStream_t>(stream));
}

size_t anyloc_attention_h3_workspace_bytes(int64_t batch, int64_t tokens, int64_t heads) {
  if (batch <= 0 || tokens <= 0 || heads <= 0) return 0;
  const int64_t rows = batch * tokens;
  return align_up(qkv_planes_bytes(rows, (int)heads), 256) + align_up(qkv_inv_count(rows, (int)heads) * sizeof(float), 256) + 256;
}

// anyloc_attention_h3 and anyloc_attention_h3_ragged: the q | k | v tiles of fp32 qkv [rows, 3 * dim] in the caller's workspace
static int h3_tiles_in_workspace(const char* who, const float* qkv, int64_t rows, int64_t dim, int64_t heads, void* workspace,
                                 size_t workspace_bytes, hipStream_t stream, unsigned char** planes, float** inv) {
  // (attn_plan's limit on the q, k and v tile images, made here in front of the launch that builds them)
  ANYLOC_CHECK_ARG(rows < (1ll << 31) && heads < (1 << 20) && heads * ((rows + 31) / 32) * 8192 < (1ll << 31),
                   "%s: operand tiles exceed the 2 GiB buffer-addressing range: heads * ceil(rows / 32) * 8192 < 2^31 (rows=%lld heads=%lld)",
                   who, (long long)rows, (long long)heads);
  if (workspace_bytes < anyloc_attention_h3_workspace_bytes(1, rows, heads)) {
    set_error("%s: workspace %zu < %zu", who, workspace_bytes, anyloc_attention_h3_workspace_bytes(1, rows, heads));
    return ANYLOC_ERR_WORKSPACE;
  }
  Arena a(workspace, workspace_bytes);
  *planes = a.take<unsigned char>(qkv_planes_bytes(rows, (int)heads));
  *inv = a.take<float>(qkv_inv_count(rows, (int)heads));
  return qkv_planes_from_f32(qkv, rows, (int)dim, (int)heads, *planes, *inv, stream);
}

int anyloc_attention_h3(const float* qkv, void* out_img, float* out_inv, int64_t batch, int64_t tokens, int64_t dim,
                        int64_t heads, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  ANYLOC_CHECK_ARG(qkv && out_img && out_inv && workspace, "attention_h3: null pointer");
  ANYLOC_CHECK_ARG(batch > 0 && tokens > 0 && heads > 0 && dim == heads * 64, "attention_h3: bad shape");
  ANYLOC_CHECK_ARG(batch < 65536, "attention_h3: batch %lld outside [1, 65535]", (long long)batch);   // (before the tiles are built)
  ANYLOC_CHECK_ARG(tokens < (1ll << 31), "attention_h3: tokens %lld must be below 2^31", (long long)tokens);
  unsigned char* planes;
  float* inv;
  ANYLOC_TRY(h3_tiles_in_workspace("attention_h3", qkv, batch * tokens, dim, heads, workspace, workspace_bytes, stream, &planes, &inv));
  return attention_h3(planes, inv, batch, (int)tokens, nullptr, batch * tokens, (int)dim, (int)heads,
                      static_cast<unsigned char*>(out_img), out_inv, stream);
}

int anyloc_vit_create(anyloc_vit_t** out, const anyloc_vit_config* cfg, const float* patch_w, const float* patch_b,
                      const float* cls_token, const anyloc_vit_block_weights* blocks) {
  ANYLOC_CHECK_ARG(out && cfg && patch_w && patch_b && cls_token && blocks, "vit_create: null pointer");
  ANYLOC_CHECK_ARG(cfg->dim > 0 && cfg->dim % 64 == 0 && cfg->heads * 64 == cfg->dim,
                   "vit_create: dim %d / heads %d (head_dim must be 64)", cfg->dim, cfg->heads);
  ANYLOC_CHECK_ARG(cfg->depth > 0 && cfg->depth <= 256, "vit_create: depth %d", cfg->depth);
  ANYLOC_CHECK_ARG(cfg->ffn_kind == 0 || cfg->ffn_kind == 1, "vit_create: ffn_kind %d", cfg->ffn_kind);
  ANYLOC_CHECK_ARG(cfg->ffn_hidden > 0 && cfg->ffn_hidden % 64 == 0, "vit_create: ffn_hidden %d", cfg->ffn_hidden);
  ANYLOC_CHECK_ARG(cfg->patch > 0 && cfg->patch_k_pad >= 3 * cfg->patch * cfg->patch && cfg->patch_k_pad % 4 == 0,
                   "vit_create: patch %d / patch_k_pad %d", cfg->patch, cfg->patch_k_pad);
  for (int i = 0; i < cfg->depth; ++i) {
    const anyloc_vit_block_weights& b = blocks[i];
    ANYLOC_CHECK_ARG(b.norm1_w && b.norm1_b && b.qkv_w && b.qkv_b && b.proj_w && b.proj_b && b.ls1 && b.norm2_w &&
                         b.norm2_b && b.fc1_w && b.fc1_b && b.fc2_w && b.fc2_b && b.ls2,
                     "vit_create: block %d has a null weight", i);
  }
  anyloc_vit* h = new (std::nothrow) anyloc_vit();
  if (!h) {
    set_error("vit_create: out of host memory");
    return ANYLOC_ERR_HIP;
  }
  h->cfg = *cfg;
  h->patch_w = patch_w;
  h->patch_b = patch_b;
  h->cls = cls_token;
  h->blocks.assign(blocks, blocks + cfg->depth);
  *out = h;
  return ANYLOC_OK;
}

int anyloc_vit_attach_x3(anyloc_vit_t* h, const anyloc_vit_block_x3* blocks) {
  ANYLOC_CHECK_ARG(h, "vit_attach_x3: null handle");
  if (!blocks) {
    h->x3.clear();
    return ANYLOC_OK;
  }
  for (int i = 0; i < h->cfg.depth; ++i)
    ANYLOC_CHECK_ARG(blocks[i].qkv_w3 && blocks[i].proj_w3 && blocks[i].fc1_w3 && blocks[i].fc2_w3,
                     "vit_attach_x3: block %d has a null plane image", i);
  h->x3.assign(blocks, blocks + h->cfg.depth);
  return ANYLOC_OK;
}

int anyloc_vit_attach_h2(anyloc_vit_t* h, const anyloc_vit_block_h2* blocks) {
  ANYLOC_CHECK_ARG(h, "vit_attach_h2: null handle");
  h->drop_patch_image();
  if (!blocks) {
    h->h2.clear();
    h->ffn_exact.assign(h->cfg.depth, 0);
    return ANYLOC_OK;
  }
  // (ffn_hidden 5120 = ViT-H+/16, the widest model the path has been run with: tests/test_gpu_dinov3.py)
  ANYLOC_CHECK_ARG(h->cfg.dim % 16 == 0 && h->cfg.ffn_hidden % 16 == 0 && h->cfg.ffn_hidden <= 5120 && h->cfg.dim <= 2048,
                   "vit_attach_h2: dim %d / ffn_hidden %d outside the fp16 path's limits", h->cfg.dim, h->cfg.ffn_hidden);
  for (int i = 0; i < h->cfg.depth; ++i) {
    const anyloc_vit_block_h2& b = blocks[i];
    ANYLOC_CHECK_ARG(b.qkv_w2 && b.qkv_inv && b.proj_w2 && b.proj_inv && b.fc1_w2 && b.fc1_inv && b.fc2_w2 && b.fc2_inv,
                     "vit_attach_h2: block %d has a null image or scale array", i);
    ANYLOC_CHECK_ARG(b.fc1_layout == 0 || (b.fc1_layout == 1 && h->cfg.ffn_kind == 1 && b.fc1_b2 && h->cfg.ffn_hidden % 64 == 0),
                     "vit_attach_h2: block %d: fc1_layout %d (1 needs a SwiGLU model, fc1_b2 and ffn_hidden %% 64 == 0)", i,
                     b.fc1_layout);
  }
  // The patch-embedding weights [dim, patch_k_pad] as an operand image of the same GEMM, the contraction zero-padded to
  // whole 16-element k-blocks (one-off, on the null stream).  Built FIRST, on the device that owns patch_w (not whatever
  // device is current), every temporary freed on every path; the handle changes only when all of it succeeded -- a failed
  // attach leaves the handle as it was before the call, minus the previous patch image (already dropped above, with the
  // previous h2 blocks detached by the clear() below).
  // The call has no stream argument and the caller's patch_w may still be in flight on ANY stream (a non-blocking stream is
  // not ordered against the null stream): the device is drained first, the null stream once more before the temporaries
  // go -- construction time, the one place of this file that synchronises (include/anyloc_hip.h, "Streams").
  h->h2.clear();
  h->ffn_exact.assign(h->cfg.depth, 0);      // the exact-quantiser switches belong to the weights that are being replaced
  const int64_t D = h->cfg.dim, K0 = h->cfg.patch_k_pad, Kp = (K0 + 15) / 16 * 16;
  int prev_dev = -1, w_dev = -1;
  hipPointerAttribute_t attr;
  if (hipGetDevice(&prev_dev) == hipSuccess && hipPointerGetAttributes(&attr, h->patch_w) == hipSuccess &&
      attr.type == hipMemoryTypeDevice)
    w_dev = attr.device;
  else
    (void)hipGetLastError();                 // (an unregistered pointer: stay on the current device)
  if (w_dev >= 0 && w_dev != prev_dev) ANYLOC_HIP(hipSetDevice(w_dev));
  float* padded = nullptr;
  unsigned char* w2 = nullptr;
  float* winv = nullptr;
  int rc = ANYLOC_OK;
  auto hip_ok = [&](hipError_t e, const char* what) {
    if (e != hipSuccess && rc == ANYLOC_OK) {
      set_error("vit_attach_h2: %s: %s", what, hipGetErrorString(e));
      rc = ANYLOC_ERR_HIP;
    }
    return e == hipSuccess;
  };
  if (hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize") &&
      hip_ok(hipMalloc(reinterpret_cast<void**>(&padded), sizeof(float) * D * Kp), "hipMalloc (padded patch weights)") &&
      hip_ok(hipMalloc(reinterpret_cast<void**>(&w2), h2_bytes(D, Kp)), "hipMalloc (patch-embedding image)") &&
      hip_ok(hipMalloc(reinterpret_cast<void**>(&winv), sizeof(float) * D), "hipMalloc (patch-embedding row scales)") &&
      hip_ok(hipMemset(padded, 0, sizeof(float) * D * Kp), "hipMemset") &&
      hip_ok(hipMemcpy2D(padded, sizeof(float) * Kp, h->patch_w, sizeof(float) * K0, sizeof(float) * K0, D, hipMemcpyDeviceToDevice),
             "hipMemcpy2D")) {
    rc = split_h2(padded, Kp, D, Kp, w2, winv, nullptr);
    if (rc == ANYLOC_OK) hip_ok(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
  }
  if (padded) (void)hipFree(padded);
  if (rc != ANYLOC_OK) {
    if (w2) (void)hipFree(w2);
    if (winv) (void)hipFree(winv);
  }
  if (w_dev >= 0 && w_dev != prev_dev) (void)hipSetDevice(prev_dev);
  if (rc != ANYLOC_OK) return rc;
  h->patch_w2 = w2;
  h->patch_inv = winv;
  h->h2.assign(blocks, blocks + h->cfg.depth);
  return ANYLOC_OK;
}

int anyloc_vit_set_registers(anyloc_vit_t* h, const float* register_tokens, int32_t n_registers) {
  ANYLOC_CHECK_ARG(h, "vit_set_registers: null handle");
  ANYLOC_CHECK_ARG(n_registers >= 0 && n_registers <= 16, "vit_set_registers: %d registers outside [0, 16]", n_registers);
  ANYLOC_CHECK_ARG(register_tokens || n_registers == 0, "vit_set_registers: null register tokens with %d registers", n_registers);
  h->regs = n_registers ? register_tokens : nullptr;
  h->n_reg = n_registers;
  return ANYLOC_OK;
}

int anyloc_vit_set_rope(anyloc_vit_t* h, int32_t on) {
  ANYLOC_CHECK_ARG(h, "vit_set_rope: null handle");
  h->rope = on ? 1 : 0;
  return ANYLOC_OK;
}

int anyloc_vit_set_ln_eps(anyloc_vit_t* h, float eps) {
  ANYLOC_CHECK_ARG(h, "vit_set_ln_eps: null handle");
  ANYLOC_CHECK_ARG(eps > 0.0f && eps < 1.0f, "vit_set_ln_eps: eps %g outside (0, 1)", (double)eps);
  h->ln_eps = eps;
  return ANYLOC_OK;
}

int anyloc_rope_rows(float* qkv, int64_t rows, int64_t heads, const float* table, int64_t tokens, int64_t prefix,
                     const int64_t* dev_meta, int32_t n_img, void* stream) {
  ANYLOC_CHECK_ARG(qkv && table, "rope_rows: null pointer");
  ANYLOC_CHECK_ARG(rows > 0 && heads > 0 && heads < 65536 && prefix >= 0 && prefix < (1 << 20), "rope_rows: bad shape");
  ANYLOC_CHECK_ARG(dev_meta ? n_img > 0 : (tokens > prefix && tokens < (1ll << 31) && rows % tokens == 0),
                   "rope_rows: uniform rows need rows = batch * tokens and tokens > prefix; ragged rows the table and n_img > 0");
  const RopeRows rp{table, dev_meta, dev_meta ? n_img : 0, dev_meta ? 0 : (int)tokens, (int)prefix};
  return rope_rows(qkv, rows, (int)heads, rp, static_cast<hipStream_t>(stream));
}

int anyloc_vit_set_telemetry(anyloc_vit_t* h, float* ffn_looseness, int32_t per_image) {
  ANYLOC_CHECK_ARG(h, "vit_set_telemetry: null handle");
  h->ffn_looseness = ffn_looseness;
  h->telemetry_per_image = per_image ? 1 : 0;
  return ANYLOC_OK;
}

int anyloc_vit_block_ffn_exact(anyloc_vit_t* h, int32_t layer, int32_t exact) {
  ANYLOC_CHECK_ARG(h && layer >= 0 && layer < h->cfg.depth, "vit_block_ffn_exact: bad handle / layer");
  if (h->ffn_exact.size() != (size_t)h->cfg.depth) h->ffn_exact.assign(h->cfg.depth, 0);
  h->ffn_exact[layer] = exact ? 1 : 0;
  return ANYLOC_OK;
}

void anyloc_vit_destroy(anyloc_vit_t* h) {
  if (h) h->drop_patch_image();
  delete h;
}

size_t anyloc_vit_workspace_bytes(const anyloc_vit_t* h, int64_t batch, int64_t img_h, int64_t img_w) {
  if (!h || batch <= 0 || img_h < h->cfg.patch || img_w < h->cfg.patch) return 0;
  const int64_t np = (img_h / h->cfg.patch) * (img_w / h->cfg.patch);
  return carve(nullptr, 0, h->cfg, batch * (np + 1 + h->n_reg), batch * np).bytes + 256;
}

// a ragged batch (anyloc_vit_forward_ragged): images of different sizes packed back to back
struct RaggedBatch {
  const int64_t* meta;      // device table (common.hpp, RAGGED_*)
  int64_t rows;             // token rows, sum of T_i
  int max_T;                // the longest image
};

// the launch sequence of one forward on `stream` (shape and taps already validated by anyloc_vit_forward /
// anyloc_vit_forward_ragged).  rg == nullptr: `batch` images of img_h x img_w; otherwise `batch` images of the sizes in rg
// (img_h / img_w unused) -- the block GEMMs, LayerNorms and quantisers work on rows and do not see the difference
static int vit_forward_launches(anyloc_vit_t* h, const float* img, int64_t batch, int64_t img_h, int64_t img_w,
                                const float* pos, int32_t n_taps, const int32_t* tap_layers, const int32_t* tap_facets,
                                unsigned flags, float* out, void* workspace, size_t workspace_bytes, hipStream_t stream,
                                const RaggedBatch* rg = nullptr) {
  const anyloc_vit_config& c = h->cfg;
  const int D = c.dim, Hh = c.ffn_hidden, np = rg ? 0 : (int)(img_h / c.patch) * (int)(img_w / c.patch);
  const int R = h->n_reg;                       // register rows per image (after CLS, before the patches)
  const int T = rg ? rg->max_T : np + 1 + R;
  const int64_t M = rg ? rg->rows : batch * T, P = rg ? rg->rows - batch * (1 + R) : batch * np;
  const int64_t* meta = rg ? rg->meta : nullptr;
  const VitWs w = carve(workspace, workspace_bytes, c, M, P);
  if (!workspace || w.bytes > workspace_bytes) {
    set_error("vit_forward: workspace %zu < %zu", workspace_bytes, w.bytes);
    return ANYLOC_ERR_WORKSPACE;
  }
  ANYLOC_CHECK_ARG(!(flags & ANYLOC_VIT_SPLIT_BF16) || !h->x3.empty(),
                   "vit_forward: ANYLOC_VIT_SPLIT_BF16 without anyloc_vit_attach_x3");
  ANYLOC_CHECK_ARG(!(flags & ANYLOC_VIT_SPLIT_FP16) || !h->h2.empty(),
                   "vit_forward: ANYLOC_VIT_SPLIT_FP16 without anyloc_vit_attach_h2");
  // The arithmetic of the call.  h3 has no row threshold by default: with q | k | v, the attention output and the FFN
  // activation kept in fp16 planes it beats the fp32-MFMA kernels at every batch (B=1: 9.6 vs 16.5 ms,
  // profiles/r02_extractor_vs_batch.log).  x6 is honoured from option x6_min_rows (1600) rows up: below ~3 images of 530
  // tokens its GEMMs have too few 128-row tiles to fill 256 CUs twice over and the fp32-MFMA kernel with its 64-row split is
  // faster (measured B=1: 60 vs 40 images/s)
  const Arith arith = (flags & ANYLOC_VIT_SPLIT_FP16) && M >= option(OPT_H3_MIN_ROWS)   ? Arith::H3
                      : (flags & ANYLOC_VIT_SPLIT_BF16) && M >= option(OPT_X6_MIN_ROWS) ? Arith::X6
                                                                                        : Arith::F32;
  const bool h3 = arith == Arith::H3, x6 = arith == Arith::X6;
  // options x6_fuse / h3_fuse = 0 (A/B measurements and tests): activations stay fp32 and are quantised in front of every GEMM
  const bool fuse_x6 = x6 && option(OPT_X6_FUSE) != 0, fuse_h3 = h3 && option(OPT_H3_FUSE) != 0;
  const bool use_cls = flags & ANYLOC_VIT_USE_CLS;
  // the tap drops the register rows: without the CLS row a skip of 1 + R, with it a gap of R behind row 0
  const int rows_per_img = use_cls ? np + 1 : np, skip = use_cls ? 0 : 1 + R, gap = use_cls ? R : 0;
  const int64_t out_rows = rg ? (use_cls ? M - batch * R : P) : batch * rows_per_img;
  const int64_t ldo = (int64_t)n_taps * D;
  const int norm_taps = (flags & ANYLOC_VIT_NORM_TAPS) ? 1 : 0;
  // the tapped rows of src (width lds_, columns coff ..) -> out columns ooff ..
  auto facet = [&](const float* src, int64_t lds_, int coff, int ooff) {
    if (rg) return facet_rows_ragged(src, lds_, coff, out, ldo, ooff, meta, (int)batch, out_rows, skip, gap, D, norm_taps, 1e-12f, stream);
    return facet_rows(src, lds_, coff, out, ldo, ooff, batch, T, skip, gap, rows_per_img, D, norm_taps, 1e-12f, stream);
  };
  // is the block output (token) / a q, k or v facet (!token) of layer l tapped?
  auto tapped = [&](int l, bool token) {
    for (int t = 0; t < n_taps; ++t)
      if (tap_layers[t] == l && (tap_facets[t] == ANYLOC_FACET_TOKEN) == token) return true;
    return false;
  };
  const int last_layer = tap_layers[n_taps - 1];
  // split-K arrival counters; with telemetry on also the rows' maxima of every block that will run (adjacent: one memset)
  const bool telem = h3 && h->ffn_looseness != nullptr;
  if (h3)
    ANYLOC_HIP(hipMemsetAsync(w.sk_tickets, 0,
                              telem ? (size_t)(reinterpret_cast<char*>(w.hmax + (size_t)(last_layer + 1) * M) - reinterpret_cast<char*>(w.sk_tickets))
                                    : (size_t)(reinterpret_cast<char*>(w.hmax) - reinterpret_cast<char*>(w.sk_tickets)),
                              stream));

  // ---- patch embedding: conv PxP stride P == GEMM over gathered patches, + bias + pos ----
  // h3: the gathered patches are quantised like every other operand (row maximum -> power-of-two scale), the contraction
  // padded to whole 16-element k-blocks
  const bool patch_h3 = h3 && h->patch_w2 && option(OPT_H3_PATCH) != 0;
  const int kp = patch_h3 ? (c.patch_k_pad + 15) / 16 * 16 : c.patch_k_pad;
  float* col = w.qkv;
  if (rg) ANYLOC_TRY(im2col_ragged(img, col, meta, (int)batch, R, P, c.patch, kp, stream));
  else ANYLOC_TRY(im2col(img, col, batch, (int)img_h, (int)img_w, c.patch, kp, stream));
  // ragged or with registers: the patch GEMM with its bias epilogue into w.y [P, D]; embed_rows then adds each image's
  // positional rows and writes the CLS and register rows (the same two sums as EPI_PATCH + cls_rows)
  // a rotary model takes the same pass: its rows have no positional term, `pos` is the rotation table(s) of the call
  const bool rope = h->rope != 0;
  const bool embed_pass = rg || R > 0 || rope;
  const RopeRows rp{pos, meta, rg ? (int)batch : 0, T, 1 + R};
  const float eps = h->ln_eps;
  const Act patches{col, w.a3, w.ainv, P, kp, false};
  const Weights Wpatch{h->patch_w, nullptr, h->patch_w2, h->patch_inv, D};
  BlockGemm pe = describe(patch_h3 ? Arith::H3 : Arith::F32, "vit_patch_embed_gemm", patches, Wpatch, 0, D, h->patch_b,
                          embed_pass ? w.y : w.x, D, H3_KIND_OTHER, w);
  pe.f32.pos = pe.h3.pos = embed_pass ? nullptr : pos;
  pe.f32.patches = pe.h3.patches = np;
  ANYLOC_TRY(run(pe, embed_pass ? EPI_STORE : EPI_PATCH, stream));
  if (embed_pass) ANYLOC_TRY(embed_rows(w.x, w.y, h->cls, h->regs, R, rope ? nullptr : pos, meta, (int)batch, T, M, D, stream));
  else ANYLOC_TRY(cls_rows(w.x, h->cls, pos, batch, T, D, stream));

  // y = LN(x): as the operand image of the GEMM that follows (h3 always, x6 when fused) or as fp32 rows in w.y
  const bool ln_quantises = h3 || fuse_x6;
  auto layer_norm = [&](const float* nw, const float* nb) {
    if (h3) return layernorm_h2(w.x, nw, nb, M, D, eps, w.a3, w.ainv, stream);
    if (fuse_x6) return layernorm_x3(w.x, nw, nb, M, D, eps, w.a3, stream);
    return layernorm(w.x, w.y, nw, nb, M, D, eps, stream);
  };
  const Act y{w.y, w.a3, w.ainv, M, D, ln_quantises};
  static const anyloc_vit_block_x3 no_x3{};
  static const anyloc_vit_block_h2 no_h2{};
  for (int l = 0; l <= last_layer; ++l) {
    const anyloc_vit_block_weights& b = h->blocks[l];
    const anyloc_vit_block_x3& b3 = x6 ? h->x3[l] : no_x3;
    const anyloc_vit_block_h2& b2 = h3 ? h->h2[l] : no_h2;
    const bool swiglu = c.ffn_kind == 1;
    const Weights Wqkv{b.qkv_w, b3.qkv_w3, b2.qkv_w2, b2.qkv_inv, 3 * D}, Wproj{b.proj_w, b3.proj_w3, b2.proj_w2, b2.proj_inv, D},
        Wfc1{b.fc1_w, b3.fc1_w3, b2.fc1_w2, b2.fc1_inv, swiglu ? 2 * Hh : Hh}, Wfc2{b.fc2_w, b3.fc2_w3, b2.fc2_w2, b2.fc2_inv, D};
    // ---- the block's decisions ----
    // only q / k / v taps remain: just the tapped thirds of the QKV projection are computed, and the forward ends
    const bool facet_exit = l == last_layer && !tapped(l, true);
    // attention fused: its output leaves as the operand image of the projection GEMM.  h3: q | k | v arrive as per-head
    // fp16 tiles too and never exist in fp32, so a q / k / v tap of the layer keeps the unfused data flow
    const bool fuse_attn = h3 ? fuse_h3 && !tapped(l, false) && D % 128 == 0 && !facet_exit : fuse_x6;
    // FFN fused: fc1 / w12 writes the hidden activation as fc2's operand image.  h3: quantised against the row bound that
    // LayerNorm 2 derives from the block's Cauchy-Schwarz constants, unless the block was switched to the exact row maximum
    const float* fb = b2.fc1_bound;
    const bool fuse_ffn = h3 ? fuse_h3 && (fb[0] > 0.f || fb[1] > 0.f) && !(l < (int)h->ffn_exact.size() && h->ffn_exact[l]) : fuse_x6;
    // h3, fused: LayerNorm 1 / 2 travels with the qkv / fc1 GEMM (BlockGemm::ln_x) instead of running here
    const bool h3_attn = h3 && fuse_attn, h3_ffn = h3 && fuse_ffn;

    // ---- y = LN1(x) ----
    if (!h3_attn) ANYLOC_TRY(layer_norm(b.norm1_w, b.norm1_b));
    if (facet_exit) {
      for (int t = 0; t < n_taps; ++t) {
        if (tap_layers[t] != l) continue;
        const int64_t row0 = (int64_t)tap_facets[t] * D;
        BlockGemm g = describe(arith, "vit_facet_gemm", y, Wqkv, row0, D, b.qkv_b + row0, w.qkv, D, H3_KIND_PROJ, w);
        ANYLOC_TRY(run(g, EPI_STORE, stream));
        ANYLOC_TRY(facet(w.qkv, D, 0, t * D));
      }
      break;
    }
    // ---- qkv = y Wqkv^T + b: fp32 [M, 3D], or (h3, fused) the per-head tiles attention_h3 reads by DMA ----
    BlockGemm qkv = describe(arith, "vit_qkv_gemm", y, Wqkv, 0, 3 * D, b.qkv_b, h3_attn ? nullptr : w.qkv, 3 * D,
                             h3_attn ? H3_KIND_QKV : H3_KIND_OTHER, w);
    if (h3_attn) {
      qkv.h3.qkv_planes = reinterpret_cast<unsigned char*>(w.qkv); qkv.h3.qkv_inv = w.qinv; qkv.h3.heads = c.heads;
      qkv.h3.rope = rp;
      qkv.ln_x = w.x; qkv.ln_w = b.norm1_w; qkv.ln_b = b.norm1_b; qkv.ln_eps = eps;
      qkv.ln_tickets = w.ln_tickets + (size_t)l * 2 * w.ln_tk;
    }
    // rotary model: q and k of the patch rows are rotated in the epilogue that writes their tiles, or -- where q | k | v exist
    // in fp32 -- in place AFTER the layer's q / k / v taps, which hand out the projections' outputs as they are
    ANYLOC_TRY(run(qkv, h3_attn ? (rope ? EPI_QKV_PLANES_ROPE : EPI_QKV_PLANES) : EPI_STORE, stream));
    for (int t = 0; t < n_taps; ++t)
      if (tap_layers[t] == l && tap_facets[t] != ANYLOC_FACET_TOKEN) ANYLOC_TRY(facet(w.qkv, 3 * D, tap_facets[t] * D, t * D));
    if (rope && !h3_attn) ANYLOC_TRY(rope_rows(w.qkv, M, c.heads, rp, stream));
    // ---- a = softmax((q/8) k^T) v ----
    const unsigned char* tiles = reinterpret_cast<const unsigned char*>(w.qkv);
    unsigned char* a_img = fuse_attn ? w.a3 : nullptr;     // x6: the output as the plane image instead of fp32 rows in w.y
    if (h3_attn) ANYLOC_TRY(attention_h3(tiles, w.qinv, batch, T, meta, M, D, c.heads, w.a3, w.ainv, stream));
    else ANYLOC_TRY(attention(w.qkv, w.y, batch, T, meta, M, D, c.heads, stream, a_img, x6 || h3));
    // ---- x += ls1 * (a Wproj^T + b)  (h3, unfused: a is fp32 -- its rows span all heads, the row maximum is only known now) ----
    const Act attn{w.y, w.a3, w.ainv, M, D, fuse_attn};
    BlockGemm proj = describe(arith, "vit_proj_gemm", attn, Wproj, 0, D, b.proj_b, w.x, D, h3_attn ? H3_KIND_PROJ : H3_KIND_OTHER, w);
    ANYLOC_TRY(run(proj, EPI_LS_RESID, stream, b.ls1));
    // ---- y = LN2(x) ----
    if (!h3_ffn) ANYLOC_TRY(layer_norm(b.norm2_w, b.norm2_b));
    // ---- h = gelu(y W1^T + b)  |  silu(y Wg^T + b) * (y Wv^T + b): fp32 [M, H], or the image of it ----
    BlockGemm fc1 = describe(arith, swiglu ? "vit_w12_gemm" : "vit_fc1_gemm", y, Wfc1, 0, Wfc1.rows,
                             swiglu && b2.fc1_b2 ? b2.fc1_b2 : b.fc1_b, h3_ffn ? nullptr : w.h, Hh,
                             h3_ffn ? H3_KIND_FC1 : H3_KIND_OTHER, w);
    if (h3_ffn) {
      // quantised in the epilogue against the row bound LayerNorm 2 leaves in w.hinv
      fc1.h3.C2 = w.h3; fc1.h3.c_inv = w.hinv;
      fc1.h3.c_max = telem ? w.hmax + (size_t)l * M : nullptr;
      fc1.ln_x = w.x; fc1.ln_w = b.norm2_w; fc1.ln_b = b.norm2_b; fc1.ln_bound = fb; fc1.ln_eps = eps;
      fc1.ln_tickets = w.ln_tickets + ((size_t)l * 2 + 1) * w.ln_tk;
    }
    if (x6 && fuse_ffn) fc1.x6.C3 = w.h3;
    ANYLOC_TRY(run(fc1, !swiglu              ? (h3_ffn ? EPI_GELU_H2 : EPI_GELU)
                        : b2.fc1_layout == 1 ? (h3_ffn ? EPI_SWIGLU_T_H2 : EPI_SWIGLU_T)
                                             : (h3_ffn ? EPI_SWIGLU_H2 : EPI_SWIGLU),
                   stream));
    // ---- x += ls2 * (h W2^T + b) ----
    const Act hid{w.h, w.h3, w.hinv, M, Hh, fuse_ffn};
    BlockGemm fc2 = describe(arith, "vit_fc2_gemm", hid, Wfc2, 0, D, b.fc2_b, w.x, D, h3_ffn ? H3_KIND_FC2 : H3_KIND_OTHER, w);
    ANYLOC_TRY(run(fc2, EPI_LS_RESID, stream, b.ls2));
    for (int t = 0; t < n_taps; ++t)
      if (tap_layers[t] == l && tap_facets[t] == ANYLOC_FACET_TOKEN) ANYLOC_TRY(facet(w.x, D, 0, t * D));
  }
  if (flags & ANYLOC_VIT_NORM_CONCAT)
    ANYLOC_TRY(l2norm_rows(out, ldo, out, ldo, out_rows, ldo, 1e-12f, stream));
  // FFN-bound telemetry: one figure per executed block (and image) from the row maxima the fc1 / w12 epilogues left
  if (telem && rg && h->telemetry_per_image)
    ANYLOC_TRY(ffn_looseness_ragged(w.hmax, last_layer + 1, M, meta, (int)batch, h->ffn_looseness, stream));
  else if (telem) ANYLOC_TRY(ffn_looseness(w.hmax, last_layer + 1, M, h->telemetry_per_image ? T : M, h->ffn_looseness, stream));
  return ANYLOC_OK;
}

int anyloc_vit_forward(anyloc_vit_t* h, const float* img, int64_t batch, int64_t img_h, int64_t img_w,
                       const float* pos, int32_t n_taps, const int32_t* tap_layers, const int32_t* tap_facets,
                       unsigned flags, float* out, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  ANYLOC_CHECK_ARG(h && img && pos && out && tap_layers && tap_facets, "vit_forward: null pointer");
  const anyloc_vit_config& c = h->cfg;
  ANYLOC_CHECK_ARG(batch > 0 && batch < 65536, "vit_forward: batch %lld", (long long)batch);
  ANYLOC_CHECK_ARG(img_h >= c.patch && img_w >= c.patch && img_h % c.patch == 0 && img_w % c.patch == 0,
                   "vit_forward: image %lldx%lld is not a positive multiple of the patch size %d", (long long)img_h,
                   (long long)img_w, c.patch);
  ANYLOC_TRY(check_taps("vit_forward", c, n_taps, tap_layers, tap_facets));
  return vit_forward_launches(h, img, batch, img_h, img_w, pos, n_taps, tap_layers, tap_facets, flags, out, workspace,
                              workspace_bytes, stream);
}

// ---- ragged batches (ABI 10) ----

// host-side check of the image sizes of a ragged call -> total token rows and the longest image
static int ragged_shape(const anyloc_vit_t* h, int32_t n_img, const int32_t* img_hw, int64_t* rows, int* max_T, const char* who) {
  ANYLOC_CHECK_ARG(h, "%s: null handle", who);
  ANYLOC_CHECK_ARG(img_hw, "%s: null size array", who);
  ANYLOC_CHECK_ARG(n_img > 0 && n_img < 65536, "%s: n_img %d outside [1, 65535]", who, n_img);
  const int P = h->cfg.patch;
  int64_t r = 0;
  int mt = 0;
  for (int i = 0; i < n_img; ++i) {
    const int64_t ih = img_hw[2 * i], iw = img_hw[2 * i + 1];
    ANYLOC_CHECK_ARG(ih >= P && iw >= P && ih % P == 0 && iw % P == 0 && ih <= 65535 && iw <= 65535,
                     "%s: image %d is %lldx%lld, not a positive multiple of the patch size %d", who, i, (long long)ih,
                     (long long)iw, P);
    const int64_t T = (ih / P) * (iw / P) + 1 + h->n_reg;
    ANYLOC_CHECK_ARG(T < (1 << 30), "%s: image %d has too many tokens", who, i);
    r += T;
    mt = std::max<int>(mt, (int)T);
  }
  ANYLOC_CHECK_ARG(r < (1ll << 31), "%s: %lld token rows in one call", who, (long long)r);
  *rows = r;
  *max_T = mt;
  return ANYLOC_OK;
}

size_t anyloc_vit_workspace_bytes_ragged(const anyloc_vit_t* h, int32_t n_img, const int32_t* img_hw) {
  int64_t rows = 0;
  int max_T = 0;
  if (ragged_shape(h, n_img, img_hw, &rows, &max_T, "vit_workspace_bytes_ragged") != ANYLOC_OK) return 0;
  return carve(nullptr, 0, h->cfg, rows, rows - (int64_t)n_img * (1 + h->n_reg)).bytes + 256;
}

int anyloc_vit_forward_ragged(anyloc_vit_t* h, const float* img, int32_t n_img, const int32_t* img_hw, const int64_t* dev_meta,
                              const float* pos, int32_t n_taps, const int32_t* tap_layers, const int32_t* tap_facets,
                              unsigned flags, float* out, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  int64_t rows = 0;
  int max_T = 0;
  ANYLOC_TRY(ragged_shape(h, n_img, img_hw, &rows, &max_T, "vit_forward_ragged"));
  ANYLOC_CHECK_ARG(img && dev_meta && pos && out && tap_layers && tap_facets, "vit_forward_ragged: null pointer");
  ANYLOC_TRY(check_taps("vit_forward_ragged", h->cfg, n_taps, tap_layers, tap_facets));
  const RaggedBatch rg{dev_meta, rows, max_T};
  return vit_forward_launches(h, img, n_img, 0, 0, pos, n_taps, tap_layers, tap_facets, flags, out, workspace, workspace_bytes,
                              stream, &rg);
}

// the attention kernels on their own, over a ragged batch (kernel tests): tokens = host [n_img] lengths, tok_off = device
// [n_img + 1] offsets of the same lengths
static int attention_ragged_shape(int32_t n_img, const int32_t* tokens, int64_t* rows, int* max_T) {
  ANYLOC_CHECK_ARG(tokens && n_img > 0 && n_img < 65536, "attention_ragged: n_img %d / null token counts", n_img);
  int64_t r = 0;
  int mt = 0;
  for (int i = 0; i < n_img; ++i) {
    ANYLOC_CHECK_ARG(tokens[i] > 0, "attention_ragged: image %d has %d tokens", i, tokens[i]);
    r += tokens[i];
    mt = std::max(mt, (int)tokens[i]);
  }
  *rows = r;
  *max_T = mt;
  return ANYLOC_OK;
}

int anyloc_attention_ragged(const float* qkv, float* out, int32_t n_img, const int32_t* tokens, const int64_t* tok_off,
                            int64_t dim, int64_t heads, void* stream) {
  ANYLOC_CHECK_ARG(qkv && out && tok_off, "attention_ragged: null pointer");
  int64_t rows = 0;
  int max_T = 0;
  ANYLOC_TRY(attention_ragged_shape(n_img, tokens, &rows, &max_T));
  return attention(qkv, out, n_img, max_T, tok_off, rows, (int)dim, (int)heads, static_cast<hipStream_t>(stream));
}

int anyloc_attention_h3_ragged(const float* qkv, void* out_img, float* out_inv, int32_t n_img, const int32_t* tokens,
                               const int64_t* tok_off, int64_t dim, int64_t heads, void* workspace, size_t workspace_bytes,
                               void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  ANYLOC_CHECK_ARG(qkv && out_img && out_inv && tok_off && workspace, "attention_h3_ragged: null pointer");
  ANYLOC_CHECK_ARG(heads > 0 && dim == heads * 64, "attention_h3_ragged: bad shape");
  int64_t rows = 0;
  int max_T = 0;
  ANYLOC_TRY(attention_ragged_shape(n_img, tokens, &rows, &max_T));
  unsigned char* planes;
  float* inv;
  ANYLOC_TRY(h3_tiles_in_workspace("attention_h3_ragged", qkv, rows, dim, heads, workspace, workspace_bytes, stream, &planes, &inv));
  return attention_h3(planes, inv, n_img, max_T, tok_off, rows, (int)dim, (int)heads, static_cast<unsigned char*>(out_img), out_inv,
                      stream);
}

}  // extern "C"
