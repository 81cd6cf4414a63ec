// Exact brute-force top-k retrieval (inner product / squared L2).
//
// replaces: faiss.IndexFlatIP / IndexFlatL2 .add + .search as called by get_top_k_recall (reference utilities.py:439-450).
//
// The database is processed in row panels: a GEMM writes the [nq, panel] score block, then one block per query merges the panel
// into that query's running top-k list (threshold filter against the list's k-th entry + one-wave selection; ties -> lower
// database index, deterministic).  Three scoring paths, one per call (topk_plan chooses, anyloc_topk_path names it):
//   fp32 panels  32 768 rows per panel on the fp32 MFMA GEMM (gemm_f32.hip); roofline: fp32 MFMA, 2*nq flop per database float
//   few queries  <= 64 queries against rows of >= 4096 columns: a [nq, panel] GEMM has too few tiles to stream the database, so
//                the panel is the M operand of a split-K launch (option topk_fewq_x6: scores_h3.hip / scores_x6.hip / gemm_nt_splitk)
//   fp16 panels  8192 rows per panel on the two-term fp16 GEMM (gemm_h3.hip), 2.5-3x the fp32-MFMA rate and as accurate: queries
//                quantised once per call, a panel once per panel -- or never: a PREPARED INDEX (anyloc_topk_index_build[_range])
//                holds every panel's operand image, row scales, sums of squares and residual norms, for every query count
// On the fp16 panels the SCREENED search (scores_screen.hip) scores whole column ranges on the leading planes alone and re-scores
// exactly the rows its error bound cannot rule out; when a query has more of those than SCREEN_CMAX the call falls back to the
// unscreened panel search, on the query operands it already has.  With ANYLOC_TOPK_NO_WAIT that decision is taken on the device
// (device_fallback): both remedies are enqueued behind gates, and a few overflowed queries are searched as a batch of their own.
// Where each decision lives: topk_plan -- path, panel height, query chunk, screened column range, few-query arithmetic; the one
// reader of the topk_* options, asked by carve, the searches, anyloc_topk_path, the index layout and the size functions of the ABI.
// topk_impl -- validation, the workspace check, whether THIS call screens, the fallback (device_fallback: the same without a wait).  prologue -- norms and the queries' operand
// images, once per call.  db_panel / score_panel -- a database panel as GEMM operand with its norms / the query-chunk x k-chunk loop
// on the fp16 planes.  screened_search, panel_search -- the two searches.  launch_* -- the one launch site of each kernel here.
#include <algorithm>
#include <optional>

#include "common.hpp"

namespace anyloc {

namespace {

constexpr int TILE = 2048;        // score columns per filtering step (at most TILE new candidates)
constexpr int BOOT = 256;         // columns of the very first step (no threshold yet: every column is a candidate)
constexpr int CAP = TILE + BOOT;  // candidates that beat the running k-th entry, buffered in LDS between selections
constexpr int64_t PANEL = 32768;  // database rows per GEMM panel
constexpr int KMAX = 1024;

__device__ __forceinline__ bool better(float v, long long i, float bv, long long bi) {
  return v > bv || (v == bv && i < bi);
}
__global__ __launch_bounds__(256) void rownorm_sq_kernel(const float* __restrict__ x, int64_t dim,
                                                         float* __restrict__ out, const int* __restrict__ gate) {
  __shared__ float red[4];
  if (gate_closed(gate)) return;
  const float* r = x + (int64_t)blockIdx.x * dim;
  float ss = 0.f;
  for (int64_t i = threadIdx.x; i < dim; i += 256) ss += r[i] * r[i];
  ss = wave_sum(ss);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// One block per query.  Running list (best first) lives in run_v/run_i [nq,k]; `first` != 0
// initialises it to (-inf, -1).  metric 1: candidate value = -(qn + dn - 2 ip).
// dnorm != nullptr: the database rows were scored RAW and are normalised here, score / dnorm[col]
// (dnorm = max(||row||, 1e-12): F.normalize of the row, reference utilities.py:436, without a normalised copy).
//
// Threshold filter + rank selection.  The k-th entry of the running list bounds everything that can still enter it, so
// the block streams the score row in steps of TILE columns and keeps only the candidates that beat that entry (value,
// then lower index) in an LDS buffer -- for a list that has seen n columns about k / n of a step.  When the buffer could
// overflow on the next step, and at the end, the best k of list + buffer are found WITHOUT selection rounds: every entry
// carries a 64-bit key whose unsigned order is the retrieval order,
//     key = order-preserving bits of the value | tie field (list entries 0xFFFF, candidates 0x7FFF - column) | ~slot,
// (list entries come from earlier columns than any buffered candidate, and the list is sorted: on equal values a list
// entry precedes a candidate and a lower slot precedes a higher one -- exactly "ties -> lower database index"), each
// thread counts the keys above those of its own entries while the whole block reads the key array as LDS broadcasts, and an
// entry of rank r < k goes to position r of the new list.  Keys are unique (the slot), so ranks are; the buffer is filled
// through an LDS counter in a varying order, which the ranks do not depend on: the result is deterministic.
__device__ __forceinline__ unsigned ord_bits(float v) {
  v += 0.0f;                                               // -0 -> +0: equal under the float comparison of the filter
  const unsigned u = __float_as_uint(v);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float ord_value(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}
__device__ __forceinline__ unsigned long long merge_key(float v, unsigned tie, int slot) {
  return ((unsigned long long)ord_bits(v) << 32) | ((unsigned long long)(tie & 0xffffu) << 16) | (unsigned long long)(0xffff - slot);
}

// rank of every entry among the `tot` keys (number of keys above it); entries of rank < k go to position rank of the new
// list.  U of a thread's entries share one pass over the key array, which every lane reads at the same address (broadcast).
template <int U>
__device__ __forceinline__ void rank_entries(const unsigned long long* key, const long long* ei, float* nv, long long* ni,
                                             int tot, int tot2, int k) {
  const int tid = threadIdx.x;
  for (int e0 = tid; e0 < tot; e0 += 256 * U) {
    unsigned long long mine[U];
    int rank[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = e0 + 256 * u;
      mine[u] = e < tot ? key[e] : ~0ull;                  // no entry: nothing ranks above it, and it is never written
      rank[u] = 0;
    }
    for (int j = 0; j < tot2; j += 2) {
      const ulonglong2 kk = *reinterpret_cast<const ulonglong2*>(&key[j]);
#pragma unroll
      for (int u = 0; u < U; ++u) rank[u] += (kk.x > mine[u]) + (kk.y > mine[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = e0 + 256 * u;
      if (e < tot && rank[u] < k) {
        nv[rank[u]] = ord_value((unsigned)(mine[u] >> 32));
        ni[rank[u]] = ei[e];
      }
    }
  }
}

__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ scores, int64_t ld, int64_t ncols,
                                                         int64_t col_base, int k, int metric,
                                                         const float* __restrict__ qn, const float* __restrict__ dn,
                                                         const float* __restrict__ dnorm,
                                                         float* __restrict__ run_v, long long* __restrict__ run_i,
                                                         int first, const int* __restrict__ gate) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  if (gate_closed(gate)) return;
  // slots [0, k): running list, best first; slots [k, k + CAP): buffered candidates
  unsigned long long* key = reinterpret_cast<unsigned long long*>(smem_raw);          // [k2 + CAP], k2 = k rounded up to even
  const int k2 = (k + 1) & ~1;
  long long* ei = reinterpret_cast<long long*>(key + k2 + CAP);                        // [k2 + CAP] global indices
  float* nv = reinterpret_cast<float*>(ei + k2 + CAP);                                 // [k] list under construction
  long long* ni = reinterpret_cast<long long*>(nv + k2);
  __shared__ int n_s;
  __shared__ float thr_v;
  __shared__ long long thr_i;

  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  const float* srow = scores + q * ld;
  const float qq = metric ? qn[q] : 0.f;

  for (int i = tid; i < k; i += 256) {
    const float v = first ? -INFINITY : run_v[q * k + i];
    key[i] = merge_key(v, 0xffffu, i);
    ei[i] = first ? -1 : run_i[q * k + i];
  }
  if (tid == 0) {
    n_s = 0;
    thr_v = first ? -INFINITY : run_v[q * k + k - 1];
    thr_i = first ? -1 : run_i[q * k + k - 1];
  }
  __syncthreads();

  // best k of slots [0, k + n_s) -> list; called by the whole block after a barrier
  auto select = [&]() {
    const int tot = k + n_s;
    const int tot2 = (tot + 1) & ~1;
    if (tid == 0 && (tot & 1)) key[tot] = 0;               // pad to a whole 16-byte read: below every real key
    __syncthreads();
    if (tot <= 256) rank_entries<1>(key, ei, nv, ni, tot, tot2, k);
    else if (tot <= 512) rank_entries<2>(key, ei, nv, ni, tot, tot2, k);
    else rank_entries<4>(key, ei, nv, ni, tot, tot2, k);
    __syncthreads();
    for (int i = tid; i < k; i += 256) {
      key[i] = merge_key(nv[i], 0xffffu, i);
      ei[i] = ni[i];
    }
    if (tid == 0) {
      thr_v = nv[k - 1];
      thr_i = ni[k - 1];
      n_s = 0;
    }
    __syncthreads();
  };

  int64_t c0 = 0;
  // block-uniform copy of n_s: read after the post-scatter barrier of a step, and nobody appends again before the
  // pre-scatter barrier of the next step, which every thread reaches only after its own read -- so all threads take the
  // same branch below (a decision made from n_s itself could see a faster wave's atomicAdd of the next step)
  int n_now = 0;
  while (c0 < ncols) {
    const int step = (first && c0 == 0) ? BOOT : TILE;    // the first step only seeds the threshold
    if (n_now + step > CAP) {
      select();
      n_now = 0;
    }
    const float tv = thr_v;
    const long long ti = thr_i;
    float v[TILE / 256];
#pragma unroll
    for (int j = 0; j < TILE / 256; ++j) {                // all loads of the step first
      const int64_t c = c0 + tid + 256 * j;
      v[j] = -INFINITY;
      if (256 * j < step && c < ncols) {
        v[j] = srow[c];
        if (dnorm) v[j] = v[j] / dnorm[c];
        if (metric) v[j] = -((qq + dn[c]) - 2.0f * v[j]);
      }
    }
    __syncthreads();                                      // every thread has read n_s / the threshold of this step
#pragma unroll
    for (int j = 0; j < TILE / 256; ++j) {
      const int64_t c = c0 + tid + 256 * j;
      const long long gi = col_base + c;
      if (256 * j < step && c < ncols && better(v[j], gi, tv, ti)) {
        const int slot = k + atomicAdd(&n_s, 1);
        key[slot] = merge_key(v[j], 0x7fffu - (unsigned)c, slot);
        ei[slot] = gi;
      }
    }
    __syncthreads();
    if (first && c0 == 0) {
      select();                                           // the seed columns become the first list: a real threshold from here on
      n_now = 0;
    } else {
      n_now = n_s;
    }
    c0 += step;
  }
  select();
  for (int i = tid; i < k; i += 256) {
    run_v[q * k + i] = ord_value((unsigned)(key[i] >> 32));
    run_i[q * k + i] = ei[i];
  }
}

// raw sums of squares -> dnorm = max(sqrt(ss), 1e-12) (F.normalize's denominator) and, for the L2 metric, the squared
// norm of the normalised row dn = ss / dnorm^2
__global__ void dbnorm_kernel(const float* __restrict__ ss, int64_t n, float* __restrict__ dnorm, float* __restrict__ dn,
                              const int* __restrict__ gate) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || gate_closed(gate)) return;
  const float d = clamp_min_nan(sqrtf(ss[i]), 1e-12f);
  dnorm[i] = d;
  dn[i] = (ss[i] / d) / d;
}

// few-query path: sum the split-K slices of C_s[row, 0..63] (and of the row sums of squares) in slice order and write
// the [nq, ncols] score panel the merge kernel reads, plus the raw sum of squares of every database row
__global__ __launch_bounds__(256) void splitk_combine_kernel(const float* __restrict__ part, const float* __restrict__ rsq_part,
                                                             int S, int64_t rows, int nq, float* __restrict__ scores,
                                                             float* __restrict__ ss) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= rows) return;
  float acc[64];
#pragma unroll
  for (int q = 0; q < 64; ++q) acc[q] = 0.f;
  float r = 0.f;
  for (int s = 0; s < S; ++s) {
    const f32x4* pr = reinterpret_cast<const f32x4*>(part + ((int64_t)s * rows + j) * 64);
#pragma unroll
    for (int q4 = 0; q4 < 16; ++q4) {
      const f32x4 v = pr[q4];
      acc[4 * q4] += v[0]; acc[4 * q4 + 1] += v[1]; acc[4 * q4 + 2] += v[2]; acc[4 * q4 + 3] += v[3];
    }
    r += rsq_part[(int64_t)s * rows + j];
  }
  ss[j] = r;
#pragma unroll
  for (int q = 0; q < 64; ++q)
    if (q < nq) scores[(int64_t)q * rows + j] = acc[q];
}

// metric 1: stored values are negated squared distances -> flip sign; padding -> +inf
__global__ void topk_finish_kernel(float* __restrict__ v, const long long* __restrict__ idx, int64_t n, int metric) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (metric) v[i] = idx[i] < 0 ? INFINITY : -v[i];
}

// ANYLOC_TOPK_NO_WAIT, a few overflowed queries (plan[]: common.hpp, screen_overflow_plan).  Gather: workgroup j copies query
// plan[4 + j] into row j of the side batch, or zeroes the row when there is none.  Scatter: the side batch's list j goes to row
// plan[4 + j] of the caller's lists.  Both behind plan[1], the gate of the side batch.
__global__ __launch_bounds__(256) void side_gather_kernel(const float* __restrict__ queries, int64_t dim, const int* __restrict__ plan,
                                                          float* __restrict__ rows) {
  if (plan[1] == 0) return;
  const int q = plan[4 + blockIdx.x];
  float* dst = rows + (int64_t)blockIdx.x * dim;
  for (int64_t i = threadIdx.x; i < dim; i += 256) dst[i] = q >= 0 ? queries[(int64_t)q * dim + i] : 0.f;
}
__global__ __launch_bounds__(64) void side_scatter_kernel(const float* __restrict__ side_v, const long long* __restrict__ side_i, int k,
                                                          const int* __restrict__ plan, float* __restrict__ run_v,
                                                          long long* __restrict__ run_i) {
  if (plan[1] == 0 || (int)blockIdx.x >= plan[0]) return;
  const int64_t q = plan[4 + blockIdx.x], j = blockIdx.x;
  for (int i = threadIdx.x; i < k; i += 64) {
    run_v[q * k + i] = side_v[j * k + i];
    run_i[q * k + i] = side_i[j * k + i];
  }
}

constexpr int SPLITK_MAX = 16;            // few-query path: K slices of the split-K launch, at most
// number of K slices: a divisor of dim/32 that fills the 512 resident workgroups (2 per CU) best, slices >= 1024 long
int choose_ksplit(int64_t rows, int64_t dim) {
  const int64_t tiles = (rows + 127) / 128, kb = dim / 32;
  int best = 1;
  double best_u = 0.0;
  for (int s = 1; s <= SPLITK_MAX; ++s) {
    if (kb % s != 0 || dim / s < 1024) continue;
    const int64_t blocks = tiles * s;
    const double u = (double)blocks / (double)((blocks + 511) / 512 * 512) * (blocks >= 256 ? 1.0 : (double)blocks / 256.0);
    if (u > best_u + 1e-9) { best_u = u; best = s; }
  }
  return best;
}

// fp16 panels (gemm_h3.hip: three fp16 matrix-core products per k-step of row-scaled 22-bit operands, fp32 accumulate).  Quantising
// a panel (split_h2_wide) is two reads + one write of it, a few % of its GEMM; the rows' sums of squares for F.normalize / L2 come
// out of the same pass.  An operand image must stay inside 2 GiB of buffer addressing: rows <= (2^31 - 1) / (64 * dim / 16).
constexpr int64_t H3_PANEL = 8192;
int64_t h3_rows_limit(int64_t dim) { return dim > 0 ? ((1ll << 31) - 1) / (4 * dim) / 256 * 256 : 0; }
// A 49 152-long contraction in ONE fp32 accumulator takes ~9 000 rounded additions: 4e-6 on a score of 1.  Cut into chunks of 8192 k
// (one launch each, the later ones adding into the panel) the error is that of ~1 500 additions plus six: 5e-7 -- the chunked summation
// of the fp32-MFMA path (gemm_f32.hip, ABL bit 5) at the price of re-reading and re-writing the score panel per chunk (3 % of the GEMM time).
constexpr int64_t SCORE_KC16 = 512;       // k-blocks of 16 per accumulated chunk: exact scores
constexpr int64_t SCREEN_KC16 = 1536;     // ... leading-plane scores (the accumulation term of the screening bound)

// Screened search (scores_screen.hip)
// (SCREEN_CMAX, candidates per query and column range, and SCREEN_RESCORE_COLS, the widest re-scoring slice: common.hpp)
constexpr int SCREEN_KMAX = 128;
constexpr int64_t SCREEN_COLS = 131072;   // database columns per range, at most (a range is a whole number of panels)
constexpr size_t SCREEN_SBUF_MAX = 12ull << 30;

enum { PATH_F32 = 0, PATH_FEWQ = 1, PATH_H3 = 2 };   // the values anyloc_topk_path answers
struct TopkPlan {
  int64_t nq, ndb, dim, k;
  bool indexed;                    // the database side is a prepared index: fp16 panels at every query count
  int path;
  int64_t panel, q_chunk;          // database rows per score panel; fp16 panels: queries per operand image
  int64_t sc_cols;                 // database columns per screened range; 0: no screened search for this shape
  int64_t rs_cols;                 // ... columns per slice of its re-scoring kernels; 0: the whole row in one, on the single-slice kernels
  int fewq;                        // few-query arithmetic: 2 = two fp16 planes, 1 = three bf16 planes, 0 = fp32 MFMA
  bool qdma;                       // ... on fp16 planes: the queries are pre-split once per call
};
// Option topk_h3: -1 (default) = where it pays (>= 256 queries, dim >= 1024, >= 2048 rows), 0 = never, 1 = wherever the shape
// allows (tests).  Option topk_screen: 0 = never, 1 = wherever the shape allows, -1 (default) = where it pays (>= 256 queries
// against >= 16 384 rows of 4096 .. 49 152 columns -- wider rows screen under 1 only: their panels are short, 3 840 rows at 131 072
// columns, the 256 x 256 tiles of gemm_screen then fill a quarter of the chip and 1 000 x 20 000 x 131 072 took 28.1 ms screened
// against 24.7 ms, profiles/wide_screen_timing.md); it serves the fp16 panels' shapes with k <= 128 and a score buffer of at most 12 GiB
// (fewer columns per range for more queries).  A range is a whole number of panels -- the indexed db_panel serves whole panels,
// and from 65 536 columns on the panel (h3_rows_limit) no longer divides SCREEN_COLS.  Option topk_rescore_cols: the columns per
// slice of the re-scoring kernels, 0 (default) = SCREEN_RESCORE_COLS, where narrower rows keep the single-slice kernels; a set value
// (a multiple of 4096) sends every width through the sliced ones.  It changes no size.
TopkPlan topk_plan(int64_t nq, int64_t ndb, int64_t dim, int64_t k, bool indexed) {
  const int64_t h3_mode = option(OPT_TOPK_H3), screen_mode = option(OPT_TOPK_SCREEN), limit = h3_rows_limit(dim);
  const int64_t rescore_cols = option(OPT_TOPK_RESCORE_COLS);
  TopkPlan p{nq, ndb, dim, k, indexed};
  p.fewq = (int)option(OPT_TOPK_FEWQ_X6);
  p.qdma = option(OPT_TOPK_FEWQ_QDMA) != 0;
  const bool h3 = indexed || (h3_mode != 0 && nq > 64 && dim % 16 == 0 && limit >= 256 &&
                              (h3_mode > 0 || (nq >= 256 && dim >= 1024 && ndb >= 2048)));
  p.path = h3 ? PATH_H3 : nq <= 64 && dim % 32 == 0 && dim >= 4096 ? PATH_FEWQ : PATH_F32;
  p.panel = h3 ? std::min(H3_PANEL, limit) : PANEL;
  p.q_chunk = std::max<int64_t>(1, h3 ? std::min(nq, limit) : nq);
  if (h3 && screen_mode != 0 && k >= 1 && k <= SCREEN_KMAX && screen_rescore_supported(dim) && nq > 0 && ndb > 0 &&
      (screen_mode > 0 || (nq >= 256 && ndb >= 16384 && dim >= 4096 && dim <= SCREEN_RESCORE_COLS))) {
    const int64_t fit = (int64_t)(SCREEN_SBUF_MAX / 4) / nq / p.panel * p.panel;
    const int64_t cols = std::min(std::min(SCREEN_COLS / p.panel * p.panel, cdiv(ndb, p.panel) * p.panel), fit);
    p.sc_cols = cols >= p.panel ? cols : 0;
    p.rs_cols = rescore_cols > 0 ? std::min(rescore_cols, SCREEN_RESCORE_COLS) : dim > SCREEN_RESCORE_COLS ? SCREEN_RESCORE_COLS : 0;
  }
  return p;
}

struct TopkWs {
  // screened search: leading-plane scores [nq, sc_cols], screened running lists, per-query margin, candidates, their re-scored values
  float *sbuf, *scr_v, *margin, *cand_v, *rho_q, *rho_d, *resid;
  long long* scr_i;
  int *cand, *count, *overflow;
  // ANYLOC_TOPK_NO_WAIT: per-query overflow marks, the device's plan, and the side batch of the overflowed queries -- their rows
  // and lists; its operand image, scales, norms and score panel are those of the full fallback, which never runs in the same call
  int *over_q, *plan;
  float *side_rows, *side_v;
  long long* side_i;
  float *scores, *qn, *dn, *dss, *dnorm, *part, *rsq_part;
  unsigned char *qimg, *dimg;      // h3 path: operand images of the queries (per chunk of q_chunk rows) and of one panel
  float *qinv, *dinv;              // ... and their row scales
  size_t bytes;
};
TopkWs carve(void* ws, size_t cap, const TopkPlan& p) {
  Arena a(ws, cap);
  TopkWs w;
  const bool h3 = p.path == PATH_H3, few = p.path == PATH_FEWQ, own_db = h3 && !p.indexed, sc = p.sc_cols > 0;
  const int64_t nq = p.nq, k = p.k, ndb1 = std::max<int64_t>(p.ndb, 1), panel = std::min(p.panel, ndb1);
  w.scores = a.take<float>(std::max<int64_t>(nq, 1) * panel);
  // (few-query fp16 path: the queries' pre-split planes, 10 KiB per 32-k slab)
  w.qimg = a.take<unsigned char>(h3 ? (size_t)cdiv(nq, p.q_chunk) * h2_bytes(p.q_chunk, p.dim) : few ? fewq_query_image_bytes(p.dim) : 1);
  w.dimg = a.take<unsigned char>(own_db ? h2_bytes(panel, p.dim) : 1);
  w.qinv = a.take<float>(h3 ? nq : 64);                  // (few-query fp16 path: the <= 64 queries' row scales)
  w.dinv = a.take<float>(own_db ? panel : 1);
  w.qn = a.take<float>(std::max<int64_t>(nq, 1));
  w.dn = a.take<float>(ndb1);
  w.dss = a.take<float>(ndb1);
  w.dnorm = a.take<float>(ndb1);
  w.part = a.take<float>(few ? (size_t)SPLITK_MAX * panel * 64 : 1);
  w.rsq_part = a.take<float>(few ? (size_t)SPLITK_MAX * panel : 1);
  w.sbuf = a.take<float>(sc ? (size_t)nq * p.sc_cols : 1);
  w.scr_v = a.take<float>(sc ? (size_t)nq * k : 1);
  w.scr_i = a.take<long long>(sc ? (size_t)nq * k : 1);
  w.margin = a.take<float>(sc ? (size_t)nq : 1);
  w.cand = a.take<int>(sc ? (size_t)nq * SCREEN_CMAX : 1);
  w.cand_v = a.take<float>(sc ? (size_t)nq * SCREEN_CMAX : 1);
  w.count = a.take<int>(sc ? (size_t)nq : 1);
  w.rho_q = a.take<float>(sc ? (size_t)nq : 1);
  w.rho_d = a.take<float>(sc && !p.indexed ? (size_t)ndb1 : 1);
  w.resid = a.take<float>(sc && !p.indexed ? (size_t)panel : 1);
  w.overflow = a.take<int>(4);                            // [0] overflow flag, [1] bits of the largest database rho, [2] of the largest raw sum of squares
  // (the size functions take no flags: a screening shape carries the side batch whether or not the call asks for it)
  const int64_t side = std::min<int64_t>(nq, SCREEN_SIDE_Q);
  w.over_q = a.take<int>(sc ? (size_t)nq : 0);             // (a shape that does not screen needs the bytes it needed before)
  w.plan = a.take<int>(sc ? SCREEN_PLAN_INTS : 0);
  w.side_rows = a.take<float>(sc ? (size_t)side * p.dim : 0);
  w.side_v = a.take<float>(sc ? (size_t)side * k : 0);
  w.side_i = a.take<long long>(sc ? (size_t)side * k : 0);
  w.bytes = a.off;
  return w;
}

// A prepared database (anyloc_topk_index_build: faiss' index.add): per panel of index_panel(dim) rows the two-plane fp16 image
// the score GEMM reads, then the rows' 2^-e and their raw sums of squares.  Layout inside the caller's buffer:
//   [n_panels][align256(h2_bytes(panel, dim))] images (a shorter last panel: an image of its own row count at its slot)
//   [ndb] float 2^-e      [ndb] float sum of squares      [ndb] float relative residual norm (ABI 9)
int64_t index_panel(int64_t dim) { return topk_plan(0, 0, dim, 0, true).panel; }
bool index_supported(int64_t ndb, int64_t dim) { return ndb > 0 && dim % 16 == 0 && dim >= 16 && h3_rows_limit(dim) >= 256; }
struct IndexView {
  unsigned char* img;
  float *dinv, *dss, *drho;        // drho (ABI 9): |row - leading plane| / |row|, the screened search's bound (scores_screen.hip)
  int64_t panel;
  size_t slot, bytes;
};
IndexView index_view(void* p, int64_t ndb, int64_t dim) {
  IndexView v;
  v.panel = index_panel(dim);
  const int64_t np = (ndb + v.panel - 1) / v.panel;
  v.slot = align_up(h2_bytes(v.panel, dim), 256);
  v.img = static_cast<unsigned char*>(p);
  v.dinv = reinterpret_cast<float*>(v.img + (size_t)np * v.slot);
  v.dss = v.dinv + align_up((size_t)ndb, 64);
  v.drho = v.dss + align_up((size_t)ndb, 64);
  v.bytes = (size_t)np * v.slot + 3 * align_up((size_t)ndb, 64) * sizeof(float);
  return v;
}

// One search: the caller's arguments, the plan, the carved workspace and the index, for the steps below
struct TopkCall {
  const float *queries, *db;       // db == nullptr: a prepared index without its fp32 rows
  int metric;
  bool norm_db, rescore_planes, no_wait;
  int64_t index_base;
  float* dist;
  long long* idx;
  hipStream_t stream;
  TopkPlan p;
  TopkWs w;
  IndexView iv;                    // of the prepared index, if any
  const int* gate;                 // nullptr, or the device word that closes every launch of this search (device_fallback)
};

int launch_rownorm(const float* x, int64_t rows, int64_t dim, float* out, const char* what, hipStream_t stream, const int* gate) {
  hipLaunchKernelGGL(rownorm_sq_kernel, dim3((unsigned)rows), dim3(256), 0, stream, x, dim, out, gate);
  return launch_status(what);
}
int launch_dbnorm(const float* ss, int64_t n, float* dnorm, float* dn, hipStream_t stream, const int* gate) {
  hipLaunchKernelGGL(dbnorm_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, stream, ss, n, dnorm, dn, gate);
  return launch_status("dbnorm_kernel");
}
// merges score columns [col0, col0 + ncols) into the lists run_v / run_i; no columns: an empty database's padding list, not profiled
int launch_merge(const TopkCall& c, const float* scores, int64_t ld, int64_t ncols, int64_t col0, const float* dn, const float* dnorm,
                 float* run_v, long long* run_i, int first) {
  static_assert(PANEL <= 0x8000 && H3_PANEL <= PANEL && CAP + KMAX + 2 <= 0xffff, "merge keys hold the column in 15 bits and the slot in 16");
  const size_t k2 = (size_t)((c.p.k + 1) & ~1ll), lds = 16 * (k2 + CAP) + 12 * k2 + 16;   // 37 KiB at k = 20: four blocks per CU
  // k = 1023 and 1024 ask for 65 552 bytes (k = 1022: 65 496), 16 more than the default limit of dynamic LDS
  constexpr int LDS_KMAX = 16 * (KMAX + CAP) + 12 * KMAX + 16;
  static_assert(KMAX % 2 == 0 && LDS_KMAX > 65536, "the merge kernel's dynamic LDS at the largest k is above the default limit");
  static DynLds dyn_lds_once;
  ANYLOC_TRY(ensure_dyn_lds(dyn_lds_once, reinterpret_cast<const void*>(topk_merge_kernel), LDS_KMAX));
  std::optional<ProfScope> prof;
  if (ncols > 0) prof.emplace("topk_merge", c.stream, 0.0, 4.0 * c.p.nq * ncols);
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)c.p.nq), dim3(256), lds, c.stream, scores, ld, ncols, c.index_base + col0,
                     (int)c.p.k, c.metric, c.w.qn, dn, dnorm, run_v, run_i, first, c.gate);
  return launch_status("topk_merge_kernel");
}

// fp16 panels: f(first query, queries, their operand image) for every chunk of q_chunk queries
template <class F> int each_query_chunk(const TopkCall& c, F f) {
  for (int64_t q0 = 0, i = 0; q0 < c.p.nq; q0 += c.p.q_chunk, ++i)
    ANYLOC_TRY(f(q0, std::min(c.p.q_chunk, c.p.nq - q0), c.w.qimg + i * h2_bytes(c.p.q_chunk, c.p.dim)));
  return ANYLOC_OK;
}

// A database panel as the score GEMM's operand: image, row scales, the rows' raw sums of squares (where the call uses them), and,
// normalising, its dnorm / dn.  Source: the slot of the prepared index; or the rows quantised now (split_h2_wide); or, screening on
// the rows, their leading plane alone (split_h1_wide), whose residual norms -- the bound -- come out of the quantiser itself.
struct DbPanel { const unsigned char* img; const float *inv, *ss; };
int db_panel(const TopkCall& c, int64_t c0, int64_t pc, bool leading_plane, DbPanel& d) {
  const TopkWs& w = c.w;
  const int64_t dim = c.p.dim;
  if (c.p.indexed) {
    d = {c.iv.img + (size_t)(c0 / c.iv.panel) * c.iv.slot, c.iv.dinv + c0, c.iv.dss + c0};
  } else if (leading_plane) {
    d = {w.dimg, w.dinv, w.dss + c0};
    ANYLOC_HIP(hipMemsetAsync(w.resid, 0, (size_t)pc * sizeof(float), c.stream));
    ANYLOC_TRY(split_h1_wide(c.db + c0 * dim, dim, pc, dim, w.dimg, w.dinv, w.dss + c0, w.resid, c.stream));
    ANYLOC_TRY(screen_rho_from_resid(w.resid, w.dinv, w.dss + c0, pc, w.rho_d + c0, reinterpret_cast<unsigned*>(w.overflow + 1), c.stream));
  } else {   // the sums of squares are the L2 term as they are, or, normalising, what dnorm / dn are made of
    float* ss = c.norm_db ? w.dss + c0 : c.metric == 1 ? w.dn + c0 : nullptr;
    d = {w.dimg, w.dinv, ss};
    ANYLOC_TRY(split_h2_wide(c.db + c0 * dim, dim, pc, dim, w.dimg, w.dinv, ss, c.stream, c.gate));
  }
  return c.norm_db ? launch_dbnorm(d.ss, pc, w.dnorm + c0, w.dn + c0, c.stream, c.gate) : ANYLOC_OK;
}

// scores of all queries against one panel on the fp16 planes -> C[nq, ldc], k-chunk by k-chunk (the later ones add):
// exact = the two-term GEMM in chunks of SCORE_KC16 k-blocks, otherwise the leading planes alone in chunks of SCREEN_KC16
int score_panel(const TopkCall& c, const DbPanel& d, int64_t pc, bool exact, float* C, int64_t ldc) {
  const int64_t K16 = c.p.dim / 16, KC16 = exact ? SCORE_KC16 : SCREEN_KC16;
  return each_query_chunk(c, [&](int64_t q0, int64_t qc, const unsigned char* qimg) {
    for (int64_t kb0 = 0; kb0 < K16; kb0 += KC16) {
      H3Problem h{};
      h.A2 = qimg + kb0 * (2 * qc * 32); h.RA = qc; h.a_inv = c.w.qinv + q0;
      h.W2 = d.img + kb0 * (2 * pc * 32); h.RW = pc; h.w_inv = d.inv;
      h.C = C + q0 * ldc; h.ldc = ldc;
      h.M = qc; h.N = pc; h.K16 = (int)std::min<int64_t>(KC16, K16 - kb0);
      h.accumulate = kb0 > 0; h.gate = exact ? c.gate : nullptr; h.tag = exact ? "topk_scores_gemm" : "topk_screen_gemm";
      ANYLOC_TRY(exact ? gemm_h3(h, EPI_STORE, c.stream) : gemm_screen(h, c.stream));
    }
    return (int)ANYLOC_OK;
  });
}

// what both searches start from: the queries' squared norms (L2, and the screening bound), the database rows' norms where no
// scoring pass delivers them (fp32 panels), and the queries' operand images, built once per call
int prologue(const TopkCall& c, bool screen) {
  const TopkWs& w = c.w;
  const int64_t nq = c.p.nq, ndb = c.p.ndb, dim = c.p.dim;
  if (c.metric == 1 || screen) ANYLOC_TRY(launch_rownorm(c.queries, nq, dim, w.qn, "rownorm_sq_kernel(q)", c.stream, c.gate));
  if ((c.metric == 1 || c.norm_db) && c.p.path == PATH_F32) {
    ProfScope prof("topk_db_norms", c.stream, 2.0 * ndb * dim, 4.0 * ndb * dim);
    float* ss = c.norm_db ? w.dss : w.dn;
    for (int64_t r0 = 0; r0 < ndb; r0 += (1ll << 30))
      ANYLOC_TRY(launch_rownorm(c.db + r0 * dim, std::min<int64_t>(1ll << 30, ndb - r0), dim, ss + r0, "rownorm_sq_kernel(db)", c.stream, c.gate));
    if (c.norm_db && ndb > 0) ANYLOC_TRY(launch_dbnorm(w.dss, ndb, w.dnorm, w.dn, c.stream, c.gate));
  }
  if (ndb == 0) return ANYLOC_OK;
  if (c.p.path == PATH_H3) {
    ANYLOC_TRY(each_query_chunk(c, [&](int64_t q0, int64_t qc, unsigned char* qimg) {
      return split_h2_wide(c.queries + q0 * dim, dim, qc, dim, qimg, w.qinv + q0, nullptr, c.stream, c.gate);
    }));
  } else if (c.p.path == PATH_FEWQ && c.p.fewq == 2) {   // few queries on fp16 planes: their row scales and, pre-split, their planes
    ANYLOC_TRY(row_scales_h2(c.queries, dim, nq, dim, w.qinv, nullptr, c.stream));
    if (c.p.qdma) ANYLOC_TRY(fewq_query_image(c.queries, dim, nq, w.qinv, dim, w.qimg, c.stream));
  }
  return ANYLOC_OK;
}

// every panel scored exactly and merged into the caller's lists (values still in merge order: topk_impl finishes them)
int panel_search(const TopkCall& c) {
  const TopkWs& w = c.w;
  const int64_t nq = c.p.nq, ndb = c.p.ndb, dim = c.p.dim;
  if (ndb == 0) ANYLOC_TRY(launch_merge(c, w.scores, 0, 0, 0, w.dn, nullptr, c.dist, c.idx, 1));   // nothing to search: the padding list
  for (int64_t c0 = 0; c0 < ndb; c0 += c.p.panel) {
    const int64_t pc = std::min<int64_t>(c.p.panel, ndb - c0);
    const float* dn = w.dn + c0;                            // the merge kernel's squared-norm term of the panel's rows (L2)
    if (c.p.path == PATH_H3) {
      DbPanel d;
      ANYLOC_TRY(db_panel(c, c0, pc, false, d));
      if (!c.norm_db) dn = d.ss;
      ANYLOC_TRY(score_panel(c, d, pc, true, w.scores, pc));
    } else if (c.p.path == PATH_FEWQ) {
      // K cut into slices: enough workgroups to stream the panel at HBM rate; the rows' sums of squares come out of the same pass
      const int S = choose_ksplit(pc, dim);
      const float* rows = c.db + c0 * dim;
      float* ss = (c.norm_db ? w.dss : w.dn) + c0;
      if (c.p.fewq == 2) {
        ANYLOC_TRY(scores_fewq_h3(rows, dim, pc, c.queries, dim, nq, w.qinv, c.p.qdma ? w.qimg : nullptr, dim / S, S, w.part, w.rsq_part, c.stream));
      } else if (c.p.fewq != 0) {
        ANYLOC_TRY(scores_fewq_x6(rows, dim, pc, c.queries, dim, nq, dim / S, S, w.part, w.rsq_part, c.stream));
      } else {
        GemmProblem g{};
        g.A = rows; g.lda = dim; g.W = c.queries; g.ldw = dim;
        g.C = w.part; g.ldc = 64; g.ksplit = S; g.c_split_stride = pc * 64; g.rowsq = w.rsq_part;
        g.M = pc; g.N = nq; g.K = dim / S; g.tag = "topk_scores_gemm";
        ANYLOC_TRY(gemm_nt_splitk(g, c.stream));
      }
      {
        ProfScope prof("topk_combine", c.stream, (double)S * pc * 64, 4.0 * ((double)S * pc * 65 + (double)nq * pc));
        hipLaunchKernelGGL(splitk_combine_kernel, dim3((unsigned)cdiv(pc, 256)), dim3(256), 0, c.stream, w.part, w.rsq_part, S, pc,
                           (int)nq, w.scores, ss);
        ANYLOC_TRY(launch_status("splitk_combine_kernel"));
      }
      if (c.norm_db) ANYLOC_TRY(launch_dbnorm(ss, pc, w.dnorm + c0, w.dn + c0, c.stream, c.gate));
    } else {
      GemmProblem g{};
      g.A = c.queries; g.lda = dim; g.W = c.db + c0 * dim; g.ldw = dim;
      g.C = w.scores; g.ldc = pc;
      g.M = nq; g.N = pc; g.K = dim; g.tag = "topk_scores_gemm";
      ANYLOC_TRY(gemm_nt(g, EPI_STORE, c.stream));
    }
    ANYLOC_TRY(launch_merge(c, w.scores, pc, pc, c0, dn, c.norm_db ? w.dnorm + c0 : nullptr, c.dist, c.idx, c0 == 0));
  }
  return ANYLOC_OK;
}

// The candidates are re-scored from the fp32 rows (a prepared index WITH its rows: anyloc_topk_search_index_rows) or, with
// ANYLOC_TOPK_RESCORE_PLANES, from the two planes of the index (the 22-bit rows it holds, which the unscreened indexed search scores
// too): no rows needed, and none read when they are given.  The bound of a query is one number: its own norm and residual x the
// LARGEST row norm the compared value sees -- 1 with ANYLOC_TOPK_NORMALIZE_DB, the largest raw row norm of the database without it.
// Leaves w.overflow[0] != 0 when some query has more candidates than SCREEN_CMAX inside its bound (near-duplicate rows).
int screened_search(const TopkCall& c) {
  const TopkWs& w = c.w;
  const int64_t nq = c.p.nq, ndb = c.p.ndb, dim = c.p.dim, K16 = dim / 16;
  ANYLOC_HIP(hipMemsetAsync(w.overflow, 0, 3 * sizeof(int), c.stream));
  if (c.no_wait) ANYLOC_HIP(hipMemsetAsync(w.over_q, 0, (size_t)nq * sizeof(int), c.stream));
  unsigned* rho_max = reinterpret_cast<unsigned*>(w.overflow + 1);
  unsigned* ss_max = reinterpret_cast<unsigned*>(w.overflow + 2);   // bits of the largest raw sum of squares (searches without NORMALIZE_DB)
  // the queries' relative residual norms, from the residual planes of their images
  ANYLOC_TRY(each_query_chunk(c, [&](int64_t q0, int64_t qc, const unsigned char* qimg) {
    return screen_resid(qimg, qc, (int)K16, qc, w.qinv + q0, w.qn + q0, w.rho_q + q0, nullptr, c.stream);
  }));
  for (int64_t s0 = 0; s0 < ndb; s0 += c.p.sc_cols) {
    const int64_t sn = std::min<int64_t>(c.p.sc_cols, ndb - s0);
    const float* dnorm_s = c.norm_db ? w.dnorm + s0 : nullptr;      // the divisors of the compared value, or none
    for (int64_t c0 = s0; c0 < s0 + sn; c0 += c.p.panel) {
      const int64_t pc = std::min<int64_t>(c.p.panel, s0 + sn - c0);
      DbPanel d;
      ANYLOC_TRY(db_panel(c, c0, pc, true, d));
      if (!c.norm_db) {
        // raw rows: the L2 term is the raw sum of squares; the bound scales with the largest raw norm seen so far
        ANYLOC_HIP(hipMemcpyAsync(w.dn + c0, d.ss, (size_t)pc * sizeof(float), hipMemcpyDeviceToDevice, c.stream));
        ANYLOC_TRY(screen_rho_max(d.ss, pc, ss_max, c.stream));
      }
      ANYLOC_TRY(score_panel(c, d, pc, false, w.sbuf + (c0 - s0), sn));
      ANYLOC_TRY(launch_merge(c, w.sbuf + (c0 - s0), sn, pc, c0, w.dn + c0, c.norm_db ? w.dnorm + c0 : nullptr, w.scr_v, w.scr_i, c0 == s0));
    }
    if (c.p.indexed) ANYLOC_TRY(screen_rho_max(c.iv.drho + s0, sn, rho_max, c.stream));
    ANYLOC_TRY(screen_margins(w.qn, w.rho_q, rho_max, c.norm_db ? nullptr : ss_max, nq, c.metric,
                              screen_accum((int)std::min(SCREEN_KC16, K16), (int)cdiv(K16, SCREEN_KC16)), w.margin, c.stream));
    ANYLOC_TRY(screen_compact(w.sbuf, sn, sn, nq, (int)c.p.k, c.metric, w.qn, w.dn + s0, dnorm_s, w.scr_v, w.margin, SCREEN_CMAX, w.cand,
                              w.count, w.overflow, c.no_wait ? w.over_q : nullptr, c.stream));
    if (c.rescore_planes)
      ANYLOC_TRY(screen_rescore_planes(c.queries, c.iv.img, c.iv.slot, c.iv.panel, ndb, s0, c.iv.dinv, dim, c.p.rs_cols, nq, SCREEN_CMAX, w.cand,
                                       w.count, c.metric, w.qn, w.dn + s0, dnorm_s, w.cand_v, c.stream));
    else
      ANYLOC_TRY(screen_rescore(c.queries, c.db + s0 * dim, dim, c.p.rs_cols, nq, SCREEN_CMAX, w.cand, w.count, c.metric, w.qn, w.dn + s0,
                                dnorm_s, w.cand_v, c.stream));
    ANYLOC_TRY(screen_select(w.cand, w.cand_v, w.count, SCREEN_CMAX, c.index_base + s0, nq, (int)c.p.k, c.dist,
                             reinterpret_cast<int64_t*>(c.idx), s0 == 0, c.stream));
  }
  return ANYLOC_OK;
}

// ANYLOC_TOPK_NO_WAIT: what topk_impl decides from the overflow flag after a wait, decided on the device.  The host cannot know
// the outcome, so it enqueues BOTH remedies, every launch of each behind a gate of the plan (a closed launch returns at entry):
//   plan[1]  1 .. SCREEN_SIDE_Q queries overflowed: they are gathered into a batch of their own (unused rows zero), searched over
//            the whole database by the unscreened panel search, and their lists scattered over those the screened search left
//            for them; every other query keeps its screened list
//   plan[2]  more: the unscreened panel search for all queries, as after the wait
// The side batch quantises into the query image, scales, norms and score panel of the full search: the gates exclude each other,
// and the screened search is done with them.
int device_fallback(const TopkCall& c) {
  const TopkWs& w = c.w;
  const int side = (int)std::min<int64_t>(c.p.nq, SCREEN_SIDE_Q);
  ANYLOC_TRY(screen_overflow_plan(w.over_q, c.p.nq, side, w.plan, c.stream));
  TopkCall s = c;
  s.queries = w.side_rows; s.dist = w.side_v; s.idx = w.side_i;
  s.p.nq = side; s.p.q_chunk = side;
  s.gate = w.plan + 1;
  hipLaunchKernelGGL(side_gather_kernel, dim3((unsigned)side), dim3(256), 0, c.stream, c.queries, c.p.dim, w.plan, w.side_rows);
  ANYLOC_TRY(launch_status("side_gather_kernel"));
  ANYLOC_TRY(prologue(s, false));
  ANYLOC_TRY(panel_search(s));
  hipLaunchKernelGGL(side_scatter_kernel, dim3((unsigned)side), dim3(64), 0, c.stream, w.side_v, w.side_i, (int)c.p.k, w.plan, c.dist, c.idx);
  ANYLOC_TRY(launch_status("side_scatter_kernel"));
  TopkCall f = c;
  f.gate = w.plan + 2;
  return panel_search(f);
}

// `index` != nullptr: the database side comes from a prepared index (db may be null)
int topk_impl(const float* queries, int64_t nq, const float* db, int64_t ndb, int64_t dim, int64_t k, int metric, unsigned flags,
              int64_t index_base, float* dist, int64_t* idx, void* workspace, size_t workspace_bytes, const void* index, hipStream_t stream) {
  ANYLOC_CHECK_ARG(nq >= 0 && ndb >= 0, "topk: negative size");
  ANYLOC_CHECK_ARG(k >= 1 && k <= KMAX, "topk: k=%lld outside [1,%d]", (long long)k, KMAX);
  if (nq == 0) return ANYLOC_OK;
  ANYLOC_CHECK_ARG(queries && dist && idx, "topk: null pointer");
  ANYLOC_CHECK_ARG(db || ndb == 0 || index, "topk: null database");
  const bool indexed = index != nullptr;
  ANYLOC_CHECK_ARG(metric == 0 || metric == 1, "topk: metric %d", metric);
  ANYLOC_CHECK_ARG(dim >= 4 && dim % 4 == 0, "topk: dim %lld must be a positive multiple of 4", (long long)dim);
  ANYLOC_CHECK_ARG(nq < (1ll << 31), "topk: too many queries");
  // (the score kernels read the rows of one tile -- at most 256, gemm_f32.hip: check_tile_span -- through one 2 GiB buffer
  // descriptor: 256 * dim * 4 < 2^31)
  ANYLOC_CHECK_ARG(dim < (1ll << 21), "topk: dim %lld must be below 2^21", (long long)dim);
  ANYLOC_CHECK_ARG((flags & ~(ANYLOC_TOPK_NORMALIZE_DB | ANYLOC_TOPK_NO_WAIT | (indexed ? ANYLOC_TOPK_RESCORE_PLANES : 0u))) == 0,
                   "topk: unknown flags %u", flags);
  TopkCall c{queries, db, metric, (flags & ANYLOC_TOPK_NORMALIZE_DB) != 0, indexed && (flags & ANYLOC_TOPK_RESCORE_PLANES) != 0,
             (flags & ANYLOC_TOPK_NO_WAIT) != 0, index_base, dist, reinterpret_cast<long long*>(idx), stream, topk_plan(nq, ndb, dim, k, indexed)};
  c.w = carve(workspace, workspace_bytes, c.p);
  if (!workspace || c.w.bytes > workspace_bytes) {
    set_error("topk: workspace %zu < %zu", workspace_bytes, c.w.bytes);
    return ANYLOC_ERR_WORKSPACE;
  }
  if (indexed) c.iv = index_view(const_cast<void*>(index), ndb, dim);
  // whether this call screens: the plan allows it, and there is something to re-score the candidates from
  const bool screen = c.p.sc_cols > 0 && (db != nullptr || c.rescore_planes) && ndb > 0;
  ANYLOC_TRY(prologue(c, screen));
  int overflow = 0;
  if (screen) {
    ANYLOC_TRY(screened_search(c));
    if (c.no_wait) {   // no wait: the device decides (a shape that does not screen never waited)
      ANYLOC_TRY(device_fallback(c));
    } else {           // the one wait of a call: the overflow flag decides between finishing and the unscreened search
      ANYLOC_HIP(hipMemcpyAsync(&overflow, c.w.overflow, sizeof(int), hipMemcpyDeviceToHost, stream));
      ANYLOC_HIP(hipStreamSynchronize(stream));
    }
  }
  if (!screen || overflow) ANYLOC_TRY(panel_search(c));
  // padding entries carry index -1 regardless of index_base (faiss); L2 distances are sign-flipped back
  hipLaunchKernelGGL(topk_finish_kernel, dim3((unsigned)cdiv(nq * k, 256)), dim3(256), 0, stream, dist, c.idx, nq * k, metric);
  return launch_status("topk_finish_kernel");
}

}  // namespace
}  // namespace anyloc

using namespace anyloc;

extern "C" {

size_t anyloc_topk_workspace_bytes(int64_t nq, int64_t ndb, int64_t dim, int64_t k) {
  return carve(nullptr, 0, topk_plan(nq, ndb, dim, k, false)).bytes + 256;
}

int anyloc_topk(const float* queries, int64_t nq, const float* db, int64_t ndb, int64_t dim, int64_t k, int metric, unsigned flags,
                int64_t index_base, float* dist, int64_t* idx, void* workspace, size_t workspace_bytes, void* stream) {
  ANYLOC_CHECK_ARG((flags & ANYLOC_TOPK_RESCORE_PLANES) == 0,
                   "topk: ANYLOC_TOPK_RESCORE_PLANES needs a prepared index (anyloc_topk_search_index / anyloc_topk_search_index_rows)");
  return topk_impl(queries, nq, db, ndb, dim, k, metric, flags, index_base, dist, idx, workspace, workspace_bytes, nullptr,
                   static_cast<hipStream_t>(stream));
}

int anyloc_topk_path(int64_t nq, int64_t ndb, int64_t dim) {
  return nq <= 0 || ndb < 0 || dim < 4 || dim % 4 ? -1 : topk_plan(nq, ndb, dim, 0, false).path;
}

size_t anyloc_topk_index_bytes(int64_t ndb, int64_t dim) {
  return index_supported(ndb, dim) ? index_view(nullptr, ndb, dim).bytes + 256 : 0;
}

int anyloc_topk_index_build(const float* db, int64_t ndb, int64_t dim, void* index, size_t index_bytes, void* stream_) {
  ANYLOC_CHECK_ARG(db && index && ndb > 0, "topk_index_build: null pointer / empty database");
  if (!index_supported(ndb, dim)) {
    set_error("topk_index_build: dim %lld is not served by the fp16 score panels", (long long)dim);
    return ANYLOC_ERR_UNSUPPORTED;
  }
  const IndexView iv = index_view(index, ndb, dim);
  if (iv.bytes > index_bytes) {
    set_error("topk_index_build: index buffer %zu < %zu", index_bytes, iv.bytes);
    return ANYLOC_ERR_WORKSPACE;
  }
  return anyloc_topk_index_build_range(db, 0, ndb, ndb, dim, index, index_bytes, stream_);
}

int64_t anyloc_topk_index_panel(int64_t dim) { return index_supported(1, dim) ? index_panel(dim) : 0; }

int anyloc_topk_index_build_range(const float* rows, int64_t row0, int64_t nrows, int64_t ndb, int64_t dim, void* index,
                                  size_t index_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!index_supported(ndb, dim)) {
    set_error("topk_index_build_range: a [%lld, %lld] database is not served by the fp16 score panels", (long long)ndb, (long long)dim);
    return ANYLOC_ERR_UNSUPPORTED;
  }
  const IndexView iv = index_view(index, ndb, dim);
  ANYLOC_CHECK_ARG(row0 >= 0 && nrows > 0 && nrows <= ndb && row0 <= ndb - nrows,
                   "topk_index_build_range: rows [%lld, %lld + %lld) are not inside the %lld rows of the database", (long long)row0,
                   (long long)row0, (long long)nrows, (long long)ndb);
  ANYLOC_CHECK_ARG(row0 % iv.panel == 0, "topk_index_build_range: row0 %lld is not a multiple of the panel (%lld rows)", (long long)row0,
                   (long long)iv.panel);
  ANYLOC_CHECK_ARG(nrows % iv.panel == 0 || row0 + nrows == ndb,
                   "topk_index_build_range: nrows %lld is neither a multiple of the panel (%lld rows) nor ends at the last row",
                   (long long)nrows, (long long)iv.panel);
  if (iv.bytes > index_bytes) {
    set_error("topk_index_build_range: index buffer %zu < %zu", index_bytes, iv.bytes);
    return ANYLOC_ERR_WORKSPACE;
  }
  ANYLOC_CHECK_ARG(rows && index, "topk_index_build_range: null pointer");
  for (int64_t c0 = row0; c0 < row0 + nrows; c0 += iv.panel) {
    const int64_t pc = std::min<int64_t>(iv.panel, ndb - c0);     // (a range ends on a panel boundary or at the last row)
    unsigned char* img = iv.img + (size_t)(c0 / iv.panel) * iv.slot;
    ANYLOC_TRY(split_h2_wide(rows + (c0 - row0) * dim, dim, pc, dim, img, iv.dinv + c0, iv.dss + c0, stream));
    ANYLOC_TRY(screen_resid(img, pc, (int)(dim / 16), pc, iv.dinv + c0, iv.dss + c0, iv.drho + c0, nullptr, stream));
  }
  return ANYLOC_OK;
}

size_t anyloc_topk_index_workspace_bytes(int64_t nq, int64_t ndb, int64_t dim, int64_t k) {
  return index_supported(ndb, dim) ? carve(nullptr, 0, topk_plan(nq, ndb, dim, k, true)).bytes + 256 : 0;
}

int anyloc_topk_search_index(const float* queries, int64_t nq, const void* index, int64_t ndb, int64_t dim, int64_t k, int metric,
                             unsigned flags, int64_t index_base, float* dist, int64_t* idx, void* workspace, size_t workspace_bytes, void* stream) {
  ANYLOC_CHECK_ARG(index && index_supported(ndb, dim), "topk_search_index: no index / shape not served by the fp16 score panels");
  return topk_impl(queries, nq, nullptr, ndb, dim, k, metric, flags, index_base, dist, idx, workspace, workspace_bytes, index,
                   static_cast<hipStream_t>(stream));
}

int anyloc_topk_search_index_rows(const float* queries, int64_t nq, const float* db, const void* index, int64_t ndb, int64_t dim, int64_t k,
                                  int metric, unsigned flags, int64_t index_base, float* dist, int64_t* idx, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  ANYLOC_CHECK_ARG(index && index_supported(ndb, dim), "topk_search_index_rows: no index / shape not served by the fp16 score panels");
  return topk_impl(queries, nq, db, ndb, dim, k, metric, flags, index_base, dist, idx, workspace, workspace_bytes, index,
                   static_cast<hipStream_t>(stream));
}

}  // extern "C"
