// Small-M plans of the row-scaled two-term fp16 GEMM (kernel: gemm_h3_kernel.hpp; arithmetic: gemm_h3.hip).
//
// The reference's scripts call the extractor with ONE image (scripts/dino_v2_vlad.py:164-188, demo/anyloc_vlad_generate.py
// :163-186): 530 token rows at 322 x 322.  A block GEMM then has a handful of row tiles and the 128 x 256 tiling of the
// batched forward leaves most of the 256 CUs idle: proj / fc2 of ViT-g on 64 x 64 tiles are 216 two-wave workgroups = 432
// waves for 1024 SIMDs.  A plan = (tile shape, k-blocks per ring stage, ring depth, split-K factor) picked per GEMM from its
// shape -- the table in choose() holds the measured winners; what the sweeps showed about this regime is written there:
//   * split-K: the contraction is cut into `ksplit` ranges, one workgroup each, so a K = 4096 GEMM of 216 tiles becomes 864
//     workgroups of 64 k-blocks; partial accumulators meet in a workspace and the LAST arrival of a tile (ticket) sums them
//     in split order -- deterministic -- and runs the fused epilogue (LayerScale-residual, q|k|v planes, SwiGLU + quantise);
//   * wider tiles (64 x 128, 64 x 256) where N is large (qkv, w12): twice the flops per staged byte of a 64 x 64 tile.
// A one-image forward is therefore no longer bitwise the same image inside a batch (other summation order over k); both
// meet the oracle bar, and they agree to ~1e-7 (tests/test_gpu_vit.py).
#include "gemm_h3_kernel.hpp"

namespace anyloc {

namespace {

constexpr int LN_LEAD_MAX_TILES = 200;        // GEMM workgroups of a lead launch: fewer than CUs, so the lead workgroups always find one

// the round-3 rule: below option h3_tiny_max tiles of 128 x 128, 64 x 64 two-wave tiles
bool tiny(const H3Problem& p) { return cdiv(p.M, 128) * cdiv(p.N, 128) < option(OPT_H3_TINY_MAX); }

// The plan table.  Starting point: the round-3 small-batch rules (64 x 64 two-wave tiles with four / two k-blocks per ring
// stage while a workgroup is alone on its CU, 128 x 128 four-wave tiles from 256 such tiles up).  Up to two images (M <= 1100
// rows) the measured winners of the plan sweeps replace them (tools/sweep_b1.py on one MI355X, ViT-G/14 322 x 322, time per
// launch inside a B = 1 / B = 2 forward: profiles/r04_b1_plan_sweep.log, r04_b1_plan_sweep_depth.log):
//   fc2   (K = 4096, N = 1536)  64 x 128 four-wave tiles, 6-deep ring; split-K 2 at B=1: 49.9 -> 39.7 us;  B=2 unsplit: 75.7 -> 56.8
//   proj  (K = 1536, N = 1536)  B=1: 64 x 64, 6-deep ring 25.0 -> 22.7 us;  B=2: 64 x 128, 6-deep ring 34.8 -> 28.3
//   qkv   (N = 4608)            B=1: 128 x 128, 6-deep ring 39.1 -> 37.8 us;   B=2: 64 x 128 four-wave 56.1 -> 53.4
//   w12   (N = 8192)            among the 64- / 128-row shapes the round-3 choice stays the fastest (128 x 128 at B=1: 59 us by HIP
//                               events, 55 us by dispatch timestamps) -- but its 5 x 64 = 320 workgroups put TWO on 64 of the 256 CUs
//                               while 192 CUs hold one: the launch lasts as long as two tiles on one CU (qkv on the same tile,
//                               180 workgroups = one per CU, takes 33 us).  One image is 530 rows = 3 row tiles of 192 (576 rows:
//                               8 % padding instead of 21 %): 192 x 128 tiles are 3 x 64 = 192 equal workgroups, one per CU, each
//                               1.5 x the work of a 128 x 128 tile instead of 2 x (option h3s_w12_tall, default 1; 0 = 128 x 128):
//                               61.0 -> 51.1 us per launch, 49.2 with the 6-deep ring (120 KiB: one workgroup per CU is all there
//                               is), 6.21 -> 5.83 ms per forward, the SAME bits (an unsplit plan keeps the order over k);
//                               192-row tiles forced on qkv / proj / fc2 lose (108 / 72 / 36 tiles; profiles/r04_b1_w12_tall.log)
// What the sweeps say about this regime: split-K pays only for the long contraction (a split workgroup's ticket hand-off and
// the last arrival's slab reads cost what the shorter k-loop saves at K = 1536); a deeper ring (bytes in flight) helps the
// GEMMs with the fewest workgroups; and with the weights resident on-die (a 2-block model) the same launches are no faster
// (profiles/r04_b1_weight_residency_probe.log) -- a one-image GEMM waits for its own fill / barrier / MFMA chain, not for HBM.
void choose(const H3Problem& p, H3Plan& pl) {
  auto set = [&](int tile, int kb, int ksplit, int stages = 3) { pl.tile = tile; pl.kb = kb; pl.ksplit = ksplit; pl.stages = stages; };
  const int64_t t64 = cdiv(p.M, 64) * cdiv(p.N, 64);
  if (!tiny(p)) set(4, 1, 1);
  else set(0, t64 < option(OPT_H3_DEEP_MAX) ? 4 : t64 < option(OPT_H3_DEEP2_MAX) ? 2 : 1, 1);
  if (option(OPT_H3S_ENABLE) == 0) return;                 // the round-3 small-batch kernels, exactly
  if (p.M <= 1100) {
    const bool one = p.M <= 600;                           // one 322 x 322 image (530 rows) / two
    if (p.N <= 2048 && p.K16 >= 192) set(2, 1, one ? 2 : 1, 6);              // fc2-like: long contraction, narrow output
    else if (p.N <= 2048) set(one ? 0 : 2, 1, 1, 6);                         // proj-like
    else if (p.N < 8192) set(one ? 4 : 2, 1, 1, one ? 6 : 3);                // qkv-like
    else if (one && p.M > 384 && option(OPT_H3S_W12_TALL)) set(7, 1, 1, 6);  // w12-like, 385 ... 576 rows: three 192-row tiles, one workgroup per CU
  } else if (p.M <= 1700) {
    // One 476 x 630 image = 1531 token rows: the reference scripts' DEFAULT shape (configs.py:141 resize [480, 640], centre crop
    // scripts/dino_v2_vlad.py:173-176) -- and three 322 x 322 images.  Round 5 sweep at that shape (tools/sweep_b1.py 1 ... 476x630,
    // profiles/r05_b1_480x640_plan_sweep.log; time per launch inside a B = 1 forward): the 128 x 128 default is within 1 - 3 % of
    // the best plan for qkv (70.6 us) and w12 (103.7 us); the two narrow GEMMs are not --
    //   fc2  (K = 4096, N = 1536): 144 tiles of 128 x 128 on 256 CUs; 64 x 128 four-wave tiles with split-K 2: 88.6 -> 76.3 us
    //   proj (K = 1536, N = 1536): 64 x 128 four-wave tiles, 6-deep ring:                                   40.1 -> 37.4 us
    if (p.N <= 2048 && p.K16 >= 192) set(2, 1, 2);
    else if (p.N <= 2048) set(2, 1, 1, 6);
  }
  const int64_t mask = option(OPT_H3S_MASK);
  const int bit = p.kind == H3_KIND_QKV ? 1 : p.kind == H3_KIND_PROJ ? 2 : p.kind == H3_KIND_FC1 ? 4 : p.kind == H3_KIND_FC2 ? 8 : 16;
  if (mask & bit) {
    const int64_t c = option(OPT_H3S_CFG), s = option(OPT_H3S_KSPLIT), k = option(OPT_H3S_KB);
    if (c >= 0 && c < NSMALL) pl.tile = (int)c;
    if (s > 0) pl.ksplit = (int)s;
    if (k == 1 || k == 2 || k == 4) pl.kb = (int)k;
    const int64_t st = option(OPT_H3S_STAGES);
    if (st == 3 || st == 6) pl.stages = (int)st;
  }
}

// the epilogues that write q|k|v tiles need whole heads per wave column block: NI even (all of kSmallTile have it)
template <int EPI, int ID, int KB, int ST>
int launch_small(const H3Problem& p, const H3Plan& pl, hipStream_t stream) {
  constexpr H3Tile T = kSmallTile[ID];
  if constexpr (small_kb(T, KB) == KB && small_stages(T, KB, ST) == ST) {
    if constexpr (small_lead_compiled(EPI, ID, KB, ST)) {
      if (pl.lead) return launch_h3<T.mi, T.ni, T.wm, T.wn, ST, 2, EPI, KB, 1>(p, pl, stream);
    }
    return launch_h3<T.mi, T.ni, T.wm, T.wn, ST, 2, EPI, KB>(p, pl, stream);
  } else {
    ANYLOC_CHECK_ARG(false, "gemm_h3: tile %d has no small-M kernel with %d k-blocks per stage and a %d-deep ring", ID, KB, ST);
  }
}

}  // namespace

// tile-rows per scheduling group (co-resident workgroups of an XCD share A / W panels through its L2): option h3_group_m, default 8
int h3_group_m() { return (int)std::max<int64_t>(1, option(OPT_H3_GROUP_M)); }

H3Plan h3_plan(const H3Problem& p, int epilogue, bool ln_in_front) {
  epilogue = plan_epilogue(epilogue);
  H3Plan pl{};
  pl.kb = 1; pl.ksplit = 1; pl.kper = p.K16;
  pl.group_m = h3_group_m();
  // option h3_epi_lds = 0: the dword read-modify-write epilogue (also the fallback for unaligned C)
  pl.epi_lds = epilogue == EPI_LS_RESID && option(OPT_H3_EPI_LDS) != 0 && p.N % 4 == 0 && p.ldc % 4 == 0 &&
               (reinterpret_cast<uintptr_t>(p.C) & 15) == 0 && (reinterpret_cast<uintptr_t>(p.resid) & 15) == 0;
  pl.fast_silu = (epilogue == EPI_SWIGLU_H2 || epilogue == EPI_SWIGLU_T || epilogue == EPI_SWIGLU_T_H2) && option(OPT_H3_FAST_SILU) != 0;
  // option h3_cfg (micro-benchmarks): 0 = 128x256 tile, 3-deep ring (default; the small-M plans when there are few tiles);
  // 1 - 5: kH3Tile, at every size
  const int cfg = (int)option(OPT_H3_CFG);
  // plain-store GEMMs of >= 256 tiles of 256 x 256 run on the 16 x 16 x 32 MFMA kernel (gemm_h3m.hip; option h3_mfma16: -1 =
  // when the contraction is >= 4096 long -- the retrieval panels, +3.6 % -- 0 never, 1 whatever the length)
  const int64_t m16 = option(OPT_H3_MFMA16);
  pl.mfma16 = epilogue == EPI_STORE && m16 != 0 && (m16 > 0 || p.K16 >= 256) && cdiv(p.M, 256) * cdiv(p.N, 256) >= 256;
  // few tiles -- one or a few images (the reference's scripts call the extractor per image): tile shape, ring depth and split-K
  // factor come from the small-M plan table; the epilogues without plans (unfused A/B data flows) keep two fixed shapes
  const bool few = cfg == 0 && cdiv(p.M, 128) * cdiv(p.N, 256) < 512;
  H3Tile t;
  if (few && small_epilogue(epilogue)) {
    pl.route = H3_ROUTE_SMALL;
    choose(p, pl);
    t = kSmallTile[pl.tile];
    // split-K needs the workspace, a plain (non-accumulating) epilogue input and enough k-blocks
    const int64_t tiles = cdiv(p.M, t.bm()) * cdiv(p.N, t.bn());
    if (!p.sk_part || !p.sk_tickets || p.accumulate) pl.ksplit = 1;
    pl.ksplit = (int)std::min<int64_t>(pl.ksplit, p.K16);
    while (pl.ksplit > 1 && ((size_t)pl.ksplit * tiles * t.bm() * t.bn() * sizeof(float) > H3_SPLIT_PART_BYTES || tiles > (int64_t)H3_SPLIT_TICKETS))
      --pl.ksplit;
    // k-blocks per split: a multiple of the ring stage's k-blocks (as the table asks for them), so that only the LAST split
    // can end inside a stage (its missing k-blocks lie beyond the buffer descriptors and read as zeros)
    if (pl.ksplit > 1) {
      pl.kper = (int)(cdiv(cdiv(p.K16, pl.ksplit), pl.kb) * pl.kb);
      pl.ksplit = (int)cdiv(p.K16, pl.kper);                 // no empty split
      if (pl.ksplit <= 1) { pl.ksplit = 1; pl.kper = p.K16; }
    }
    pl.kb = small_kb(t, pl.kb);
    pl.stages = small_stages(t, pl.kb, pl.stages);
  } else {
    pl.route = few ? H3_ROUTE_FIXED : H3_ROUTE_BATCHED;
    pl.tile = few ? (tiny(p) ? H3_TILE_TINY : H3_TILE_128) : (cfg >= 1 && cfg <= 5 ? cfg : 0);
    t = kH3Tile[pl.tile];
    pl.stages = t.stages;
  }
  pl.tiles_m = (int)cdiv(p.M, t.bm());
  pl.tiles_n = (int)cdiv(p.N, t.bn());
  pl.grid = (unsigned)(pl.tiles_m * pl.tiles_n * pl.ksplit);
  if (!ln_in_front) return pl;
  // The LayerNorm in front of this GEMM as the lead role of its launch.  One image per call (option h3s_ln_lead): an unsplit plan
  // the role is compiled for, with a CU left for every lead workgroup -- one row per wave, a multiple of 8 of them (XCD mapping
  // of the GEMM ids).  Batched (option h3_ln_lead): the default tile, an epilogue the role is compiled for, rows of at most
  // 1536 columns, and a workgroup order that passes the host check (tile_order.hpp: LeadPlan), which also gives the grid.
  static_assert(kH3Tile[0].bm() == 128, "h3_lead_plan_check simulates 128-row tiles");
  unsigned lead_grid = 0;
  if (pl.route == H3_ROUTE_SMALL && option(OPT_H3S_LN_LEAD) != 0 && small_lead_compiled(epilogue, pl.tile, pl.kb, pl.stages) &&
      pl.ksplit == 1 && pl.tiles_m * pl.tiles_n <= LN_LEAD_MAX_TILES) {
    pl.lead = 1;
    pl.grid += (unsigned)((cdiv(p.M, t.nw()) + 7) / 8 * 8);
  } else if (pl.route == H3_ROUTE_BATCHED && cfg == 0 && option(OPT_H3_LN_LEAD) != 0 && batched_lead_compiled(epilogue) &&
             16 * (int64_t)p.K16 <= 1536 && p.ksplit <= 1 &&
             h3_lead_plan_check(pl.tiles_m, pl.tiles_n, pl.group_m, p.M, &lead_grid)) {
    pl.lead = 2;
    pl.grid = lead_grid;
  }
  return pl;
}

int gemm_h3_small(const H3Problem& p, int epilogue, const H3Plan& pl, hipStream_t stream) {
  return with_constant<0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10>(epilogue, [&](auto e) -> int {
    constexpr int EPI = decltype(e)::value;
    if constexpr (small_epilogue(EPI)) {
      static_assert(NSMALL == 8);
      return with_constant<0, 1, 2, 3, 4, 5, 6, 7>(pl.tile, [&](auto id) {
        return with_constant<1, 2, 4>(pl.kb, [&](auto kb) {
          return with_constant<3, 6>(pl.stages, [&](auto st) {
            return launch_small<EPI, decltype(id)::value, decltype(kb)::value, decltype(st)::value>(p, pl, stream);
          });
        });
      });
    } else {
      set_error("gemm_h3_small: epilogue %d has no small-M plan", EPI);
      return ANYLOC_ERR_UNSUPPORTED;
    }
  });
}

}  // namespace anyloc
