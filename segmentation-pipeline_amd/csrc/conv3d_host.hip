// Host layer of the 3x3x3 convolutions: ONE resolver per descriptor (route_conv, route_bww, route_bww_c8), the planners it
// calls, and every extern "C" conv, pack and act16 entry point.  A query returns a number of the route; a launch resolves the
// route once, checks its workspace against that number and switches on the kind.  Kernels: conv3d*.hip, none here.
#include "conv3d_common.hpp"

namespace m355 {

// ------------------------------------------------------------------ planning
// Lanes along x per 32-voxel group: the widest of {32, 16, 8} unless a narrower one wastes noticeably
// fewer padded voxels (W = 24: 16 -> 2 tiles = 32 columns, 8 -> 3 tiles = 24 columns).

int pick_gx(int W) {
  int best = 8;
  int64_t best_pad = round_up(W, 8);
  for (int gx : {16, 32}) {
    const int64_t pad = round_up(W, gx);
    if (W >= gx && pad * 100 <= best_pad * 108) {  // prefer the wider tile unless it pads > 8 % more
      best = gx;
      best_pad = std::min(best_pad, pad);
    }
  }
  return best;
}

// M355_COMPUTE_F32X3 (conv3d_f32x3.hip): a 32-row tile must carry real rows, and the 8-channel slab of a sample must fit
// the 31-bit byte offsets its loads add up.  Layers with 3..7 K-channels (4 -> 32 forward, 3 -> 32 data gradient @128^3:
// one chunk, 4 / 3 of its 8 channels real) run 0.183 / 0.174 ms on the split kernel against 0.21 / 0.19 on the fp32 MFMA
// (0.06 ms of that is the 268 MB they write, the rest the half-empty K of their MFMAs) -- behind M355_F32X3_EDGE=1, off
// by default: with the FIRST layer of the net on the split kernel one voxel of the 2.1 M of the bench volume (a near-tie
// of two class probabilities) takes the other side of the CPU reference's argmax; with it on the fp32 MFMA none does.
static bool x3_layer(int kin, int mout, int D, int H, int W) {
  return tuning().f32x3 && kin >= (tuning().f32x3_edge ? 3 : 8) && mout > 4 && (int64_t)D * H * W < (1ll << 26);
}

// (tile height NTW, split-K) of one kernel family.  Each family has its own cost model below; all read the geometry that
// plan_mfma has filled into the plan.
struct TilePick {
  int ntw = 1, ks = 1;
};

// fp32 MFMA kernels.  Cost model instead of "fill the chip once":
// workgroups of one launch do equal work, so the time is rounds x (workgroups sharing a CU) x
// time of one workgroup, and a launch that needs 1.1 rounds costs as much as one that needs 2.
//   slots     NTW <= 4: 66.8 KB LDS -> two workgroups per CU (512); NTW = 8: one (256)
//   one chunk 54 x NTW MFMAs of 64 cycles per wave at ~2.04 GHz; + fill/epilogue (see `fixed`)
//   split-K   ks x out bytes written + read again by the reduce kernel (~4 TB/s) + a launch
static TilePick pick_f32(const FwdPlan& p, int N, int H, int64_t out_bytes) {
  const int gy = 32 / p.gx, cus = num_cus(), force_ntw = tuning().conv_ntw;
  const int wtiles = p.otiles + p.tile16;   // workgroup items per spatial tile
  int chosen = 1, chosen_ks = 1;
  double best = 1e30;
  for (int ntw : {4, 8, 2, 1}) {
    if (p.tile16 && ntw == 8) continue;              // the 16-row kernel is instantiated for NTW <= 4
    if (force_ntw && ntw != force_ntw && !(p.tile16 && force_ntw == 8)) continue;
    const int ty = ntw * gy;
    if (ty > H && ntw > 1 && !force_ntw) continue;  // do not overhang H by a whole factor
    const int64_t base_wg = (int64_t)p.tz_tiles * ceil_div(H, ty) * p.tx_tiles * wtiles * N;
    const int per_cu = ntw <= 4 ? 2 : 1;
    // narrow tiles re-read the weights from LDS more often per MFMA ((1 + NTW) / NTW reads each)
    const double chunk_us = 54.0 * ntw * 64.0 / 2040.0 / (ntw >= 4 ? 1.0 : ntw == 2 ? 0.96 : 0.8);
    for (int ks = 1; ks <= std::min(p.nchunks, 8); ++ks) {
      if (ks > 1 && (ks - 1) * ceil_div(p.nchunks, ks) >= p.nchunks) continue;  // an empty split
      if (ks > 1 && ks * out_bytes > (128ll << 20)) break;
      const int64_t nwg = base_wg * ks;
      const double rounds = (double)ceil_div(nwg, (int64_t)cus * per_cu);
      // a lone workgroup on a CU has nothing to cover its barriers and LDS commits: measured ~0.8 of
      // the paired rate for NTW <= 4 (u0.c0 pinned to one per CU: 111 vs 126 TFLOP/s), ~0.93 for NTW = 8
      const bool lone = per_cu == 1 || nwg <= cus;
      const double share = lone ? 1.0 / (per_cu == 1 ? 0.93 : 0.8) : (double)per_cu;
      // fixed cost of an item: ~1 chunk for a one-shot workgroup, ~0.5 when the persistent kernel
      // (more items than resident workgroups) prefetches across the item boundary
      const double fixed = nwg > (int64_t)cus * per_cu ? 0.5 : 1.0;
      double cost = rounds * share * ((double)ceil_div(p.nchunks, ks) + fixed) * chunk_us;
      if (ks > 1) cost += (2.0 * ks + 1.0) * (double)out_bytes / 4.0e6 + 4.0;
      if (cost < best * 0.98) {  // candidates come in order of preference: switch only for a real gain
        best = cost;
        chosen = ntw;
        chosen_ks = ks;
      }
    }
  }
  return {chosen, chosen_ks};
}

// conv3_f32x3_kernel: one item per workgroup, two workgroups per CU, NTW <= 4.  A chunk (8 channels) is 14 x 6 x NTW
// MFMAs of 32 cycles per wave at the ~1.6 GHz the bf16 pipe holds; split-K as for the fp32 kernels
static TilePick pick_x3(const FwdPlan& p, int N, int H, int64_t out_bytes) {
  const int gy = 32 / p.gx, cus = num_cus(), force_ntw = tuning().conv_ntw;
  int chosen = 1, chosen_ks = 1;
  double best3 = 1e30;
  for (int ntw : {4, 2, 1}) {
    if (force_ntw && ntw != force_ntw && force_ntw != 8) continue;
    const int ty = ntw * gy;
    if (ty > H && ntw > 1 && !force_ntw) continue;
    const int64_t base_wg = (int64_t)p.tz_tiles * ceil_div(H, ty) * p.tx_tiles * (p.otiles + p.tile16) * N;   // (a 16-row item: half the time)
    const double chunk_us = 14.0 * 6.0 * ntw * 32.0 / 1600.0 / (ntw >= 4 ? 1.0 : ntw == 2 ? 0.9 : 0.75);
    for (int ks = 1; ks <= std::min(p.nchunks, 8); ++ks) {
      if (ks > 1 && (ks - 1) * ceil_div(p.nchunks, ks) >= p.nchunks) continue;
      if (ks > 1 && ks * out_bytes > (128ll << 20)) break;
      const int64_t nwg = base_wg * ks;
      const double rounds = (double)ceil_div(nwg, (int64_t)cus * 2);
      const double share = nwg <= cus ? 1.0 / 0.8 : 2.0;
      double cost = rounds * share * ((double)ceil_div(p.nchunks, ks) + 1.0) * chunk_us;
      if (ks > 1) cost += (2.0 * ks + 1.0) * (double)out_bytes / 4.0e6 + 4.0;
      if (cost < best3 * 0.98) {
        best3 = cost;
        chosen = ntw;
        chosen_ks = ks;
      }
    }
  }
  return {chosen, chosen_ks};
}

// 16-bit kernels, one item per workgroup (conv3_h16_kernel, ONE): cost model over (tile height, split-K).
//   time ~ residencies x (chunks per item x chunk time(NTW) x share + fixed(NTW)) + split-K reduction
// chunk time per workgroup with two resident per CU (measured: ~44 % of the MFMA rate at NTW = 4; narrower tiles
// re-read the weights more often), `share` < 1 when the launch leaves CUs with a single workgroup, the reduction
// pass ~12 us + its slab traffic.  Constants fitted on the cfg2 layers (tools/plan_sweep_h16.py).
static TilePick pick_h16_oneshot(const FwdPlan& p, int N, int H, int64_t out_bytes) {
  const int gy = 32 / p.gx, cus = num_cus(), force_ntw = tuning().conv_ntw;
  int chosen = 1, chosen_ks = 1;
  double best_h = 1e30;
  for (int ntw : {4, 2, 1}) {
    if (p.gx == 8 && ntw == 4) continue;                 // not instantiated
    if (force_ntw && ntw != force_ntw && force_ntw != 8 && !(p.gx == 8 && force_ntw == 4)) continue;
    const int ty = ntw * gy;
    if (ty > H && ntw > 1 && !force_ntw) continue;
    const double chunk_us = ntw == 4 ? 5.8 : (ntw == 2 ? 3.5 : 2.8), fixed_us = ntw == 4 ? 6.0 : (ntw == 2 ? 3.5 : 2.5);
    const int64_t nwg1 = (int64_t)p.tz_tiles * ceil_div(H, ty) * p.tx_tiles * p.otiles * N;
    for (int ks = 1; ks <= std::min(p.nchunks, 8); ++ks) {
      if (ks > 1 && (ks - 1) * ceil_div(p.nchunks, ks) >= p.nchunks) continue;   // an empty split
      if (ks > 1 && ks * out_bytes > (128ll << 20)) break;
      const int64_t nwg = nwg1 * ks;
      const double per_cu = (double)nwg / cus;
      const double share = 0.58 + 0.42 * std::min(1.0, std::max(0.0, per_cu - 1.0));
      const double rounds = std::max(1.0, (double)ceil_div(nwg, 2 * (int64_t)cus));
      double cost = rounds * ((double)ceil_div(p.nchunks, ks) * chunk_us * share + fixed_us);
      if (ks > 1) cost += 14.0 + (double)(ks + 1) * (double)out_bytes / 2.5e6;
      if (cost < best_h * 0.97) {
        best_h = cost;
        chosen = ntw;
        chosen_ks = ks;
      }
    }
  }
  return {chosen, chosen_ks};
}

// 16-bit operand modes, queue-driven kernels (M355_H16_ONESHOT=0 / 3): fill the chip once, largest tile
// first; the instantiated tiles are NTW <= 4 (<= 2 for 8 lanes along x).  May switch the plan to the 8-wave variant.
static TilePick pick_h16_queue(FwdPlan& p, int N, int D, int H, int64_t out_bytes) {
  const int gy = 32 / p.gx, cus = num_cus(), force_ntw = tuning().conv_ntw;
  int chosen = 1, chosen_ks = 1;
  for (int ntw : {4, 2, 1}) {
    if (p.gx == 8 && ntw == 4) continue;
    if (force_ntw && ntw != force_ntw && force_ntw != 8 && !(p.gx == 8 && force_ntw == 4)) continue;
    const int ty = ntw * gy;
    if (ty > H && ntw > 1 && !force_ntw) continue;
    const int64_t nwg = (int64_t)p.tz_tiles * ceil_div(H, ty) * p.tx_tiles * p.otiles * N;
    int64_t ks = std::max<int64_t>(1, std::min<int64_t>(ceil_div(512, nwg), std::min<int64_t>(p.nchunks, 8)));
    while (ks > 1 && ks * out_bytes > (128ll << 20)) --ks;
    while (ks > 1 && (ks - 1) * ceil_div(p.nchunks, ks) >= p.nchunks) --ks;
    chosen = ntw;
    chosen_ks = (int)ks;
    if (nwg * ks * 4 >= 512 * 3) break;
  }
  if (p.gx == 32 && tuning().h16_w8 && D >= 8 && H >= 2) {
    // 8-wave double-buffered variant (tile 8 x 2 x 32, one workgroup per CU) for SHORT items (<= 4 chunks = 64
    // input channels) whose tiles fill the chip without split-K: there the single-buffered kernel spends as long
    // on chunk boundaries and item switches as on MFMAs (32->32 @128^3: 0.194 -> 0.167 ms, 32->64 @64^3: 0.088 ->
    // 0.058).  Long items stay on the 4-wave kernel: its 4-row wave tile needs 0.75 LDS fragment reads per MFMA,
    // the 2-row tile of this variant 1.17, and at 6+ chunks that LDS traffic costs more than the boundaries
    // (96->32 @128^3: 0.33 vs 0.41 ms).
    const int64_t items8 = (int64_t)ceil_div(D, 8) * ceil_div(H, 2) * p.tx_tiles * p.otiles * N;
    if (((items8 >= 2 * (int64_t)cus && p.nchunks <= 4) || tuning().h16_w8 == 2) && (!force_ntw || force_ntw == 2)) {   // 2: always (tests)
      p.nw = 8;
      p.tz_tiles = (int)ceil_div(D, 8);
      chosen = 2;
      chosen_ks = 1;
    }
  }
  return {chosen, chosen_ks};
}

// Plan for a 3x3x3/s1/p1 conv with K-channels `kin` and M-channels `mout`.
static FwdPlan plan_mfma(int N, int kin, int mout, int D, int H, int W, int compute) {
  FwdPlan p{};
  p.mfma = true;
  p.gx = pick_gx(W);
  const int gy = 32 / p.gx;
  const bool h16 = is16(compute);  // bf16 / fp16 operand modes share one plan
  if (compute == M355_COMPUTE_F32 && tuning().f32x3 == 2) compute = M355_COMPUTE_F32X3;   // M355_F32X3=2: test hook
  const bool x3 = compute == M355_COMPUTE_F32X3 && x3_layer(kin, mout, D, H, W);
  p.x3 = x3 ? 1 : 0;
  const int cc = h16 ? 16 : (x3 ? 8 : 4);  // input channels per LDS chunk
  p.kin_pad = (int)round_up(kin, cc);
  p.mout_pad = (int)round_up(mout, 32);
  p.otiles = p.mout_pad / 32;
  // fp32: a remainder of 1..16 channels runs as ONE 16-row tile on v_mfma_f32_16x16x4_f32 (half the MFMA time of a
  // padded 32-row tile): 40 channels = 32 + 16 rows instead of 64, 80 = 64 + 16 instead of 96
  p.tile16 = (!h16 && tuning().tile16 && mout % 32 >= 1 && mout % 32 <= 16) ? 1 : 0;   // (split kernels: conv3_f32x3_m16_kernel)
  if (p.tile16) p.otiles -= 1;
  p.nchunks = p.kin_pad / cc;
  p.nw = 4;
  p.tz_tiles = (int)ceil_div(D, 4);
  p.tx_tiles = (int)ceil_div(W, p.gx);
  const int64_t ob = (int64_t)N * mout * D * H * W * 4;
  p.oneshot = h16 && tuning().h16_oneshot && tuning().h16_oneshot != 3;
  TilePick t = h16 ? (p.oneshot ? pick_h16_oneshot(p, N, H, ob) : pick_h16_queue(p, N, D, H, ob))
                   : (x3 ? pick_x3(p, N, H, ob) : pick_f32(p, N, H, ob));
  if (const int force_ks = tuning().conv_ksplit) {
    t.ks = std::min(force_ks, p.nchunks);
    while (t.ks > 1 && (t.ks - 1) * (int)ceil_div(p.nchunks, t.ks) >= p.nchunks) --t.ks;
  }
  p.ntw = t.ntw;
  p.ty_tiles = (int)ceil_div(H, p.ntw * gy);
  p.ksplit = t.ks;
  // resident workgroups (LDS + registers: 2 per CU up to NTW = 4); the override exists for the tests
  const int64_t slots = (tuning().conv_slots ? tuning().conv_slots : (p.nw == 8 ? 1 : (p.ntw <= 4 ? 2 : 1)) * num_cus());
  const int64_t items = (int64_t)p.tz_tiles * p.ty_tiles * p.tx_tiles * p.otiles * N * p.ksplit;
  // single-chunk items (Cin <= 4: the first conv of the network, the data gradient of the output conv) have no
  // second chunk to hide the queue ticket's round trip or the next item's prefetch behind: the one-shot grid is
  // faster there (4->32 @128^3: 0.187 vs 0.248 ms)
  // ... and the queue only pays beyond two residencies of items: up to there the one-shot grid, whose workgroups
  // the hardware hands out as CUs free up, is 3-7 % faster (192->64 @64^3, 2.0 residencies: 1.237 -> 1.195 ms;
  // 128->384 @32^3, 1.5: 0.672 -> 0.628); from 3.4 residencies (40->40 @96^3) the queue wins by 7-9 %
  p.persistent = !h16 && !x3 && items < (1ll << 31) && tuning().conv_persistent &&
                 (tuning().conv_persistent > 1 ? items > slots
                                               : (items > 2 * slots && ceil_div(p.nchunks, p.ksplit) > 1));
  // packed weights + 256 B for the work counter of the persistent kernel
  p.wp_bytes = (size_t)round_up((int64_t)p.kin_pad * 27 * p.mout_pad * (h16 ? 2 : 4), 256) + 256;
  if (x3)   // [tile][chunk][pair][plane][lane] x 16 B, then the 16-row tile's [chunk][quad][plane][lane] x 16 B
    p.wp_bytes = (size_t)p.otiles * p.nchunks * (14 * 3 * 1024) + (size_t)p.tile16 * p.nchunks * (7 * 3 * 1024) + 256;
  p.slab_bytes = p.ksplit > 1 ? (size_t)p.ksplit * N * mout * D * H * W * 4 : 0;
  return p;
}

static BwwPlan plan_bww(int N, int Cin, int Cout, int D, int H, int W) {
  BwwPlan p{};
  p.gx = pick_gx(W);
  const int tz = p.gx == 8 ? 4 : 2, ty = p.gx == 32 ? 4 : 8;
  p.tz_tiles = (int)ceil_div(D, tz);
  p.ty_tiles = (int)ceil_div(H, ty);
  p.tx_tiles = (int)ceil_div(W, p.gx);
  p.otiles = (int)ceil_div(Cout, 32);
  p.ctiles = (int)ceil_div(Cin, 32);
  const int64_t ntiles = (int64_t)N * p.tz_tiles * p.ty_tiles * p.tx_tiles;
  const int64_t pairs = (int64_t)p.otiles * p.ctiles;
  const auto rem16 = [](int c) { return c % 32 >= 1 && c % 32 <= 16 ? 1 : 0; };
  p.k.orem = tuning().tile16 ? rem16(Cout) : 0;
  p.k.crem = tuning().tile16 ? rem16(Cin) : 0;
  p.k.of = p.otiles - p.k.orem;
  p.k.cf = p.ctiles - p.k.crem;
  p.classes = (p.k.orem || p.k.crem) && Cin > 4 && Cout > 4;
  // One workgroup per CU; workgroups have equal work, so time ~ rounds x (tiles per split + fixed
  // cost of a workgroup: pipeline fill + the 110 KB slab write, ~half a tile).  Pick the split that
  // minimises it (a power of two up to the tile count) instead of just filling 256 CUs once.
  int64_t nsplit = 1;
  const int cus = num_cus();
  {
    int64_t cand[80];   // <= 63 powers of two + 8 round counts + the tile count
    int nc = 0;
    for (int64_t ns = 1; ns < ntiles; ns *= 2) cand[nc++] = ns;
    for (int r = 1; r <= 8; ++r) cand[nc++] = std::max<int64_t>(1, (int64_t)cus * r / pairs);  // exactly r rounds
    cand[nc++] = std::max<int64_t>(1, ntiles);
    std::sort(cand, cand + nc);
    double best = 1e30;
    for (int i = 0; i < nc; ++i) {
      const int64_t ns = std::min<int64_t>(cand[i], std::max<int64_t>(1, ntiles));
      const double rounds = (double)ceil_div(pairs * ns, cus);
      const double cost = rounds * ((double)ceil_div(ntiles, ns) + 0.5);
      if (cost < best * 0.97) {  // prefer fewer splits (less slab traffic) unless clearly better
        best = cost;
        nsplit = ns;
      }
    }
  }
  // Queue-driven: the plan above fills the chip in ONE residency (one workgroup per CU), so a CU that another
  // kernel still holds when this one starts -- an RCCL gradient bucket overlapping the backward pass -- delays
  // exactly the workgroup mapped there, and the launch takes up to twice as long.  Splitting the voxel range 2-3x
  // finer makes 2-3 units per CU that the hardware dispatcher hands to whichever CU is free (a held CU simply
  // takes fewer); every unit still sums a FIXED tile set into its own slab, so the result does not depend on who
  // ran what and stays bit-reproducible.  Each unit pays a pipeline fill and a slab write (and the reduce reads
  // one more slab), so this is only done where a unit keeps >= 32 tiles: measured +0.8 % on 96->32 @128^3 at 3
  // units per CU, but +9 % / +18 % on 32->32 @128^3 / 64->64 @64^3 (11 / 5 tiles per unit), which stay static.
  if (tuning().bww_queue && Cin > 4 && Cout > 4 && pairs * nsplit <= cus) {
    const int64_t per_unit = ceil_div(ntiles, nsplit);
    const int m = per_unit >= 96 ? 3 : (per_unit >= 64 ? 2 : 1);
    if (m * nsplit * (int64_t)Cout * Cin * 27 * 4 <= (96ll << 20)) nsplit *= m;
  }
  if (const int force = tuning().bww_nsplit) nsplit = std::min<int64_t>(force, std::max<int64_t>(1, ntiles));
  if (Cin <= 4 || Cout <= 4)  // tap-on-lane kernel: small LDS footprint, ~3 workgroups per CU
    nsplit = std::max<int64_t>(1, 768 / std::max<int64_t>(1, ceil_div(Cin <= 4 ? Cout : Cin, 32)));
  nsplit = std::min<int64_t>(nsplit, ntiles);
  p.nsplit = (int)nsplit;
  int64_t max_ns = nsplit;
  for (int c = 0; c < 4; ++c) p.k.ns[c] = p.nsplit;
  if (p.classes) {
    // pair classes of the remainder kernel: MFMA cost of a pair in units of a full 32 x 32 pair; the split count of
    // a class is proportional to it, scaled so that the whole launch is `rounds` residencies of equal workgroups
    const double cost[4] = {1.0, 0.5, 0.5, 0.25};
    const int64_t npairs[4] = {(int64_t)p.k.of * p.k.cf, (int64_t)p.k.of * p.k.crem, (int64_t)p.k.orem * p.k.cf,
                               (int64_t)p.k.orem * p.k.crem};
    double units = 0;
    for (int c = 0; c < 4; ++c) units += cost[c] * (double)npairs[c];
    // splits of a full pair: one residency of the chip (one workgroup per CU), never more splits than tiles; the
    // rounding of the per-class counts must not spill a workgroup into a second residency
    double base = std::min((double)ntiles, (double)cus / units);
    if (const int force = tuning().bww_nsplit) base = (double)std::min<int64_t>(force, std::max<int64_t>(1, ntiles));
    int wg = 0;
    for (;;) {
      wg = 0;
      max_ns = 1;
      for (int c = 0; c < 4; ++c) {
        const int64_t ns = std::max<int64_t>(1, std::min<int64_t>(ntiles, (int64_t)(base * cost[c] + 0.5)));
        p.k.ns[c] = npairs[c] ? (int)ns : 1;
        p.k.start[c] = wg;
        wg += (int)(npairs[c] * p.k.ns[c]);
        if (npairs[c]) max_ns = std::max<int64_t>(max_ns, ns);
      }
      if (wg <= cus || base <= 1.0 || tuning().bww_nsplit) break;
      base *= 0.99;
    }
    p.class_wgs = wg;
    max_ns = std::max<int64_t>(max_ns, nsplit);   // the uniform plan stays usable (generic kernel when W % 4 != 0)
  }
  p.slab_bytes = (size_t)round_up(max_ns * Cout * Cin * 27 * 4, 256);
  return p;
}

static int bww_c8_nsplit(const m355_conv3d_desc* d) {
  const int64_t ntiles = (int64_t)d->N * ceil_div(d->D, 2) * ceil_div(d->H, 4) * ceil_div(d->W, 32);
  const int64_t pairs = ceil_div(d->Cin, 32) * ceil_div(d->Cout, 32);
  const int64_t slots = 2 * (int64_t)num_cus();
  if (const int force = tuning().bww_nsplit) return (int)std::min<int64_t>(force, ntiles);
  // time ~ residencies x (tiles per split x tile time + ~4 us pipeline fill and slab write) + the slab traffic (written
  // by the kernel, read by the reduction).  Tile time ~1.8 us with two workgroups sharing a CU, ~1.1 us alone: for few
  // pairs one workgroup per CU with half the slabs wins (32->32 @128^3: 256 splits 170 us, 512 splits 184 us), for many
  // tiles per pair two per CU do (tools/plan_sweep_bww_c8.py).
  const double slab_us = 2.0 * (double)d->Cout * d->Cin * 27 * 4 / 4.0e6;
  double best = 1e30;
  int64_t best_ns = 1;
  for (int h = pairs <= 2 ? 1 : 2; h <= 8; ++h) {   // h half-residencies: 256, 512, 768, ... workgroups (one per CU
                                                    // only pays for one or two pairs: more pairs share tiles in L2)
    const int64_t ns = std::max<int64_t>(1, std::min<int64_t>(ntiles, slots * h / (2 * pairs)));
    const int64_t wgs = pairs * ns;
    const double rounds = (double)ceil_div(wgs, slots);
    const double tile_us = wgs * 2 <= slots ? 1.1 : (wgs >= slots ? 1.8 : 1.1 + 0.7 * (double)(wgs * 2 - slots) / (double)slots);
    const double cost = rounds * ((double)ceil_div(ntiles, ns) * tile_us + 4.0) + (double)ns * slab_us;
    if (cost < best * 0.97) {
      best = cost;
      best_ns = ns;
    }
  }
  return (int)best_ns;
}

// ------------------------------------------------------------------ routes
// The MFMA kernels: 3x3x3, stride 1, padding 1, and a volume whose 4-channel slab fits the 32-bit byte
// offsets of a buffer descriptor (< 2^27 voxels, i.e. below 512^3); anything else takes the generic
// direct kernels (64-bit indexing).
static bool is_k3s1p1(const m355_conv3d_desc* d) {
  return d->k == 3 && d->stride == 1 && d->pad == 1 && (int64_t)d->D * d->H * d->W < (1ll << 27);
}
// Cout <= 4 forward in exact fp32: packed rows instead of a mostly-empty 32-row tile
static bool small_cout_fwd(const m355_conv3d_desc* d) {
  return d->Cout <= 4 && !is16(d->compute) && d->W >= 32 && d->D >= 8 && d->Cin >= 8 &&
         !tuning().no_small && (int64_t)std::max(d->Cin, d->Cout) * d->D * d->H * d->W < (1ll << 31);
}
// bytes of the c8 staging copy the fp32-input entry points make in 16-bit operand modes
static size_t act16_staging_bytes(int N, int C, int64_t S) { return (size_t)round_up((int64_t)N * c8_blocks(C) * S * 16, 256); }
static int64_t out_voxels(const m355_conv3d_desc* d) {
  return (int64_t)out_dim(d->D, d->k, d->stride, d->pad) * out_dim(d->H, d->k, d->stride, d->pad) * out_dim(d->W, d->k, d->stride, d->pad);
}
static size_t dbias_ws_bytes(int Cout, int64_t S) {
  return (size_t)round_up((int64_t)Cout * ceil_div(S, DBIAS_CHUNK) * 8, 256);
}

ConvRoute route_conv(const m355_conv3d_desc* d, int which) {
  ConvRoute r{};
  r.kind = ConvKind::Direct;
  if (!is_k3s1p1(d)) return r;
  const int64_t S = (int64_t)d->D * d->H * d->W;
  if (which == 0 && small_cout_fwd(d)) {
    // the packed-FMA kernel by default; both take the (larger) buffer of the z-Toeplitz MFMA variant
    const bool valu = tuning().smallcout_valu && S < (1ll << 27);
    r.kind = valu ? ConvKind::SmallCoutValu : ConvKind::SmallCoutToeplitz;
    r.packed_bytes = r.workspace_bytes = smallcout_packed_bytes(d->Cin);
    r.fuses_softmax = valu && tuning().fuse_softmax;   // softmax over the output channels in the epilogue
    r.plan_code[0] = 2;
    return r;
  }
  // data gradient: dx = conv(dy, flipped / transposed w), K-channels = Cout, M-channels = Cin
  const int kin = which == 0 ? d->Cin : d->Cout, mout = which == 0 ? d->Cout : d->Cin;
  const FwdPlan& p = r.plan = plan_mfma(d->N, kin, mout, d->D, d->H, d->W, d->compute);
  const bool h16 = is16(d->compute);
  r.kind = h16 ? (p.oneshot ? ConvKind::H16OneShot : (p.nw == 8 ? ConvKind::H16Queue8 : ConvKind::H16Queue))
               : (p.x3 ? ConvKind::X3 : (p.persistent ? ConvKind::MfmaF32Queue : ConvKind::MfmaF32));
  r.packed_bytes = p.wp_bytes;
  r.h16_workspace_bytes = h16 ? p.wp_bytes + p.slab_bytes : 0;
  r.workspace_bytes = p.wp_bytes + p.slab_bytes + (h16 ? act16_staging_bytes(d->N, kin, S) : 0);
  // fused statistics: 4 (8) waves x spatial tiles partials from the kernel; a split-K plan emits them from its reduction
  // pass (one slot per block of it), which the 16-bit kernels have only for a c8 output
  const int64_t tile_slots = (int64_t)p.tz_tiles * p.ty_tiles * p.tx_tiles * p.nw, split_slots = splitk_c8_slots(S);
  r.stats_slots = p.ksplit == 1 ? tile_slots : (!h16 && d->N <= 65535 && mout <= 65535 ? split_slots : 0);
  r.stats_slots_c8 = !h16 ? 0 : (p.ksplit == 1 ? tile_slots : split_slots);
  // 16-bit kernels (c8 input, m355_conv3d_fwd_h16): in-register softmax epilogue, unsplit plans
  r.fuses_softmax = which == 0 && h16 && tuning().fuse_softmax && d->Cout <= 4 && p.ksplit == 1;
  const int32_t code = h16 ? (p.oneshot ? 6 : (p.nw == 8 ? 5 : 4)) : (p.x3 ? 7 : (p.persistent ? 3 : 1));
  r.plan_code[0] = code; r.plan_code[1] = p.ntw; r.plan_code[2] = p.gx; r.plan_code[3] = p.ksplit;
  return r;
}

// Weight gradient with both operands in c8 (m355_conv3d_bwd_weight_h16 / _c8, and the plain entry point behind a pack)
struct BwwC8Route {
  bool h16;       // a 3x3x3 / s1 / p1 descriptor in a 16-bit mode
  bool ok;        // ... whose volume fits the c8 kernel's 32-bit offsets
  bool edge;      // Cin <= 4 or Cout <= 4: tap and narrow channel share the MFMA column (conv3_bww_c8_small_kernel)
  int nsplit;
  size_t slab_bytes, h16_workspace_bytes, c8_workspace_bytes;   // slabs + scratch of the bias gradient from fp32 dy / c8 dy
};
static BwwC8Route route_bww_c8(const m355_conv3d_desc* d) {
  BwwC8Route r{};
  const int64_t S = (int64_t)d->D * d->H * d->W;
  r.h16 = is_k3s1p1(d) && is16(d->compute);
  r.ok = r.h16 && S * 64 < (1ll << 31);
  if (!r.ok) return r;
  r.edge = (d->Cin <= 4 || d->Cout <= 4) && !tuning().no_small;
  r.nsplit = bww_c8_nsplit(d);
  r.slab_bytes = (size_t)round_up((int64_t)r.nsplit * d->Cout * d->Cin * 27 * 4, 256);
  r.h16_workspace_bytes = r.slab_bytes + dbias_ws_bytes(d->Cout, S);
  r.c8_workspace_bytes = r.slab_bytes + dbias_c8_ws_bytes(d->N, d->Cout, S);
  return r;
}

BwwRoute route_bww(const m355_conv3d_desc* d) {
  BwwRoute r{};
  r.kind = BwwKind::Direct;
  const int64_t OS = out_voxels(d);
  const size_t db = dbias_ws_bytes(d->Cout, OS);
  r.workspace_bytes = db;
  if (!is_k3s1p1(d)) return r;
  const int64_t S = (int64_t)d->D * d->H * d->W;
  // M355_COMPUTE_F32X3: the weight gradient on the split kernels too (M355_F32X3=2 forces every fp32 layer there,
  // M355_F32X3_BWW=0 keeps the weight gradient on the fp32 MFMA kernels)
  const bool x3_mode = d->compute == M355_COMPUTE_F32X3 || (d->compute == M355_COMPUTE_F32 && tuning().f32x3 == 2);
  if (x3_mode && tuning().f32x3 && tuning().f32x3_bww && d->Cin > 4 && d->Cout > 4 && d->D >= 2 && S < (1ll << 24)) {
    r.kind = BwwKind::X3;
    r.x3 = plan_bww_x3(d->N, d->Cin, d->Cout, d->D, d->H, d->W);
    r.slab_bytes = r.x3.slab_bytes;
    r.workspace_bytes = r.slab_bytes + db;
    r.plan_code[0] = 8; r.plan_code[2] = r.x3.tx; r.plan_code[3] = r.x3.nsplit;
    return r;
  }
  r.plan = plan_bww(d->N, d->Cin, d->Cout, d->D, d->H, d->W);
  r.slab_bytes = r.plan.slab_bytes;
  r.workspace_bytes = r.slab_bytes + db;
  // tap-on-lane kernel; a sample must fit the 32-bit byte offsets of a buffer descriptor
  const bool small = (d->Cin <= 4 || d->Cout <= 4) && !tuning().no_small &&
                     (int64_t)std::max(d->Cin, d->Cout) * S < (1ll << 29);
  const BwwC8Route c8 = route_bww_c8(d);
  if (c8.ok && !small && d->N <= 65535) {
    // 16-bit operand mode: both operands are rounded into c8 copies that follow the c8 kernel's own workspace
    r.kind = BwwKind::H16ViaPack;
    r.workspace_bytes = std::max(r.workspace_bytes, c8.h16_workspace_bytes + act16_staging_bytes(d->N, d->Cin, S) +
                                                        act16_staging_bytes(d->N, d->Cout, S));
  } else {
    r.kind = small ? BwwKind::Small : BwwKind::Mfma2;
  }
  r.plan_code[0] = r.kind == BwwKind::H16ViaPack ? 11 : (small ? 10 : 9); r.plan_code[2] = r.plan.gx; r.plan_code[3] = r.plan.nsplit;
  return r;
}

}  // namespace m355

using namespace m355;

// ---------------------------------------------------------------------- ABI

static int validate_conv(const m355_conv3d_desc* d, const char* who) {
  M355_REQUIRE(d != nullptr, M355_EINVALID_ARG, "%s: null descriptor", who);
  M355_REQUIRE(d->N > 0 && d->Cin > 0 && d->Cout > 0 && d->D > 0 && d->H > 0 && d->W > 0,
               M355_EINVALID_ARG, "%s: non-positive dimension", who);
  M355_REQUIRE(d->k >= 1 && d->k <= 7 && d->stride >= 1 && d->pad >= 0, M355_EINVALID_ARG,
               "%s: bad k/stride/pad (%d/%d/%d)", who, d->k, d->stride, d->pad);
  M355_REQUIRE(d->compute == M355_COMPUTE_F32 || d->compute == M355_COMPUTE_BF16 || d->compute == M355_COMPUTE_F16 ||
                   d->compute == M355_COMPUTE_F32X3,
               M355_EINVALID_ARG, "%s: unknown compute mode %d", who, d->compute);
  return M355_OK;
}

// ---- queries: a number of the route ----
extern "C" size_t m355_conv3d_fwd_workspace(const m355_conv3d_desc* d) { return d ? route_conv(d, 0).workspace_bytes : 0; }
extern "C" size_t m355_conv3d_bwd_data_workspace(const m355_conv3d_desc* d) { return d ? route_conv(d, 1).workspace_bytes : 0; }
extern "C" size_t m355_conv3d_h16_workspace(const m355_conv3d_desc* d, int32_t which) {
  return d ? route_conv(d, which).h16_workspace_bytes : 0;
}
extern "C" size_t m355_conv3d_bwd_weight_workspace(const m355_conv3d_desc* d) { return d ? route_bww(d).workspace_bytes : 0; }
extern "C" size_t m355_conv3d_bwd_weight_h16_workspace(const m355_conv3d_desc* d) {
  return d ? route_bww_c8(d).h16_workspace_bytes : 0;
}
extern "C" size_t m355_conv3d_bwd_weight_c8_workspace(const m355_conv3d_desc* d) {
  return d ? route_bww_c8(d).c8_workspace_bytes : 0;
}
extern "C" size_t m355_conv3d_packed_bytes(const m355_conv3d_desc* d, int32_t which) {
  if (!d || d->N <= 0 || d->Cin <= 0 || d->Cout <= 0) return 0;
  return route_conv(d, which).packed_bytes;
}
extern "C" int64_t m355_conv3d_stats_slots(const m355_conv3d_desc* d) { return d ? route_conv(d, 0).stats_slots : 0; }
extern "C" int64_t m355_conv3d_stats_slots_c8(const m355_conv3d_desc* d) { return d ? route_conv(d, 0).stats_slots_c8 : 0; }
extern "C" int32_t m355_conv3d_fuses_softmax(const m355_conv3d_desc* d) { return d && route_conv(d, 0).fuses_softmax ? 1 : 0; }
// (the codes: include/m355seg.h; 2 = the small-Cout forward, conv3_valu_smallcout_kernel unless M355_SMALLCOUT_VALU=0)
extern "C" int m355_conv3d_plan(const m355_conv3d_desc* d, int32_t which, int32_t* out4) {
  M355_REQUIRE(d && out4, M355_EINVALID_ARG, "conv3d_plan: null pointer");
  std::copy_n(which == 2 ? route_bww(d).plan_code : route_conv(d, which).plan_code, 4, out4);
  return M355_OK;
}

// ---- forward and data gradient: checks the workspace against the route's own number and runs the route ----
static int run_conv(const ConvRoute& r, ConvCall c) {
  const m355_conv3d_desc* d = c.d;
  const size_t need = c.in16 ? r.h16_workspace_bytes : r.workspace_bytes;
  M355_REQUIRE(c.ws_bytes >= need && (c.ws || !need), M355_EWORKSPACE, "conv3d: workspace too small (%zu < %zu)",
               c.ws_bytes, need);
  if (!is_h16(r.kind)) {
    M355_REQUIRE(r.kind == ConvKind::Direct || ((uintptr_t)c.ws & 15) == 0, M355_EINVALID_ARG,
                 "conv3d: workspace not 16B aligned");
    return launch_f32_conv(r, c);
  }
  const int kin = c.transpose ? d->Cout : d->Cin, mout = c.transpose ? d->Cin : d->Cout;
  const int64_t S = (int64_t)d->D * d->H * d->W;
  if (!c.in16) {
    // fp32 NCDHW input: one conversion pass into the c8 layout (the model path hands over c8 tensors that its
    // normalisation / pooling passes wrote, m355_conv3d_fwd_h16)
    void* stage = (char*)c.ws + r.h16_workspace_bytes;
    c.in16_bs = c8_blocks(kin) * S * 8;
    if (int rc = launch_pack_act16(c.in, stage, d->N, kin, S, c.in_bs, c.in16_bs, d->compute, c.st)) return rc;
    c.in16 = stage;
  }
  return run_h16_conv(r.plan, d->compute, c.in16, c.in16_bs, c.prepacked ? nullptr : c.w, c.transpose, d->Cout, d->Cin,
                      c.bias, c.add, c.out, d->N, kin, mout, d->D, d->H, d->W, c.out_bs, c.ws, c.ws_bytes, c.st, c.stat,
                      c.prepacked ? c.w : nullptr, c.out16, c.softmax, c.oflag);
}

// the fields every entry point fills the same way
static ConvCall conv_call(const m355_conv3d_desc* d, bool transpose, const float* w, void* workspace, size_t workspace_bytes,
                          void* stream) {
  ConvCall c{};
  c.d = d; c.transpose = transpose;
  c.w = w; c.prepacked = (d->flags & M355_CONV_W_PACKED) != 0;
  c.softmax = (d->flags & M355_CONV_SOFTMAX) != 0;
  c.ws = workspace; c.ws_bytes = workspace_bytes;
  c.st = (hipStream_t)stream;
  return c;
}

static int conv3d_fwd_impl(const m355_conv3d_desc* d, const float* x, const float* w, const float* bias,
                           const float* add, float* y, float* stat, void* workspace, size_t workspace_bytes,
                           void* stream) {
  if (int rc = validate_conv(d, "conv3d_fwd")) return rc;
  const ConvRoute r = route_conv(d, 0);
  M355_REQUIRE(!(d->flags & M355_CONV_SOFTMAX) || r.fuses_softmax, M355_EUNSUPPORTED,
               "conv3d_fwd: M355_CONV_SOFTMAX needs m355_conv3d_fuses_softmax(desc) != 0");
  M355_REQUIRE(!stat || r.stats_slots > 0, M355_EINVALID_ARG,
               "conv3d_fwd_stats: this descriptor has no fused statistics (m355_conv3d_stats_slots() == 0)");
  M355_REQUIRE(x && w && y, M355_EINVALID_ARG, "conv3d_fwd: null pointer");
  const int OD = out_dim(d->D, d->k, d->stride, d->pad), OH = out_dim(d->H, d->k, d->stride, d->pad),
            OW = out_dim(d->W, d->k, d->stride, d->pad);
  M355_REQUIRE(OD > 0 && OH > 0 && OW > 0, M355_EINVALID_ARG, "conv3d_fwd: empty output");
  M355_REQUIRE(r.kind != ConvKind::Direct || !(d->flags & M355_CONV_W_PACKED), M355_EINVALID_ARG,
               "conv3d_fwd: this descriptor has no packed weights");
  ConvCall c = conv_call(d, false, w, workspace, workspace_bytes, stream);
  c.in = x; c.in_bs = dense_or(d->x_batch_stride, (int64_t)d->Cin * d->D * d->H * d->W);
  c.bias = bias; c.add = add;
  c.out = y; c.out_bs = dense_or(d->y_batch_stride, (int64_t)d->Cout * OD * OH * OW);
  c.stat = stat;
  return run_conv(r, c);
}

extern "C" int m355_conv3d_fwd(const m355_conv3d_desc* d, const float* x, const float* w,
                               const float* bias, const float* add, float* y, void* workspace,
                               size_t workspace_bytes, void* stream) {
  return conv3d_fwd_impl(d, x, w, bias, add, y, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int m355_conv3d_fwd_stats(const m355_conv3d_desc* d, const float* x, const float* w,
                                     const float* bias, const float* add, float* y, float* stat_partials,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  M355_REQUIRE(stat_partials, M355_EINVALID_ARG, "conv3d_fwd_stats: null statistics buffer");
  return conv3d_fwd_impl(d, x, w, bias, add, y, stat_partials, workspace, workspace_bytes, stream);
}

extern "C" int m355_conv3d_bwd_data(const m355_conv3d_desc* d, const float* dy, const float* w, float* dx, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  if (int rc = validate_conv(d, "conv3d_bwd_data")) return rc;
  M355_REQUIRE(dy && w && dx, M355_EINVALID_ARG, "conv3d_bwd_data: null pointer");
  const ConvRoute r = route_conv(d, 1);
  M355_REQUIRE(r.kind != ConvKind::Direct || !(d->flags & M355_CONV_W_PACKED), M355_EINVALID_ARG,
               "conv3d_bwd_data: this descriptor has no packed weights");
  const int64_t OS = out_voxels(d);
  ConvCall c = conv_call(d, true, w, workspace, workspace_bytes, stream);
  c.softmax = false;
  c.in = dy; c.in_bs = dense_or(d->y_batch_stride, (int64_t)d->Cout * OS);
  c.out = dx; c.out_bs = dense_or(d->x_batch_stride, (int64_t)d->Cin * d->D * d->H * d->W);
  return run_conv(r, c);
}

// ---- packed weights (M355_CONV_W_PACKED) ----
extern "C" int m355_conv3d_pack(const m355_conv3d_desc* d, int32_t which, const float* w, void* packed, void* stream) {
  if (int rc = validate_conv(d, "conv3d_pack")) return rc;
  M355_REQUIRE(w && packed && ((uintptr_t)packed & 15) == 0, M355_EINVALID_ARG, "conv3d_pack: null / unaligned pointer");
  const ConvRoute r = route_conv(d, which);
  M355_REQUIRE(r.kind != ConvKind::Direct && (which == 0 || which == 1), M355_EUNSUPPORTED,
               "conv3d_pack: only the 3x3x3 / stride 1 / pad 1 kernels have packed weights");
  launch_pack_weights(r, d, which == 1, w, packed, (hipStream_t)stream);
  return check_launch("conv3d_pack");
}

extern "C" int m355_conv3d_pack_batch(const m355_pack_item* items, int32_t n, void* stream) {
  M355_REQUIRE(items || n == 0, M355_EINVALID_ARG, "conv3d_pack_batch: null items");
  hipStream_t st = (hipStream_t)stream;
  PackBatch b;
  X3PackBatch b3;
  int nb = 0, nb3 = 0;
  for (int i = 0; i < n; ++i) {
    const m355_pack_item& it = items[i];
    const m355_conv3d_desc* d = &it.desc;
    if (int rc = validate_conv(d, "conv3d_pack_batch")) return rc;
    M355_REQUIRE(it.w && it.packed && ((uintptr_t)it.packed & 15) == 0, M355_EINVALID_ARG,
                 "conv3d_pack_batch: item %d: null / unaligned pointer", i);
    const ConvRoute r = route_conv(d, it.which);
    const FwdPlan& p = r.plan;
    M355_REQUIRE(r.kind != ConvKind::Direct && (it.which == 0 || it.which == 1), M355_EUNSUPPORTED,
                 "conv3d_pack_batch: item %d: only the 3x3x3 / stride 1 / pad 1 kernels have packed weights", i);
    if (r.kind == ConvKind::SmallCoutValu || r.kind == ConvKind::SmallCoutToeplitz) {
      launch_pack_weights(r, d, false, it.w, it.packed, st);   // (the Cout <= 4 forward layouts: one per model, launched on its own)
      continue;
    }
    if (r.kind == ConvKind::X3) {   // split + fragment-ordered weights: a batch of their own
      X3PackEntry& e = b3.e[nb3++];
      e.w = it.w; e.wq = it.packed;
      e.Cout = d->Cout; e.Cin = d->Cin;
      e.nchunks = p.nchunks; e.otiles = p.otiles; e.tile16 = p.tile16;
      e.transpose = it.which == 1;
      if (nb3 == PACK_BATCH) {
        launch_pack_x3_batch(b3, nb3, st);
        nb3 = 0;
      }
      continue;
    }
    const int kind = !is_h16(r.kind) ? 0 : (d->compute == M355_COMPUTE_BF16 ? 1 : 2);
    if (nb && (kind == 0) != (b.e[0].kind == 0)) {   // a launch holds fp32 entries or 16-bit entries, not both
      launch_pack_batch(b, nb, st);
      nb = 0;
    }
    PackEntry& e = b.e[nb++];
    e.w = it.w; e.wp = it.packed;
    e.counter = (int*)((char*)it.packed + p.wp_bytes - 256);
    e.Cout = d->Cout; e.Cin = d->Cin;
    e.kdim = kind == 0 ? p.kin_pad : p.nchunks;
    e.mout_pad = p.mout_pad;
    e.transpose = it.which == 1; e.kind = kind;
    if (nb == PACK_BATCH) {
      launch_pack_batch(b, nb, st);
      nb = 0;
    }
  }
  if (nb) launch_pack_batch(b, nb, st);
  if (nb3) launch_pack_x3_batch(b3, nb3, st);
  return check_launch("conv3d_pack_batch");
}

// ---- 16-bit operand modes with c8 tensors handed over by the caller (h16.hpp) ----
extern "C" size_t m355_act16_bytes(int32_t N, int32_t C, int64_t S) {
  if (N <= 0 || C <= 0 || S <= 0) return 0;
  return (size_t)N * (size_t)c8_blocks(C) * (size_t)S * 16;
}

static int validate_act16(const char* who, const void* a, const void* b, int N, int C, int64_t S, int compute) {
  M355_REQUIRE(a && b, M355_EINVALID_ARG, "%s: null pointer", who);
  M355_REQUIRE(N > 0 && C > 0 && S > 0 && N <= 65535 && c8_blocks(C) <= 65535, M355_EINVALID_ARG, "%s: bad shape", who);
  M355_REQUIRE(compute == M355_COMPUTE_BF16 || compute == M355_COMPUTE_F16, M355_EINVALID_ARG,
               "%s: compute must be M355_COMPUTE_BF16 or M355_COMPUTE_F16", who);
  return M355_OK;
}

extern "C" int m355_act16_pack(const float* x, void* x16, int32_t N, int32_t C, int64_t S, int64_t x_batch_stride,
                               int64_t x16_batch_stride, int32_t compute, void* stream) {
  if (int rc = validate_act16("act16_pack", x, x16, N, C, S, compute)) return rc;
  M355_REQUIRE(((uintptr_t)x16 & 15) == 0 && x16_batch_stride % 8 == 0, M355_EINVALID_ARG, "act16_pack: c8 tensor not 16B aligned");
  return launch_pack_act16(x, x16, N, C, S, dense_or(x_batch_stride, (int64_t)C * S),
                           dense_or(x16_batch_stride, c8_blocks(C) * S * 8), compute, (hipStream_t)stream);
}

extern "C" int m355_act16_unpack(const void* x16, float* x, int32_t N, int32_t C, int64_t S, int64_t x16_batch_stride,
                                 int64_t x_batch_stride, int32_t compute, void* stream) {
  if (int rc = validate_act16("act16_unpack", x16, x, N, C, S, compute)) return rc;
  M355_REQUIRE(((uintptr_t)x16 & 15) == 0 && x16_batch_stride % 8 == 0, M355_EINVALID_ARG, "act16_unpack: c8 tensor not 16B aligned");
  return launch_unpack_act16(x16, x, N, C, S, dense_or(x16_batch_stride, c8_blocks(C) * S * 8),
                             dense_or(x_batch_stride, (int64_t)C * S), compute, (hipStream_t)stream);
}

// Validates the descriptor of a c8 entry point and resolves its route.
static int resolve_h16(const m355_conv3d_desc* d, int which, const char* who, ConvRoute* r) {
  if (int rc = validate_conv(d, who)) return rc;
  *r = route_conv(d, which);
  M355_REQUIRE(is_h16(r->kind), M355_EUNSUPPORTED,
               "%s: c8 input is only defined for the 3x3x3 / stride 1 / pad 1 kernels in a 16-bit compute mode", who);
  return M355_OK;
}

// forward from a c8 x: fp32 y with optional residual / softmax, or (out16) a c8 y
static int fwd_h16(const char* who, const m355_conv3d_desc* d, const void* x16, int64_t x16_batch_stride, const float* w,
                   const float* bias, const float* add, void* y, int64_t y_bs, bool out16, float* stat, void* workspace,
                   size_t workspace_bytes, void* stream) {
  ConvRoute r;
  if (int rc = resolve_h16(d, 0, who, &r)) return rc;
  M355_REQUIRE(x16 && w && y && workspace, M355_EINVALID_ARG, "%s: null pointer", who);
  M355_REQUIRE(!stat || (out16 ? r.stats_slots_c8 : r.stats_slots) > 0, M355_EINVALID_ARG,
               "%s: this descriptor has no fused statistics (m355_conv3d_stats_slots%s() == 0)", who, out16 ? "_c8" : "");
  ConvCall c = conv_call(d, false, w, workspace, workspace_bytes, stream);
  c.softmax = c.softmax && !out16;
  M355_REQUIRE(!c.softmax || r.fuses_softmax, M355_EUNSUPPORTED,
               "%s: M355_CONV_SOFTMAX needs m355_conv3d_fuses_softmax(desc) != 0", who);
  const int64_t S = (int64_t)d->D * d->H * d->W;
  c.in16 = x16; c.in16_bs = dense_or(x16_batch_stride, c8_blocks(d->Cin) * S * 8);
  c.bias = bias; c.add = add;
  c.out = (float*)y; c.out_bs = dense_or(y_bs, out16 ? c8_blocks(d->Cout) * S * 8 : (int64_t)d->Cout * S);
  c.out16 = out16;
  c.stat = stat;
  return run_conv(r, c);
}

extern "C" int m355_conv3d_fwd_h16(const m355_conv3d_desc* d, const void* x16, int64_t x16_batch_stride, const float* w,
                                   const float* bias, const float* add, float* y, float* stat_partials, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  return fwd_h16("conv3d_fwd_h16", d, x16, x16_batch_stride, w, bias, add, y, d ? d->y_batch_stride : 0, false, stat_partials,
                 workspace, workspace_bytes, stream);
}

extern "C" int m355_conv3d_fwd_h16_c8(const m355_conv3d_desc* d, const void* x16, int64_t x16_batch_stride,
                                      const float* w, const float* bias, void* y16, int64_t y16_batch_stride,
                                      float* stat_partials, void* workspace, size_t workspace_bytes, void* stream) {
  return fwd_h16("conv3d_fwd_h16_c8", d, x16, x16_batch_stride, w, bias, nullptr, y16, y16_batch_stride, true, stat_partials,
                 workspace, workspace_bytes, stream);
}

// data gradient from a c8 dy: fp32 dx, or (dx16_c8, the c8-only training flow) a c8 dx whose fp16 stores report overflow
static int bwd_data_h16(const char* who, const m355_conv3d_desc* d, const void* dy16, int64_t dy16_batch_stride,
                        const float* w, void* dx, int64_t dx_bs, bool dx16_c8, void* workspace, size_t workspace_bytes,
                        void* stream) {
  ConvRoute r;
  if (int rc = resolve_h16(d, 1, who, &r)) return rc;
  M355_REQUIRE(dy16 && w && dx && workspace, M355_EINVALID_ARG, "%s: null pointer", who);
  ConvCall c = conv_call(d, true, w, workspace, workspace_bytes, stream);
  c.softmax = false;
  c.in16 = dy16; c.in16_bs = dense_or(dy16_batch_stride, c8_blocks(d->Cout) * (int64_t)d->D * d->H * d->W * 8);
  c.out = (float*)dx;
  c.out_bs = dense_or(dx_bs, (dx16_c8 ? c8_blocks(d->Cin) * 8 : (int64_t)d->Cin) * d->D * d->H * d->W);
  c.out16 = dx16_c8;
  c.oflag = dx16_c8 && d->compute == M355_COMPUTE_F16 ? overflow_flag() : nullptr;
  return run_conv(r, c);
}

extern "C" int m355_conv3d_bwd_data_h16(const m355_conv3d_desc* d, const void* dy16, int64_t dy16_batch_stride,
                                        const float* w, float* dx, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  return bwd_data_h16("conv3d_bwd_data_h16", d, dy16, dy16_batch_stride, w, dx, d ? d->x_batch_stride : 0, false, workspace,
                      workspace_bytes, stream);
}

extern "C" int m355_conv3d_bwd_data_h16_c8(const m355_conv3d_desc* d, const void* dy16, int64_t dy16_batch_stride,
                                           const float* w, void* dx16, int64_t dx16_batch_stride, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  return bwd_data_h16("conv3d_bwd_data_h16_c8", d, dy16, dy16_batch_stride, w, dx16, dx16_batch_stride, true, workspace,
                      workspace_bytes, stream);
}

// ---- weight gradient with both operands in c8 (the 16-bit training flow keeps the packed conv input of the forward
// pass and packs dy once for the data and the weight gradient).  One body for m355_conv3d_bwd_weight_h16 (bias gradient
// from the fp32 dy) and, `c8_flow`, m355_conv3d_bwd_weight_c8 (the c8-only training flow: edge-layer kernel, bias
// gradient reduced from the c8 dy, the loss scale of the fp16 mode removed in the fp32 epilogue by grad_unscale) ----
static int bww_c8_impl(const char* who, bool c8_flow, const m355_conv3d_desc* d, const void* x16, int64_t x16_batch_stride,
                       const void* dy16, int64_t dy16_batch_stride, const float* dy, float* dw, float* dbias,
                       float grad_unscale, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = validate_conv(d, who)) return rc;
  const BwwC8Route r = route_bww_c8(d);
  M355_REQUIRE(r.h16, M355_EUNSUPPORTED,
               "%s: c8 input is only defined for the 3x3x3 / stride 1 / pad 1 kernels in a 16-bit compute mode", who);
  M355_REQUIRE(x16 && dy16 && dw && workspace, M355_EINVALID_ARG, "%s: null pointer", who);
  M355_REQUIRE(r.ok, M355_EUNSUPPORTED, "%s: volume too large for the c8 kernel (>= 2^25 voxels)", who);
  M355_REQUIRE(c8_flow || !dbias || dy, M355_EINVALID_ARG, "%s: the bias gradient needs the fp32 dy", who);
  const size_t need = c8_flow ? r.c8_workspace_bytes : r.h16_workspace_bytes;
  M355_REQUIRE(workspace_bytes >= need, M355_EWORKSPACE, "%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
  const int64_t S = (int64_t)d->D * d->H * d->W;
  const int64_t xbs = dense_or(x16_batch_stride, c8_blocks(d->Cin) * S * 8);
  const int64_t ybs = dense_or(dy16_batch_stride, c8_blocks(d->Cout) * S * 8);
  M355_REQUIRE((((uintptr_t)x16 | (uintptr_t)dy16) & 15) == 0 && xbs % 8 == 0 && ybs % 8 == 0, M355_EINVALID_ARG,
               "%s: c8 tensor not 16B aligned", who);
  hipStream_t st = (hipStream_t)stream;
  float* slab = (float*)workspace;
  if (int rc = (c8_flow && r.edge ? launch_bww_c8_small : launch_bww_c8)(d->compute, x16, dy16, slab, d->N, d->Cin, d->Cout,
                                                                       d->D, d->H, d->W, r.nsplit, xbs, ybs, st))
    return rc;
  BwwClasses kred{};
  kred.of = (int)ceil_div(d->Cout, 32);
  kred.cf = (int)ceil_div(d->Cin, 32);
  for (int c = 0; c < 4; ++c) kred.ns[c] = r.nsplit;
  launch_slab_reduce_t(slab, dw, d->Cin, d->Cout, kred.cf, kred, grad_unscale, st);
  void* dbias_ws = (char*)workspace + r.slab_bytes;
  if (dbias && c8_flow) {
    if (int rc = launch_dbias_c8(dy16, ybs, dbias, d->N, d->Cout, S, d->compute, grad_unscale, dbias_ws, st)) return rc;
  } else if (dbias) {
    launch_dbias(dy, dbias, d->N, d->Cout, S, dense_or(d->y_batch_stride, (int64_t)d->Cout * S), dbias_ws, st);
  }
  return check_launch(who);
}

extern "C" int m355_conv3d_bwd_weight_h16(const m355_conv3d_desc* d, const void* x16, int64_t x16_batch_stride,
                                          const void* dy16, int64_t dy16_batch_stride, const float* dy, float* dw,
                                          float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
  return bww_c8_impl("conv3d_bwd_weight_h16", false, d, x16, x16_batch_stride, dy16, dy16_batch_stride, dy, dw, dbias, 1.f,
                     workspace, workspace_bytes, stream);
}

extern "C" int m355_conv3d_bwd_weight_c8(const m355_conv3d_desc* d, const void* x16, int64_t x16_batch_stride,
                                         const void* dy16, int64_t dy16_batch_stride, float* dw, float* dbias,
                                         float grad_unscale, void* workspace, size_t workspace_bytes, void* stream) {
  return bww_c8_impl("conv3d_bwd_weight_c8", true, d, x16, x16_batch_stride, dy16, dy16_batch_stride, nullptr, dw, dbias,
                     grad_unscale, workspace, workspace_bytes, stream);
}

// ---- weight gradient from fp32 NCDHW operands ----
extern "C" int m355_conv3d_bwd_weight(const m355_conv3d_desc* d, const float* x, const float* dy, float* dw, float* dbias,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = validate_conv(d, "conv3d_bwd_weight")) return rc;
  M355_REQUIRE(x && dy && dw, M355_EINVALID_ARG, "conv3d_bwd_weight: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int64_t S = (int64_t)d->D * d->H * d->W;
  const int64_t OS = out_voxels(d);
  const int64_t xbs = dense_or(d->x_batch_stride, (int64_t)d->Cin * S);
  const int64_t ybs = dense_or(d->y_batch_stride, (int64_t)d->Cout * OS);
  const BwwRoute r = route_bww(d);
  M355_REQUIRE(workspace && workspace_bytes >= r.workspace_bytes, M355_EWORKSPACE,
               "conv3d_bwd_weight: workspace too small (%zu < %zu)", workspace_bytes, r.workspace_bytes);
  M355_REQUIRE(r.kind == BwwKind::Direct || r.kind == BwwKind::X3 ||
                   ((int64_t)d->Cin * S < (1ll << 31) && (int64_t)d->Cout * S < (1ll << 31)),
               M355_EUNSUPPORTED, "conv3d_bwd_weight: tensor exceeds 2^31 elements per sample");
  if (r.kind == BwwKind::H16ViaPack) {
    // fp32 NCDHW operands in a 16-bit compute mode (the model path hands over c8 tensors through
    // m355_conv3d_bwd_weight_h16 / _c8): both operands are rounded into c8 copies and the c8 kernel runs
    const size_t hws = route_bww_c8(d).h16_workspace_bytes;
    char* x16 = (char*)workspace + hws;
    char* dy16 = x16 + act16_staging_bytes(d->N, d->Cin, S);
    if (int rc = launch_pack_act16(x, x16, d->N, d->Cin, S, xbs, c8_blocks(d->Cin) * S * 8, d->compute, st)) return rc;
    if (int rc = launch_pack_act16(dy, dy16, d->N, d->Cout, S, ybs, c8_blocks(d->Cout) * S * 8, d->compute, st)) return rc;
    m355_conv3d_desc dd = *d;
    dd.y_batch_stride = ybs;
    return m355_conv3d_bwd_weight_h16(&dd, x16, 0, dy16, 0, dbias ? dy : nullptr, dw, dbias, workspace, hws, stream);
  }
  if (int rc = launch_f32_bww(r, d, x, dy, dw, (float*)workspace, xbs, ybs, st)) return rc;
  if (dbias) launch_dbias(dy, dbias, d->N, d->Cout, OS, ybs, (char*)workspace + r.slab_bytes, st);   // its scratch follows the slabs
  return check_launch("conv3d_bwd_weight");
}
