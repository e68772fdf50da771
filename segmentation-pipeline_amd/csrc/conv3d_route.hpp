// Host half of the 3x3x3 convolution family (conv3d.hip: fp32 kernels; conv3d_f32x3.hip: split kernels; conv3d_h16.hip:
// bf16 / fp16 operand kernels).  Pure host code: the planners, ONE route per call -- route_conv (forward / data gradient),
// route_bww and route_bww_c8 (weight gradients) -- and ONE check per entry-point group (check_conv, check_bww) that runs
// every argument check before the first launch.  A route fixes the kernel variant, every grid and block size, the
// auxiliary launches and the workspace layout; the queries return a route's numbers, m355_conv3d_launch_plan reports them,
// the launchers in the kernel files start what the route says.  Nothing else decides.
#pragma once
#include "h16.hpp"

namespace m355 {

inline bool is16(int compute) { return compute == M355_COMPUTE_BF16 || compute == M355_COMPUTE_F16; }
inline int out_dim(int in, int k, int s, int p) { return (in + 2 * p - k) / s + 1; }
// blocks along the voxel axis of splitk_reduce_c8_kernel == statistics slots it emits per sample
inline int64_t splitk_c8_slots(int64_t S) { return std::max<int64_t>(1, std::min<int64_t>(ceil_div(S, 256), 2048)); }
// tile constants of the two Cout <= 4 forward kernels (conv3d.hip asserts that its kernels use the same)
constexpr int SMALLCOUT_TZ_K = 90, SMALLCOUT_VS_TZ = 4, SMALLCOUT_VS_TY = 8, SMALLCOUT_VS_TX = 64;
inline size_t smallcout_packed_bytes(int Cin) { return (size_t)round_up((int64_t)round_up(Cin, 2) * SMALLCOUT_TZ_K * 32 * 4, 256); }

// ------------------------------------------------------------------ plans
struct FwdPlan {
  bool mfma;
  bool persistent;  // more items than resident workgroups: the queue-driven kernel variants
  int gx, ntw;
  int tz_tiles, ty_tiles, tx_tiles;
  int otiles, kin_pad, mout_pad, nchunks, ksplit;   // otiles: 32-row output tiles
  int tile16;       // + one 16-row remainder tile at channel 32 * otiles (fp32 path, mout % 32 in 1..16)
  int nw;           // waves per workgroup = z slices of a tile: 4, or 8 (16-bit kernels, double-buffered variant)
  int oneshot;      // 16-bit kernels: one item per workgroup instead of the work queue (items of 1-2 chunks)
  int x3;           // M355_COMPUTE_F32X3 and the layer qualifies: conv3_f32x3_kernel (conv3d_f32x3.hip), 8-channel chunks
  int64_t slots;    // resident workgroups of the queue-driven kernels (LDS + registers: 2 per CU up to NTW = 4)
  size_t wp_bytes, slab_bytes;
};
// pair classes of a weight gradient whose channel counts leave a 1..16 channel remainder (conv3_mfma_bww2c_kernel,
// conv3_bww_x3c_kernel)
struct BwwClasses {
  int of, cf, orem, crem;   // full 32-channel tiles per side, and whether a 16-row remainder tile follows them
  int ns[4];                // voxel-range splits of a pair of class (o remainder ? 2 : 0) + (c remainder ? 1 : 0)
  int start[4];             // first workgroup of each class
};
struct BwwPlan {
  int gx, tz_tiles, ty_tiles, tx_tiles, otiles, ctiles, nsplit;
  size_t slab_bytes;
  bool classes;     // a 1..16 channel remainder on either side: conv3_mfma_bww2c_kernel (needs the gen-2 conditions)
  BwwClasses k;     // always filled: without remainders one class with ns[*] = nsplit
  int class_wgs;    // grid of the class kernel
};
// the split kernels' weight gradient (conv3_bww_x3_kernel / conv3_bww_x3c_kernel): slab[split][27][Cout][Cin] partials
struct BwwX3Plan {
  int tx, ty_tiles, tx_tiles, ctiles, otiles, nsplit;
  bool classes;     // a 1..16 channel remainder on either side: the class kernel
  BwwClasses k;     // always filled: without remainders one class with ns[*] = nsplit
  int class_wgs;
  size_t slab_bytes;
};

// ------------------------------------------------------------------ planning
// Lanes along x per 32-voxel group: the widest of {32, 16, 8} unless a narrower one wastes noticeably
// fewer padded voxels (W = 24: 16 -> 2 tiles = 32 columns, 8 -> 3 tiles = 24 columns).
static inline int pick_gx(int W) {
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
static inline bool x3_layer(int kin, int mout, int D, int H, int W) {
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
static inline TilePick pick_f32(const FwdPlan& p, int N, int H, int64_t out_bytes) {
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
static inline TilePick pick_x3(const FwdPlan& p, int N, int H, int64_t out_bytes) {
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
static inline TilePick pick_h16_oneshot(const FwdPlan& p, int N, int H, int64_t out_bytes) {
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
static inline TilePick pick_h16_queue(FwdPlan& p, int N, int D, int H, int64_t out_bytes) {
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
static inline FwdPlan plan_mfma(int N, int kin, int mout, int D, int H, int W, int compute) {
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
  p.slots = (tuning().conv_slots ? tuning().conv_slots : (p.nw == 8 ? 1 : (p.ntw <= 4 ? 2 : 1)) * num_cus());
  const int64_t slots = p.slots;
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

// Pair classes of a weight gradient with a 1..16 channel remainder on either side (k.of / cf / orem / crem filled): the
// split count of a class is proportional to the MFMA cost of its pairs (`cost`, in units of a full 32 x 32 pair), starting
// from `base` splits of a full pair and scaled down until the launch fits `budget` workgroups -- the rounding of the
// per-class counts must not spill a workgroup into another residency.  Fills k.ns / k.start and the grid; returns the
// largest split count of a populated class.
static inline int64_t split_pair_classes(BwwClasses& k, const double (&cost)[4], int64_t ntiles, int64_t budget, double base,
                                         int* class_wgs) {
  const int64_t npairs[4] = {(int64_t)k.of * k.cf, (int64_t)k.of * k.crem, (int64_t)k.orem * k.cf, (int64_t)k.orem * k.crem};
  int64_t max_ns;
  for (;;) {
    int wg = 0;
    max_ns = 1;
    for (int c = 0; c < 4; ++c) {
      const int64_t ns = std::max<int64_t>(1, std::min<int64_t>(ntiles, (int64_t)(base * cost[c] + 0.5)));
      k.ns[c] = npairs[c] ? (int)ns : 1;
      k.start[c] = wg;
      wg += (int)(npairs[c] * k.ns[c]);
      if (npairs[c]) max_ns = std::max<int64_t>(max_ns, ns);
    }
    *class_wgs = wg;
    if (wg <= budget || base <= 1.0 || tuning().bww_nsplit) return max_ns;
    base *= 0.99;
  }
}
static inline double pair_class_units(const BwwClasses& k, const double (&cost)[4]) {
  return cost[0] * (double)((int64_t)k.of * k.cf) + cost[1] * (double)((int64_t)k.of * k.crem) +
         cost[2] * (double)((int64_t)k.orem * k.cf) + cost[3] * (double)((int64_t)k.orem * k.crem);
}
static inline void fill_pair_classes(BwwClasses& k, int Cin, int Cout, int ctiles, int otiles) {
  const auto rem16 = [](int c) { return c % 32 >= 1 && c % 32 <= 16 ? 1 : 0; };
  k.orem = tuning().tile16 ? rem16(Cout) : 0;
  k.crem = tuning().tile16 ? rem16(Cin) : 0;
  k.of = otiles - k.orem;
  k.cf = ctiles - k.crem;
}

static inline BwwPlan plan_bww(int N, int Cin, int Cout, int D, int H, int W) {
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
  fill_pair_classes(p.k, Cin, Cout, p.ctiles, p.otiles);
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
    // splits of a full pair: one residency of the chip (one workgroup per CU), never more splits than tiles
    const double cost[4] = {1.0, 0.5, 0.5, 0.25};
    double base = std::min((double)ntiles, (double)cus / pair_class_units(p.k, cost));
    if (const int force = tuning().bww_nsplit) base = (double)std::min<int64_t>(force, std::max<int64_t>(1, ntiles));
    max_ns = split_pair_classes(p.k, cost, ntiles, cus, base, &p.class_wgs);
    max_ns = std::max<int64_t>(max_ns, nsplit);   // the uniform plan stays usable (generic kernel when W % 4 != 0)
  }
  p.slab_bytes = (size_t)round_up(max_ns * Cout * Cin * 27 * 4, 256);
  return p;
}

// tile width of the split kernels' weight gradient: the padded volume decides (ties: the wider tile, whose rows coalesce better)
static inline int bww_x3_tx(int H, int W) {
  int best = 32;
  int64_t best_v = -1;
  for (int tx : {32, 16, 8}) {
    const int ty = 64 / tx;
    const int64_t v = round_up(W, tx) * round_up(H, ty);
    if (best_v < 0 || v < best_v) best = tx, best_v = v;
  }
  return best;
}

static inline BwwX3Plan plan_bww_x3(int N, int Cin, int Cout, int D, int H, int W) {
  BwwX3Plan p{};
  p.tx = bww_x3_tx(H, W);
  p.ty_tiles = (int)ceil_div(H, 64 / p.tx);
  p.tx_tiles = (int)ceil_div(W, p.tx);
  p.ctiles = (int)ceil_div(Cin, 32);
  p.otiles = (int)ceil_div(Cout, 32);
  const int64_t ntiles = (int64_t)N * p.ty_tiles * p.tx_tiles * D;
  fill_pair_classes(p.k, Cin, Cout, p.ctiles, p.otiles);
  p.classes = p.k.orem || p.k.crem;
  // cost of a tile of each pair class in units of a full 32 x 32 pair (the (16, 16) class is bound by its staging)
  const double cost[4] = {1.0, 0.5, 0.5, 0.35};
  const double units = pair_class_units(p.k, cost);
  const int cus = num_cus();
  // one workgroup per CU: time ~ residencies x (tiles per split x ~3.5 us + ~10 us of cold start and slab write) + the
  // slab traffic (written here, read by the reduction)
  const double slab_us = 2.0 * (double)Cout * Cin * 27 * 4 / 4.0e6;   // per split
  int64_t cand[32];
  int nc = 0;
  for (int64_t ns = 1; ns < ntiles && nc < 20; ns *= 2) cand[nc++] = ns;
  for (int r = 1; r <= 6; ++r) cand[nc++] = std::max<int64_t>(1, (int64_t)((double)cus * r / units));
  cand[nc++] = std::max<int64_t>(1, ntiles);
  std::sort(cand, cand + nc);
  double best = 1e30;
  int64_t nsplit = 1;
  for (int i = 0; i < nc; ++i) {
    const int64_t ns = std::min<int64_t>(cand[i], std::max<int64_t>(1, ntiles));
    if (ns * Cout * Cin * 27 * 4 > (256ll << 20) && ns > 1) continue;
    const double rounds = std::ceil(units * (double)ns / (double)cus - 1e-9);
    const double cost_us = rounds * ((double)ceil_div(ntiles, ns) * 4.0 + 10.0) + (double)ns * slab_us;
    if (cost_us < best * 0.97) {
      best = cost_us;
      nsplit = ns;
    }
  }
  if (const int force = tuning().bww_nsplit) nsplit = std::min<int64_t>(force, std::max<int64_t>(1, ntiles));
  p.nsplit = (int)nsplit;
  int64_t max_ns = nsplit;
  for (int c = 0; c < 4; ++c) p.k.ns[c] = p.nsplit;
  if (p.classes) {
    // every workgroup of the launch lasts about equally long, within the residencies the uniform count needs
    const double base = (double)nsplit;
    const int64_t budget = (int64_t)std::ceil(units * base / (double)cus - 1e-9) * cus;
    max_ns = split_pair_classes(p.k, cost, ntiles, budget, base, &p.class_wgs);
  }
  p.slab_bytes = (size_t)round_up(max_ns * Cout * Cin * 27 * 4, 256);
  return p;
}

static inline int bww_c8_nsplit(const m355_conv3d_desc* d) {
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

// ------------------------------------------------------------------ what a call adds to its descriptor
// The ten launching entry points, in the order m355_conv3d_launch_plan numbers them.
enum ConvEntry {
  CE_FWD, CE_FWD_STATS, CE_BWD_DATA, CE_BWD_WEIGHT, CE_FWD_H16, CE_FWD_H16_C8, CE_BWD_DATA_H16, CE_BWD_DATA_H16_C8,
  CE_BWD_WEIGHT_H16, CE_BWD_WEIGHT_C8, CE_COUNT
};
// A call as its entry point takes it.  Pointers are integers here: they are compared with zero and masked, never followed.
struct ConvArgs {
  int entry;           // ConvEntry: fp32 or c8 input, fp32 or c8 output, the c8-only training flow
  uintptr_t in;        // x | dy | x16 | dy16: the first operand
  uintptr_t w;         // the weights (weight gradients: the second operand, dy | dy16)
  uintptr_t bias;      // (m355_conv3d_bwd_weight_h16: the fp32 dy its bias gradient reads)
  uintptr_t add;
  uintptr_t out;       // y | dx | dw
  uintptr_t stat;      // statistics partials (weight gradients: dbias)
  uintptr_t ws;
  size_t ws_bytes;
  int64_t bs[2];       // the batch strides that are arguments (c8 entry points): first operand, then c8 output | dy16; 0 = dense
};
inline bool conv_entry_c8_in(int e) { return e >= CE_FWD_H16 && e != CE_BWD_WEIGHT_H16 && e != CE_BWD_WEIGHT_C8; }
inline bool conv_entry_c8_out(int e) { return e == CE_FWD_H16_C8 || e == CE_BWD_DATA_H16_C8; }
inline bool conv_entry_dgrad(int e) { return e == CE_BWD_DATA || e == CE_BWD_DATA_H16 || e == CE_BWD_DATA_H16_C8; }
// the facts of a query: everything aligned, everything optional absent
inline ConvArgs conv_query_args(int which) {
  ConvArgs a{};
  a.entry = which == 0 ? CE_FWD : (which == 2 ? CE_BWD_WEIGHT : CE_BWD_DATA);
  return a;
}

enum ConvAux : uint32_t {   // the launches of a route besides the main kernel
  AUX_PACK_W = 1,           // weight pack (no M355_CONV_W_PACKED)
  AUX_PACK_IN = 2,          // fp32 operand -> c8 staging copy (16-bit modes, fp32 entry points)
  AUX_PACK_DY = 4,          //   ... the second operand of the weight gradient
  AUX_TILE16 = 8,           // 16-row remainder tile
  AUX_SPLITK = 16,          // split-K reduction ...
  AUX_SPLITK_STATS = 32,    //   ... that also emits the statistics partials
  AUX_SLAB_T = 64,          // slab reduction of a weight gradient: transposed (slab_reduce_t_kernel),
  AUX_SLAB_TAP = 128,       //   per tap (slab_reduce_tap_kernel),
  AUX_SLAB_PLAIN = 256,     //   plain (slab_reduce_kernel)
  AUX_DBIAS_F32 = 512,      // bias gradient from the fp32 dy,
  AUX_DBIAS_C8 = 1024       //   from the c8 dy
};

// ------------------------------------------------------------------ forward / data gradient
enum class ConvKind {   // one enumerator per kernel template family
  Direct,             // not 3x3x3 / s1 / p1 (or >= 2^27 voxels): conv3d_direct_*_kernel
  MfmaF32,            // conv3_mfma_fwd_kernel, one tile per workgroup
  MfmaF32Queue,       // conv3_mfma_fwd_p_kernel
  SmallCoutValu,      // Cout <= 4 forward: conv3_valu_smallcout_kernel (optional softmax epilogue)
  SmallCoutToeplitz,  //   ... conv3_mfma_fwd_smallcout_kernel (M355_SMALLCOUT_VALU=0)
  X3,                 // conv3_f32x3_kernel
  H16Queue, H16Queue8, H16OneShot,  // conv3_h16_kernel: queue-driven, its 8-wave variant, one item per workgroup
  H16C4,              // conv3_c4_h16_kernel: <= 4 K-channels into a c8 output
  H16Cout4            // conv3_cout4_h16_kernel: <= 4 M-channels, fp32 output, optional softmax
};
inline bool is_h16(ConvKind k) { return k >= ConvKind::H16Queue; }
inline bool is_smallcout(ConvKind k) { return k == ConvKind::SmallCoutValu || k == ConvKind::SmallCoutToeplitz; }

struct ConvRoute {
  ConvKind kind;
  FwdPlan plan;               // the MFMA kinds (MfmaF32, MfmaF32Queue, X3, H16*)
  // numbers of the descriptor alone: the queries
  size_t packed_bytes;        // m355_conv3d_packed_bytes
  size_t workspace_bytes;     // fp32 NCDHW input (16-bit modes: + the c8 staging copy)
  size_t h16_workspace_bytes; // c8 input handed over by the caller
  int64_t stats_slots, stats_slots_c8;   // fused statistics partials per (sample, channel): fp32 / c8 output; 0 = none
  bool fuses_softmax;         // ... and m355_conv3d_fuses_sigmoid: one epilogue slot, either head
  int32_t plan_code[4];       // m355_conv3d_plan
  // the call
  bool transpose;             // data gradient: flipped / transposed filter, K-channels = Cout
  bool prepacked, out16, softmax, sigmoid;
  int head;                   // kernel argument of the epilogue: 0 none, 1 softmax, 2 sigmoid
  int kin, mout;
  int64_t in_bs, in16_bs, out_bs;   // elements between samples: fp32 input, c8 input (the staging copy: dense), output
  dim3 grid;                  // main launch; grid.x == 0: none (every channel of a <= 16 channel output is on the 16-row tile)
  int block;
  dim3 grid16;                // AUX_TILE16
  dim3 reduce_grid;           // AUX_SPLITK
  int sched, order;           // scheduling arguments of the kernel: item order (fp32 / split: `sched`), 16-bit: XCD spread | stagger, item order
  uint32_t aux;               // ConvAux
  size_t slab_off, stage_off; // workspace layout: packed weights at 0, split-K slabs, the c8 staging copy
  size_t need;                // workspace bytes this call is checked against
};

// The MFMA kernels: 3x3x3, stride 1, padding 1, and a volume whose 4-channel slab fits the 32-bit byte
// offsets of a buffer descriptor (< 2^27 voxels, i.e. below 512^3); anything else takes the generic
// direct kernels (64-bit indexing).
static inline bool is_k3s1p1(const m355_conv3d_desc* d) {
  return d->k == 3 && d->stride == 1 && d->pad == 1 && (int64_t)d->D * d->H * d->W < (1ll << 27);
}
// Cout <= 4 forward in exact fp32: packed rows instead of a mostly-empty 32-row tile
static inline bool small_cout_fwd(const m355_conv3d_desc* d) {
  return d->Cout <= 4 && !is16(d->compute) && d->W >= 32 && d->D >= 8 && d->Cin >= 8 &&
         !tuning().no_small && (int64_t)std::max(d->Cin, d->Cout) * d->D * d->H * d->W < (1ll << 31);
}
// bytes of the c8 staging copy the fp32-input entry points make in 16-bit operand modes
static inline size_t act16_staging_bytes(int N, int C, int64_t S) { return (size_t)round_up((int64_t)N * c8_blocks(C) * S * 16, 256); }
static inline int64_t out_voxels(const m355_conv3d_desc* d) {
  return (int64_t)out_dim(d->D, d->k, d->stride, d->pad) * out_dim(d->H, d->k, d->stride, d->pad) * out_dim(d->W, d->k, d->stride, d->pad);
}
static inline size_t dbias_ws_bytes(int Cout, int64_t S) {
  return (size_t)round_up((int64_t)Cout * ceil_div(S, DBIAS_CHUNK) * 8, 256);
}

static inline ConvRoute route_conv(const m355_conv3d_desc* d, const ConvArgs& a) {
  ConvRoute r{};
  r.kind = ConvKind::Direct;
  r.block = 256;
  r.grid16 = r.reduce_grid = dim3(0, 0, 0);
  const bool dgrad = conv_entry_dgrad(a.entry), in16 = conv_entry_c8_in(a.entry);
  const int64_t S = (int64_t)d->D * d->H * d->W, OS = out_voxels(d);
  // data gradient: dx = conv(dy, flipped / transposed w), K-channels = Cout, M-channels = Cin
  const int kin = r.kin = dgrad ? d->Cout : d->Cin, mout = r.mout = dgrad ? d->Cin : d->Cout;
  r.transpose = dgrad;
  r.prepacked = (d->flags & M355_CONV_W_PACKED) != 0;
  r.out16 = conv_entry_c8_out(a.entry);
  r.softmax = !dgrad && !r.out16 && (d->flags & M355_CONV_SOFTMAX) != 0;
  r.sigmoid = !dgrad && !r.out16 && (d->flags & M355_CONV_SIGMOID) != 0;
  r.head = r.softmax ? 1 : (r.sigmoid ? 2 : 0);
  const int64_t x_dense = (int64_t)d->Cin * S, y_dense = (int64_t)d->Cout * OS;
  r.in_bs = dgrad ? dense_or(d->y_batch_stride, y_dense) : dense_or(d->x_batch_stride, x_dense);
  r.in16_bs = dense_or(in16 ? a.bs[0] : 0, c8_blocks(kin) * S * 8);
  r.out_bs = r.out16 ? dense_or(a.bs[1], c8_blocks(mout) * S * 8)
                     : (dgrad ? dense_or(d->x_batch_stride, x_dense) : dense_or(d->y_batch_stride, y_dense));
  if (!is_k3s1p1(d)) {
    const int64_t total = (int64_t)d->N * (dgrad ? x_dense : y_dense);
    r.grid = dim3((unsigned)std::min<int64_t>(ceil_div(total, 256), 65535));
    return r;
  }
  if (!dgrad && small_cout_fwd(d)) {
    // the packed-FMA kernel by default; both take the (larger) buffer of the z-Toeplitz MFMA variant
    const bool valu = tuning().smallcout_valu && S < (1ll << 27);
    r.kind = valu ? ConvKind::SmallCoutValu : ConvKind::SmallCoutToeplitz;
    r.packed_bytes = r.workspace_bytes = r.need = smallcout_packed_bytes(d->Cin);
    r.fuses_softmax = valu && tuning().fuse_softmax;   // softmax over the output channels in the epilogue
    r.plan_code[0] = 2;
    r.grid = valu ? dim3((unsigned)(ceil_div(d->D, SMALLCOUT_VS_TZ) * ceil_div(d->H, SMALLCOUT_VS_TY) * ceil_div(d->W, SMALLCOUT_VS_TX)),
                         (unsigned)d->N)
                  : dim3((unsigned)(ceil_div(d->D, 8) * ceil_div(d->H, 8) * ceil_div(d->W, 32)), (unsigned)d->N);
    r.aux = r.prepacked ? 0 : AUX_PACK_W;
    return r;
  }
  const FwdPlan& p = r.plan = plan_mfma(d->N, kin, mout, d->D, d->H, d->W, d->compute);
  const bool h16 = is16(d->compute);
  r.kind = h16 ? (p.oneshot ? ConvKind::H16OneShot : (p.nw == 8 ? ConvKind::H16Queue8 : ConvKind::H16Queue))
               : (p.x3 ? ConvKind::X3 : (p.persistent ? ConvKind::MfmaF32Queue : ConvKind::MfmaF32));
  r.packed_bytes = p.wp_bytes;
  r.h16_workspace_bytes = h16 ? p.wp_bytes + p.slab_bytes : 0;
  r.workspace_bytes = p.wp_bytes + p.slab_bytes + (h16 ? act16_staging_bytes(d->N, kin, S) : 0);
  r.need = in16 ? r.h16_workspace_bytes : r.workspace_bytes;
  r.slab_off = p.wp_bytes;
  r.stage_off = p.wp_bytes + p.slab_bytes;
  // fused statistics: 4 (8) waves x spatial tiles partials from the kernel; a split-K plan emits them from its reduction
  // pass (one slot per block of it), which the 16-bit kernels have only for a c8 output
  const int64_t tile_slots = (int64_t)p.tz_tiles * p.ty_tiles * p.tx_tiles * p.nw, split_slots = splitk_c8_slots(S);
  r.stats_slots = p.ksplit == 1 ? tile_slots : (!h16 && d->N <= 65535 && mout <= 65535 ? split_slots : 0);
  r.stats_slots_c8 = !h16 ? 0 : (p.ksplit == 1 ? tile_slots : split_slots);
  // 16-bit kernels (c8 input, m355_conv3d_fwd_h16): in-register softmax epilogue, unsplit plans
  r.fuses_softmax = !dgrad && h16 && tuning().fuse_softmax && d->Cout <= 4 && p.ksplit == 1;
  const int32_t code = h16 ? (p.oneshot ? 6 : (p.nw == 8 ? 5 : 4)) : (p.x3 ? 7 : (p.persistent ? 3 : 1));
  r.plan_code[0] = code; r.plan_code[1] = p.ntw; r.plan_code[2] = p.gx; r.plan_code[3] = p.ksplit;

  // ---- the launches ----
  const int64_t sp = (int64_t)p.tz_tiles * p.ty_tiles * p.tx_tiles;
  const unsigned nz = (unsigned)(d->N * p.ksplit);
  r.aux = (r.prepacked ? 0 : AUX_PACK_W) | (h16 && !in16 ? AUX_PACK_IN : 0) | (p.tile16 ? AUX_TILE16 : 0);
  if (h16) {
    // edge layers on kernels of their own (unsplit plan, 32 lanes along x, 4 waves): <= 4 K-channels into a c8 output
    // -- four taps per k-step --, <= 4 M-channels into a plain fp32 output -- tap rows folded onto the MFMA's M side
    const bool edge = p.ksplit == 1 && p.gx == 32 && p.nw == 4 && !tuning().no_small;
    const int64_t items = sp * p.otiles * d->N, items_cout4 = sp * d->N;
    if (edge && kin <= 4 && r.out16 && !r.head && items > 0 && items < (1ll << 31)) {
      r.kind = ConvKind::H16C4;
      r.grid = dim3((unsigned)items);
    } else if (edge && mout <= 4 && !r.out16 && !a.add && !a.stat && p.ntw == 4 && p.otiles == 1 && items_cout4 > 0 &&
               items_cout4 < (1ll << 31)) {
      r.kind = ConvKind::H16Cout4;
      r.grid = dim3((unsigned)items_cout4);
    } else {
      const int64_t all = items * p.ksplit;
      r.grid = dim3(p.oneshot ? (unsigned)all : (unsigned)std::max<int64_t>(1, std::min<int64_t>(all, p.slots)));
      r.block = p.nw == 8 ? 512 : 256;
      r.sched = p.oneshot ? tuning().h16_xcd : (p.nw == 8 ? 0 : tuning().h16_stagger);
      r.order = tuning().h16_order;
    }
  } else if (p.x3) {
    r.grid = p.otiles > 0 ? dim3((unsigned)(sp * p.otiles), 1u, nz) : dim3(0, 0, 0);
    if (p.tile16) r.grid16 = dim3((unsigned)sp, 1u, nz);
    r.sched = tuning().conv_cube & 2;
  } else {
    if (p.otiles <= 0) r.grid = dim3(0, 0, 0);
    else if (p.persistent) r.grid = dim3((unsigned)p.slots);
    else r.grid = dim3((unsigned)(sp * std::max(1, p.otiles)), 1u, nz);
    // the 16-row remainder tile: queue-driven kernel over (spatial tile x sample x split) items; up to two residencies
    // one workgroup per item (see plan_mfma)
    const int64_t items16 = sp * d->N * p.ksplit;
    const int64_t g16 = (items16 <= 2 * p.slots && tuning().conv_persistent < 2) ? items16 : std::min<int64_t>(items16, p.slots);
    if (p.tile16) r.grid16 = dim3((unsigned)g16);
    r.sched = tuning().conv_cube;
  }
  if (p.ksplit > 1) {
    r.aux |= AUX_SPLITK | (a.stat ? AUX_SPLITK_STATS : 0);
    if (h16 && r.out16) r.reduce_grid = dim3((unsigned)splitk_c8_slots(S), (unsigned)c8_blocks(mout), (unsigned)d->N);
    else if (a.stat) r.reduce_grid = dim3((unsigned)splitk_c8_slots(S), (unsigned)mout, (unsigned)d->N);
    else r.reduce_grid = dim3((unsigned)std::min<int64_t>(ceil_div((int64_t)d->N * mout * S, 256), 4096));
  }
  return r;
}

static inline int validate_conv(const m355_conv3d_desc* d, const char* who) {
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

static const char* const CONV_ENTRY_NAMES[CE_COUNT] = {
    "conv3d_fwd", "conv3d_fwd", "conv3d_bwd_data", "conv3d_bwd_weight", "conv3d_fwd_h16", "conv3d_fwd_h16_c8",
    "conv3d_bwd_data_h16", "conv3d_bwd_data_h16_c8", "conv3d_bwd_weight_h16", "conv3d_bwd_weight_c8"};

// Every check of a forward / data-gradient entry point, in the order the entry points have always made them (a call that
// is wrong in two ways keeps its code), and the route of a call that passes.
static inline int check_conv(const ConvArgs& a, const m355_conv3d_desc* d, ConvRoute* route) {
  const char* who = CONV_ENTRY_NAMES[a.entry];
  const bool dgrad = conv_entry_dgrad(a.entry), c8_entry = a.entry >= CE_FWD_H16;
  M355_REQUIRE(a.entry != CE_FWD_STATS || a.stat, M355_EINVALID_ARG, "conv3d_fwd_stats: null statistics buffer");
  if (int rc = validate_conv(d, who)) return rc;
  const bool softmax_flag = (d->flags & M355_CONV_SOFTMAX) != 0, sigmoid_flag = (d->flags & M355_CONV_SIGMOID) != 0;
  M355_REQUIRE(!(softmax_flag && sigmoid_flag), M355_EINVALID_ARG, "%s: M355_CONV_SOFTMAX and M355_CONV_SIGMOID exclude each other", who);
  const ConvRoute& r = *route = route_conv(d, a);
  if (!c8_entry) {
    if (!dgrad) {
      M355_REQUIRE(!softmax_flag || r.fuses_softmax, M355_EUNSUPPORTED,
                   "conv3d_fwd: M355_CONV_SOFTMAX needs m355_conv3d_fuses_softmax(desc) != 0");
      M355_REQUIRE(!sigmoid_flag || r.fuses_softmax, M355_EUNSUPPORTED,
                   "conv3d_fwd: M355_CONV_SIGMOID needs m355_conv3d_fuses_sigmoid(desc) != 0");
      M355_REQUIRE(!a.stat || r.stats_slots > 0, M355_EINVALID_ARG,
                   "conv3d_fwd_stats: this descriptor has no fused statistics (m355_conv3d_stats_slots() == 0)");
    }
    M355_REQUIRE(a.in && a.w && a.out, M355_EINVALID_ARG, "%s: null pointer", who);
    M355_REQUIRE(dgrad || (out_dim(d->D, d->k, d->stride, d->pad) > 0 && out_dim(d->H, d->k, d->stride, d->pad) > 0 &&
                           out_dim(d->W, d->k, d->stride, d->pad) > 0),
                 M355_EINVALID_ARG, "conv3d_fwd: empty output");
    M355_REQUIRE(r.kind != ConvKind::Direct || !r.prepacked, M355_EINVALID_ARG, "%s: this descriptor has no packed weights", who);
  } else {
    M355_REQUIRE(is_h16(r.kind), M355_EUNSUPPORTED,
                 "%s: c8 input is only defined for the 3x3x3 / stride 1 / pad 1 kernels in a 16-bit compute mode", who);
    M355_REQUIRE(a.in && a.w && a.out && a.ws, M355_EINVALID_ARG, "%s: null pointer", who);
    M355_REQUIRE(!a.stat || (r.out16 ? r.stats_slots_c8 : r.stats_slots) > 0, M355_EINVALID_ARG,
                 "%s: this descriptor has no fused statistics (m355_conv3d_stats_slots%s() == 0)", who, r.out16 ? "_c8" : "");
    M355_REQUIRE(!r.softmax || r.fuses_softmax, M355_EUNSUPPORTED,
                 "%s: M355_CONV_SOFTMAX needs m355_conv3d_fuses_softmax(desc) != 0", who);
    M355_REQUIRE(!r.sigmoid || r.fuses_softmax, M355_EUNSUPPORTED,
                 "%s: M355_CONV_SIGMOID needs m355_conv3d_fuses_sigmoid(desc) != 0", who);
  }
  M355_REQUIRE(a.ws_bytes >= r.need && (a.ws || !r.need), M355_EWORKSPACE, "conv3d: workspace too small (%zu < %zu)",
               a.ws_bytes, r.need);
  if (!is_h16(r.kind)) {
    M355_REQUIRE(r.kind == ConvKind::Direct || (a.ws & 15) == 0, M355_EINVALID_ARG, "conv3d: workspace not 16B aligned");
    return M355_OK;
  }
  // 16-bit operand kernels; an fp32 input is first rounded into the c8 staging copy behind the slabs
  const uintptr_t in16 = c8_entry ? a.in : a.ws + r.stage_off;
  M355_REQUIRE((a.ws & 15) == 0 && (in16 & 15) == 0 && (r.in16_bs % 8) == 0, M355_EINVALID_ARG,
               "conv3d(16-bit operands): workspace / c8 input not 16B aligned");
  M355_REQUIRE((int64_t)d->D * d->H * d->W * 32 < (1ll << 31) && (int64_t)r.mout * d->D * d->H * d->W < (1ll << 31),
               M355_EUNSUPPORTED, "conv3d(16-bit operands): volume exceeds the 32-bit offsets of a buffer descriptor");
  M355_REQUIRE(!a.stat || r.plan.ksplit == 1 || r.out16, M355_EINVALID_ARG,
               "conv3d(16-bit operands): fused statistics of a split-K plan exist only for the c8 output");
  M355_REQUIRE(!r.out16 || (!a.add && (a.out & 15) == 0 && r.out_bs % 8 == 0), M355_EINVALID_ARG,
               "conv3d(16-bit operands): a c8 output takes no fused `add` and must be 16B aligned");
  M355_REQUIRE(!r.softmax || (r.mout <= 4 && r.plan.ksplit == 1 && !a.add && !a.stat && !r.out16), M355_EUNSUPPORTED,
               "conv3d(16-bit operands): the softmax epilogue needs Cout <= 4, an unsplit plan, fp32 output, no add / statistics");
  M355_REQUIRE(!r.sigmoid || (r.mout <= 4 && r.plan.ksplit == 1 && !a.add && !a.stat && !r.out16), M355_EUNSUPPORTED,
               "conv3d(16-bit operands): the sigmoid epilogue needs Cout <= 4, an unsplit plan, fp32 output, no add / statistics");
  return M355_OK;
}

// ------------------------------------------------------------------ weight gradient
enum class BwwKind {   // one enumerator per kernel template family
  Direct,       // conv3d_direct_bwd_weight_kernel
  MfmaVec,      // conv3_mfma_bww_kernel<GX, true>: float4 interior rows
  MfmaScalar,   // conv3_mfma_bww_kernel<GX, false>
  Mfma2,        // conv3_mfma_bww2_kernel
  Mfma2c,       // conv3_mfma_bww2c_kernel: pair classes of a 1..16 channel remainder
  Small,        // conv3_mfma_bww_small_kernel (<= 4 channels on one side)
  X3,           // conv3_bww_x3_kernel
  X3c,          // conv3_bww_x3c_kernel
  C8,           // conv3_bww_c8_kernel
  C8Small       // conv3_bww_c8_small_kernel: the c8-only flow's edge layers
};
struct BwwRoute {
  BwwKind kind;
  bool via_pack;              // the plain entry point in a 16-bit mode: both operands packed to c8, then the c8 kernel
  bool h16, ok;               // c8 kernels: a 3x3x3 / s1 / p1 descriptor in a 16-bit mode ... whose volume fits 32-bit offsets
  BwwPlan plan;               // Mfma*, Small
  BwwX3Plan x3;               // X3, X3c
  int nsplit;                 // C8, C8Small
  dim3 grid;
  int block;
  BwwClasses kred;            // what the transposed reduction sums: the splits of each pair class
  int reduce_ctiles;
  dim3 reduce_grid;
  int reduce_block;
  uint32_t aux;               // ConvAux
  int64_t xbs, ybs;           // elements between samples of the operands the kernel reads; ...
  int64_t x32_bs, dy_bs;      // ... of the fp32 x (via_pack) and dy (via_pack, bias gradient)
  size_t slab_bytes;          // the slabs, at the head of the workspace
  size_t dbias_off, x16_off, dy16_off;   // the bias gradient's scratch follows them; via_pack: the c8 copies
  size_t workspace_bytes, h16_workspace_bytes, c8_workspace_bytes;   // the three queries
  size_t need;                // workspace bytes this call is checked against
  int32_t plan_code[4];
  const char* who;            // the entry point whose checks and launches these are
};

// the transposed slab reduction: per-tap blocks where the (o, c-tile) grid alone cannot fill the chip
static inline void route_slab_reduce_t(BwwRoute& r, int Cout, int ctiles) {
  int max_ns = 1;
  for (int c = 0; c < 4; ++c) max_ns = std::max(max_ns, r.kred.ns[c]);
  const bool tap = (int64_t)Cout * ctiles < 2 * (int64_t)num_cus() && max_ns >= 16;
  r.aux |= tap ? AUX_SLAB_TAP : AUX_SLAB_T;
  r.reduce_ctiles = ctiles;
  r.reduce_grid = tap ? dim3((unsigned)Cout, (unsigned)ctiles, 27u) : dim3((unsigned)Cout, (unsigned)ctiles);
  r.reduce_block = 256;
}

// Weight gradient with both operands in c8 (m355_conv3d_bwd_weight_h16 / _c8, and the plain entry point behind a pack)
static inline BwwRoute route_bww_c8(const m355_conv3d_desc* d, const ConvArgs& a) {
  BwwRoute r{};
  const bool c8_flow = a.entry == CE_BWD_WEIGHT_C8;
  const int64_t S = (int64_t)d->D * d->H * d->W;
  r.who = CONV_ENTRY_NAMES[c8_flow ? CE_BWD_WEIGHT_C8 : CE_BWD_WEIGHT_H16];
  r.kind = BwwKind::C8;
  r.block = 256;
  r.reduce_grid = dim3(0, 0, 0);
  r.h16 = is_k3s1p1(d) && is16(d->compute);
  r.ok = r.h16 && S * 64 < (1ll << 31);
  if (!r.ok) return r;
  // edge layers (Cin <= 4 or Cout <= 4) of the c8-only flow: tap and narrow channel share the MFMA column
  const bool edge = (d->Cin <= 4 || d->Cout <= 4) && !tuning().no_small;
  r.nsplit = bww_c8_nsplit(d);
  r.slab_bytes = r.dbias_off = (size_t)round_up((int64_t)r.nsplit * d->Cout * d->Cin * 27 * 4, 256);
  r.h16_workspace_bytes = r.slab_bytes + dbias_ws_bytes(d->Cout, S);
  r.c8_workspace_bytes = r.slab_bytes + dbias_c8_ws_bytes(d->N, d->Cout, S);
  r.need = c8_flow ? r.c8_workspace_bytes : r.h16_workspace_bytes;
  r.xbs = dense_or(a.bs[0], c8_blocks(d->Cin) * S * 8);
  r.ybs = dense_or(a.bs[1], c8_blocks(d->Cout) * S * 8);
  r.dy_bs = dense_or(d->y_batch_stride, (int64_t)d->Cout * S);
  const int ctiles = (int)ceil_div(d->Cin, 32), otiles = (int)ceil_div(d->Cout, 32);
  if (c8_flow && edge) {
    r.kind = BwwKind::C8Small;
    r.grid = dim3((unsigned)(ceil_div(d->Cin <= 4 ? d->Cout : d->Cin, 32) * r.nsplit));
  } else {
    r.grid = dim3((unsigned)(ctiles * otiles * r.nsplit));
  }
  r.kred.of = otiles;
  r.kred.cf = ctiles;
  for (int c = 0; c < 4; ++c) r.kred.ns[c] = r.nsplit;
  route_slab_reduce_t(r, d->Cout, ctiles);
  if (a.stat) r.aux |= c8_flow ? AUX_DBIAS_C8 : AUX_DBIAS_F32;
  return r;
}

// Weight gradient of the plain entry point (fp32 NCDHW operands)
static inline BwwRoute route_bww(const m355_conv3d_desc* d, const ConvArgs& a) {
  BwwRoute r{};
  r.who = CONV_ENTRY_NAMES[CE_BWD_WEIGHT];
  r.kind = BwwKind::Direct;
  r.block = 256;
  r.reduce_grid = dim3(0, 0, 0);
  const int64_t S = (int64_t)d->D * d->H * d->W, OS = out_voxels(d);
  const size_t db = dbias_ws_bytes(d->Cout, OS);
  r.workspace_bytes = r.need = db;
  r.xbs = dense_or(d->x_batch_stride, (int64_t)d->Cin * S);
  r.ybs = r.dy_bs = dense_or(d->y_batch_stride, (int64_t)d->Cout * OS);
  if (a.stat) r.aux |= AUX_DBIAS_F32;
  if (!is_k3s1p1(d)) {
    r.grid = dim3((unsigned)((int64_t)d->Cout * d->Cin * d->k * d->k * d->k));   // (check_bww: below 2^31)
    return r;
  }
  const int64_t total = (int64_t)d->Cout * d->Cin * 27;
  // M355_COMPUTE_F32X3: the weight gradient on the split kernels too (M355_F32X3=2 forces every fp32 layer there,
  // M355_F32X3_BWW=0 keeps the weight gradient on the fp32 MFMA kernels)
  const bool x3_mode = d->compute == M355_COMPUTE_F32X3 || (d->compute == M355_COMPUTE_F32 && tuning().f32x3 == 2);
  if (x3_mode && tuning().f32x3 && tuning().f32x3_bww && d->Cin > 4 && d->Cout > 4 && d->D >= 2 && S < (1ll << 24)) {
    const BwwX3Plan& p = r.x3 = plan_bww_x3(d->N, d->Cin, d->Cout, d->D, d->H, d->W);
    r.kind = p.classes ? BwwKind::X3c : BwwKind::X3;
    r.grid = dim3((unsigned)(p.classes ? p.class_wgs : p.ctiles * p.otiles * p.nsplit));
    r.block = 512;
    r.kred = p.k;   // k.ns: splits of each pair class
    route_slab_reduce_t(r, d->Cout, p.ctiles);
    r.slab_bytes = r.dbias_off = p.slab_bytes;
    r.workspace_bytes = r.need = r.slab_bytes + db;
    r.plan_code[0] = 8; r.plan_code[2] = p.tx; r.plan_code[3] = p.nsplit;
    return r;
  }
  const BwwPlan& p = r.plan = plan_bww(d->N, d->Cin, d->Cout, d->D, d->H, d->W);
  r.slab_bytes = r.dbias_off = p.slab_bytes;
  r.workspace_bytes = r.need = r.slab_bytes + db;
  // tap-on-lane kernel; a sample must fit the 32-bit byte offsets of a buffer descriptor
  const bool small = (d->Cin <= 4 || d->Cout <= 4) && !tuning().no_small &&
                     (int64_t)std::max(d->Cin, d->Cout) * S < (1ll << 29);
  r.plan_code[2] = p.gx; r.plan_code[3] = p.nsplit;
  ConvArgs a16 = a;   // the c8 kernel behind the pack reads dense c8 copies
  a16.entry = CE_BWD_WEIGHT_H16;
  a16.bs[0] = a16.bs[1] = 0;
  const BwwRoute c8 = route_bww_c8(d, a16);
  if (c8.ok && !small && d->N <= 65535) {
    // 16-bit operand mode: both operands are rounded into c8 copies that follow the c8 kernel's own workspace; the
    // launches, the checks' name and the bias gradient's scratch are the c8 route's
    BwwRoute v = c8;
    v.via_pack = true;
    v.aux |= AUX_PACK_IN | AUX_PACK_DY;
    v.plan = p;
    v.x32_bs = r.xbs;
    v.x16_off = c8.h16_workspace_bytes;
    v.dy16_off = v.x16_off + act16_staging_bytes(d->N, d->Cin, S);
    v.workspace_bytes = v.need = std::max(r.workspace_bytes, v.dy16_off + act16_staging_bytes(d->N, d->Cout, S));
    std::copy_n(r.plan_code, 4, v.plan_code);
    v.plan_code[0] = 11;
    return v;
  }
  if (small) {
    // narrow side (<= 4 channels) shares the lane index with the taps
    r.kind = BwwKind::Small;
    r.grid = dim3((unsigned)ceil_div(d->Cin <= 4 ? d->Cout : d->Cin, 32), (unsigned)p.nsplit);
    r.aux |= AUX_SLAB_PLAIN;
    r.reduce_grid = dim3((unsigned)std::min<int64_t>(ceil_div(total, 256), 2048));
    r.reduce_block = 256;
    r.plan_code[0] = 10;
    return r;
  }
  r.plan_code[0] = 9;
  // The choice of the MFMA kernel that a descriptor cannot make.  vec: float4 interior rows need 16-byte aligned rows.
  // gen2: the second-generation kernels need float4 rows, and a sample must fit the 32-bit byte offsets of a buffer
  // descriptor (the hardware zero-fills what lies past it); otherwise conv3_mfma_bww_kernel<GX, vec>.
  const bool vec = (d->W % 4 == 0) && (r.xbs % 4 == 0) && (a.in & 15) == 0;
  const bool gen2 = vec && (a.w & 3) == 0 && (int64_t)d->Cin * S < (1ll << 29) && (int64_t)d->Cout * S < (1ll << 29) &&
                    tuning().bww_gen == 2;
  r.kred = p.k;
  if (gen2 && p.classes) {
    r.kind = BwwKind::Mfma2c;
    r.grid = dim3((unsigned)p.class_wgs);
  } else if (gen2) {
    r.kind = BwwKind::Mfma2;
    r.grid = dim3((unsigned)(p.ctiles * p.otiles * p.nsplit));
    for (int c = 0; c < 4; ++c) r.kred.ns[c] = p.nsplit;   // the uniform count
  } else {
    r.kind = vec ? BwwKind::MfmaVec : BwwKind::MfmaScalar;
    r.grid = dim3((unsigned)p.ctiles, (unsigned)p.otiles, (unsigned)p.nsplit);
  }
  if (gen2) {
    route_slab_reduce_t(r, d->Cout, p.ctiles);
  } else {
    r.aux |= AUX_SLAB_PLAIN;
    r.reduce_grid = dim3((unsigned)std::min<int64_t>(ceil_div(total, 64), 4096));
    r.reduce_block = 64;
  }
  return r;
}

// Every check of a weight-gradient entry point, in the entry points' order, and the route of a call that passes.
static inline int check_bww(const ConvArgs& a, const m355_conv3d_desc* d, BwwRoute* route) {
  const char* who = CONV_ENTRY_NAMES[a.entry];
  if (int rc = validate_conv(d, who)) return rc;
  const int64_t S = (int64_t)d->D * d->H * d->W;
  if (a.entry == CE_BWD_WEIGHT) {
    M355_REQUIRE(a.in && a.w && a.out, M355_EINVALID_ARG, "conv3d_bwd_weight: null pointer");
    const BwwRoute& r = *route = route_bww(d, a);
    M355_REQUIRE(a.ws && a.ws_bytes >= r.need, M355_EWORKSPACE, "conv3d_bwd_weight: workspace too small (%zu < %zu)",
                 a.ws_bytes, r.need);
    M355_REQUIRE(r.kind == BwwKind::Direct || r.kind == BwwKind::X3 || r.kind == BwwKind::X3c ||
                     ((int64_t)d->Cin * S < (1ll << 31) && (int64_t)d->Cout * S < (1ll << 31)),
                 M355_EUNSUPPORTED, "conv3d_bwd_weight: tensor exceeds 2^31 elements per sample");
    if (r.via_pack)   // the c8 copies sit at multiples of 256 bytes behind the workspace pointer
      M355_REQUIRE((a.ws & 15) == 0, M355_EINVALID_ARG, "conv3d_bwd_weight_h16: c8 tensor not 16B aligned");
    else if (r.kind == BwwKind::Direct)
      M355_REQUIRE((int64_t)d->Cout * d->Cin * d->k * d->k * d->k < (1ll << 31), M355_EUNSUPPORTED,
                   "conv3d_bwd_weight: grid too large");
    else if (r.kind == BwwKind::X3 || r.kind == BwwKind::X3c)
      M355_REQUIRE(((a.in | a.w) & 3) == 0, M355_EINVALID_ARG, "conv3d_bwd_weight: misaligned tensor");
    return M355_OK;
  }
  const bool c8_flow = a.entry == CE_BWD_WEIGHT_C8;
  const BwwRoute& r = *route = route_bww_c8(d, a);
  M355_REQUIRE(r.h16, M355_EUNSUPPORTED,
               "%s: c8 input is only defined for the 3x3x3 / stride 1 / pad 1 kernels in a 16-bit compute mode", who);
  M355_REQUIRE(a.in && a.w && a.out && a.ws, M355_EINVALID_ARG, "%s: null pointer", who);
  M355_REQUIRE(r.ok, M355_EUNSUPPORTED, "%s: volume too large for the c8 kernel (>= 2^25 voxels)", who);
  M355_REQUIRE(c8_flow || !a.stat || a.bias, M355_EINVALID_ARG, "%s: the bias gradient needs the fp32 dy", who);
  M355_REQUIRE(a.ws_bytes >= r.need, M355_EWORKSPACE, "%s: workspace too small (%zu < %zu)", who, a.ws_bytes, r.need);
  M355_REQUIRE(((a.in | a.w) & 15) == 0 && r.xbs % 8 == 0 && r.ybs % 8 == 0, M355_EINVALID_ARG,
               "%s: c8 tensor not 16B aligned", who);
  return M355_OK;
}

}  // namespace m355
