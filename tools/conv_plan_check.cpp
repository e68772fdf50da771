// Stand-alone host check of the 3x3x3 conv routes (csrc/conv3d_route.hpp): walks check_conv / check_bww -- the checks and the
// route_* behind them -- of all ten launching entry points over valid and faulty argument tuples under every variant-forcing
// tuning value, for a sanitizer build of the host code -- no GPU, nothing is launched, no pointer is followed:
//   cd segmentation-pipeline_amd/csrc && hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined \
//     -x hip abi.cpp norm.hip act16.hip train16.hip ../../tools/conv_plan_check.cpp -I ../../include -o /tmp/conv_plan_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../segmentation-pipeline_amd/csrc/conv3d_route.hpp"

using namespace m355;

static long calls = 0, served = 0, bad = 0, seen_conv[11], seen_bww[10];
static uint64_t sum = 0;

static void report(const m355_conv3d_desc& d, const ConvArgs& a, int variant, dim3 g, dim3 g2, unsigned aux, size_t need) {
  if (++bad <= 10)
    std::fprintf(stderr, "implausible: entry %d N%d %d->%d %dx%dx%d k%d c%d variant %d grid %u/%u/%u second grid %u/%u/%u aux %u need %zu\n",
                 a.entry, d.N, d.Cin, d.Cout, d.D, d.H, d.W, d.k, d.compute, variant, g.x, g.y, g.z, g2.x, g2.y, g2.z, aux, need);
}

static bool grid_ok(dim3 g) { return g.x >= 1 && g.x < (1u << 31) && g.y >= 1 && g.y <= 65535 && g.z >= 1 && g.z <= 65535; }

static void walk(const m355_conv3d_desc& d, const ConvArgs& a) {
  ++calls;
  if (a.entry == CE_BWD_WEIGHT || a.entry == CE_BWD_WEIGHT_H16 || a.entry == CE_BWD_WEIGHT_C8) {
    BwwRoute r;
    const int rc = check_bww(a, &d, &r);
    if (rc != M355_OK) { sum += (uint64_t)-rc; return; }
    ++served;
    const int v = (int)r.kind;
    const bool reduces = (r.aux & (AUX_SLAB_T | AUX_SLAB_TAP | AUX_SLAB_PLAIN)) != 0;
    if (v < 0 || v > 9 || !grid_ok(r.grid) || (r.block != 256 && r.block != 512) || r.need > a.ws_bytes || r.dbias_off > r.need ||
        (r.via_pack && !(r.dbias_off <= r.x16_off && r.x16_off < r.dy16_off && r.dy16_off < r.need)) ||
        reduces != (r.kind != BwwKind::Direct) || (reduces && (!grid_ok(r.reduce_grid) || r.reduce_block < 64)) || r.xbs <= 0 ||
        r.ybs <= 0)
      report(d, a, v, r.grid, r.reduce_grid, r.aux, r.need);
    else
      ++seen_bww[v];
    sum += v + r.grid.x + r.grid.y + r.grid.z + r.block + r.aux + r.need + r.reduce_grid.x + r.dbias_off + r.x16_off;
    return;
  }
  ConvRoute r;
  const int rc = check_conv(a, &d, &r);
  if (rc != M355_OK) { sum += (uint64_t)-rc; return; }
  ++served;
  const int v = (int)r.kind;
  const bool only16 = (r.aux & AUX_TILE16) && r.plan.otiles == 0;   // a <= 16 channel output: no main launch
  if (v < 0 || v > 10 || (only16 ? r.grid.x != 0 : !grid_ok(r.grid)) || (r.block != 256 && r.block != 512) ||
      r.need > a.ws_bytes || r.slab_off > r.need || r.stage_off > r.need || ((r.aux & AUX_PACK_IN) && r.stage_off >= r.need) ||
      ((r.aux & AUX_SPLITK) && (!grid_ok(r.reduce_grid) || r.slab_off >= r.need)) ||
      ((r.aux & AUX_TILE16) != 0) != (r.grid16.x != 0) || ((r.aux & AUX_TILE16) && !grid_ok(r.grid16)) || r.in_bs <= 0 ||
      r.in16_bs <= 0 || r.out_bs <= 0)
    report(d, a, v, r.grid, r.grid16, r.aux, r.need);
  else
    ++seen_conv[v];
  sum += v + r.grid.x + r.grid.y + r.grid.z + r.block + r.grid16.x + r.grid16.z + r.aux + r.need + r.reduce_grid.x + r.slab_off +
         r.stage_off;
}

int main() {
  // each forces a variant (or a side of a choice) that the default tuning does not reach on these shapes
  const char* tunings[][2] = {{"", ""}, {"M355_CONV_SLOTS", "5"}, {"M355_CONV_KSPLIT", "2"}, {"M355_CONV_NTW", "4"},
                              {"M355_CONV_NTW", "8"}, {"M355_CONV_PERSISTENT", "2"}, {"M355_H16_ONESHOT", "3"},
                              {"M355_H16_ONESHOT", "0"}, {"M355_H16_W8", "2"}, {"M355_NO_SMALL", "1"}, {"M355_SMALLCOUT_VALU", "0"},
                              {"M355_BWW_GEN", "1"}, {"M355_BWW_NSPLIT", "3"}, {"M355_BWW_QUEUE", "0"}, {"M355_TILE16", "0"},
                              {"M355_F32X3", "2"}, {"M355_F32X3", "0"}, {"M355_F32X3_BWW", "0"}, {"M355_F32X3_EDGE", "1"}};
  const int vols[][3] = {{6, 9, 36}, {5, 7, 33}, {8, 4, 32}, {1, 1, 1}, {16, 16, 16}, {64, 64, 64}, {128, 128, 128},
                         {256, 256, 512}, {512, 512, 512}, {0, 4, 4}};
  const int chans[][2] = {{3, 32}, {32, 4}, {40, 24}, {32, 32}, {8, 40}, {1, 1}, {16, 3}, {120, 80}, {32, 0}};
  const int geoms[][3] = {{3, 1, 1}, {1, 1, 0}, {3, 2, 1}, {9, 1, 1}};
  const uintptr_t offs[] = {0, 4, 8};
  const int64_t pads[] = {0, 8, 1};   // batch strides: dense, padded by a multiple of 8 elements, by an odd count
  for (auto& t : tunings) {
    if (t[0][0]) setenv(t[0], t[1], 1);
    m355_reload_tuning();
    for (int entry = 0; entry < CE_COUNT; ++entry)
      for (auto& v : vols)
        for (auto& c : chans)
          for (auto& g : geoms)
            // (65536: past the sample limit of the pack behind the plain weight gradient; forward and data gradient put
            // N * split-K, split-K <= 8, on grid.z -- past 65535 there the launch itself fails)
            // (the sample limit on the test volumes only: with 65535 samples of 2^25 voxels the one-shot grids pass 2^32 items,
            // in a workspace of tens of terabytes)
            for (int n : {1, 2, &v - vols >= 3 ? 2 : (entry == CE_BWD_WEIGHT ? 65536 : (entry >= CE_BWD_WEIGHT_H16 ? 65535 : 8191))})
              for (int compute = 0; compute < 5; ++compute)
                for (int flags = 0; flags < 4; ++flags) {
                  if ((g[0] != 3 && (flags || n > 2)) || (n > 2 && flags)) continue;
                  const int64_t S = (int64_t)v[0] * v[1] * v[2];
                  // optional tensors (bit 0 add, bit 1 statistics / dbias, bit 2 bias / fp32 dy) alone, with a fault (1..4 a
                  // pointer pair at +4 / +8, 5..6 a null pointer, 7 no workspace bytes), with padded batch strides
                  for (int variation = 0; variation < 24; ++variation) {
                    const int optional = variation & 7, fault = variation >= 8 && variation < 16 ? variation - 8 : 0;
                    const int64_t pad = variation >= 16 ? pads[1 + (variation & 1)] : 0;
                    m355_conv3d_desc d = {};
                    d.N = n; d.Cin = c[0]; d.Cout = c[1]; d.D = v[0]; d.H = v[1]; d.W = v[2];
                    d.k = g[0]; d.stride = g[1]; d.pad = g[2]; d.compute = compute;
                    d.flags = (flags & 1 ? M355_CONV_W_PACKED : 0) | (flags & 2 ? M355_CONV_SOFTMAX : 0);
                    if (pad) d.x_batch_stride = (int64_t)(c[0] + 8) * S + pad, d.y_batch_stride = (int64_t)(c[1] + 8) * S + 2 * pad;
                    ConvArgs a = {entry, 1 << 20, 2 << 20, optional & 4 ? 3u << 20 : 0, optional & 1 ? 4u << 20 : 0, 5 << 20,
                                  optional & 2 ? 6u << 20 : 0, 7 << 20, (size_t)1 << 60, {0, 0}};
                    if (pad) a.bs[0] = 8 * ((c[0] + c[1] + 8) / 8 + 1) * S + pad, a.bs[1] = a.bs[0] + pad;
                    const uintptr_t off = offs[1 + (fault & 1)];
                    if (fault == 1 || fault == 2) a.in += off, a.w += off;
                    if (fault == 3 || fault == 4) a.out += off, a.ws += off;
                    if (fault == 5) a.in = 0;
                    if (fault == 6) a.ws = 0;
                    if (fault == 7) a.ws_bytes = 0;
                    walk(d, a);
                  }
                }
    if (t[0][0]) unsetenv(t[0]);
  }
  long missing = 0;
  for (long s : seen_conv) missing += s == 0;
  for (long s : seen_bww) missing += s == 0;
  std::printf("tuples %ld, served %ld, implausible plans %ld, variants never produced %ld, checksum %llu\n", calls, served, bad,
              missing, (unsigned long long)sum);
  return bad != 0 || served == 0 || missing != 0;
}
