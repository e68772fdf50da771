// Stand-alone host check of the normalisation plan (csrc/norm_host.hpp): calls m355_norm_num_stats, m355_norm_workspace and
// m355_norm_plan (all ten passes) over the descriptor list of tools/conv_routes.py --norm, for a sanitizer build of the host
// code -- no GPU, nothing is launched:
//   cd segmentation-pipeline_amd/csrc && hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined \
//     -x hip abi.cpp norm.hip act16.hip train16.hip ../../tools/norm_plan_check.cpp -I ../../include -o /tmp/norm_plan_check
#include <cstdint>
#include <cstdio>

#include "m355seg.h"

int main() {
  const int channels[][2] = {{8, 0}, {20, 0}, {32, 0}, {8, 8}, {8, 2}, {32, 8}, {20, 4}, {40, 8}};
  const int64_t sizes[] = {1, 63, 64, 3276, 3277, 4095, 4096, 4097, 4100, 8191, 8192, 8193, 16383, 16384, 16385, 16388, 32768,
                           64 * 64 * 64, 128 * 128 * 128, 32 * 256 * 256};
  const int strides[] = {0, 4, 1};
  uint64_t sum = 0;
  long lines = 0, failed = 0;
  for (int n = 1; n <= 2; ++n)
    for (auto& cg : channels)
      for (int64_t s : sizes)
        for (int k : strides) {
          m355_norm_desc d = {n, cg[0], s, cg[1], 1, 1e-5f, 0.f, 0, 0, 0};
          if (k) d.x_batch_stride = cg[0] * s + k, d.y_batch_stride = cg[0] * s + 2 * k, d.add_batch_stride = cg[0] * s + 3 * k;
          sum += (uint64_t)m355_norm_num_stats(&d) + m355_norm_workspace(&d);
          for (int which = 0; which < 10; ++which) {
            int32_t out[4];
            if (m355_norm_plan(&d, which, out) != 0) ++failed;
            sum += (uint64_t)out[0] + out[1] + out[2] + out[3];
          }
          ++lines;
        }
  int32_t out[4];
  const m355_norm_desc bad = {1, 30, 64, 8, 0, 1e-5f, 0.f, 0, 0, 0};
  if (m355_norm_plan(nullptr, 0, out) != -1 || m355_norm_plan(&bad, 0, out) != -1 || m355_norm_workspace(nullptr) != 0) ++failed;
  std::printf("descriptors %ld, failed calls %ld, checksum %llu\n", lines, failed, (unsigned long long)sum);
  return failed != 0;
}
