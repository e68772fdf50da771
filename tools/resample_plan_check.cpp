// Stand-alone host check of the resampling plans (csrc/resample_host.hpp): walks validate_resample / plan_resample of all 17
// entry points over valid and faulty argument tuples, for a sanitizer build of the host code -- no GPU, nothing is launched,
// no pointer is followed:
//   cd segmentation-pipeline_amd/csrc && hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined \
//     -x hip abi.cpp ../../tools/resample_plan_check.cpp -I ../../include -o /tmp/resample_plan_check
#include <cstdint>
#include <cstdio>

#include "../segmentation-pipeline_amd/csrc/resample_host.hpp"

using namespace m355;

int main() {
  const int vols[][3] = {{2, 2, 2}, {2, 4, 4}, {2, 2, 6}, {4, 6, 8}, {1, 2, 2}, {2, 2, 3}, {3, 5, 7}, {2, 2, 306}, {2, 2, 308},
                         {36, 10, 132}, {128, 128, 128}, {4096, 4096, 308}, {0, 4, 4}, {4, -2, 4}};
  const int channels[] = {1, 3, 8, 9, 32, 0};
  const int64_t pads[] = {0, 8, 1, 2};
  const uintptr_t offs[] = {0, 8, 4, 1};
  const int computes[] = {M355_COMPUTE_BF16, M355_COMPUTE_F16, 0, 7};
  uint64_t sum = 0;
  long calls = 0, served = 0, bad = 0;
  for (int op = 0; op < RS_COUNT; ++op)
    for (auto& v : vols)
      for (int c : channels)
        for (int n = 1; n <= 2; ++n)
          for (int64_t pad : pads)
            for (uintptr_t off : offs)
              for (int null = 0; null < 5; ++null)   // 4: none
                for (int compute : computes) {
                  ResampleArgs a = {n, c, v[0], v[1], v[2], compute, {0, 0, 0}, {4096 + off, 8192 + off, 12288 + off, 16384 + off}};
                  if (pad)
                    for (int i = 0; i < 3; ++i) a.bs[i] = 64ll * (c + 7) * v[0] * v[1] * v[2] + pad * (i + 1);
                  if (null < 4) a.ptr[null] = 0;
                  ++calls;
                  const int rc = validate_resample((ResampleOp)op, a);
                  if (rc != M355_OK) {
                    sum += (uint64_t)-rc;
                    continue;
                  }
                  const ResamplePlan p = plan_resample((ResampleOp)op, a);
                  ++served;
                  if (p.grid.x < 1 || p.grid.x > 65536 || p.bs[0] <= 0 || p.bs[1] <= 0 || p.variant < 0 || p.variant > RS_LDS ||
                      (p.variant == RS_LDS) != (p.lds != 0) || p.lds > 48 * 1024)
                    ++bad;
                  sum += p.grid.x + p.grid.y + p.grid.z + p.lds + (uint64_t)p.bs[0] + (uint64_t)p.bs[1] + (uint64_t)p.bs[2] + p.variant;
                }
  std::printf("tuples %ld, served %ld, implausible plans %ld, checksum %llu\n", calls, served, bad, (unsigned long long)sum);
  return bad != 0 || served == 0;
}
