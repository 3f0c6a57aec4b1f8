// draw_kernel_time.hip -- the kernels of nidreg_draw alone, timed with HIP events (tools/draw_time.py builds and runs this; the
// library's entry point is stateless and reports no timing of its own).  Same kernels (csrc/nid_draw_kernels.hpp), same launch shapes
// and the same null-stream sequence as csrc/nidreg_draw.hip: owner words zeroed, k_draw_prims, k_draw_compose.
//   draw_kernel_time <left_w> <left_h> <right_w> <right_h> <prims.bin: 8 int32 per primitive> <repeats>
// prints one JSON line: the median milliseconds of the three steps and of the whole sequence.
#include "../direct_visual_lidar_calibration_amd/csrc/nid_draw_kernels.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace nidreg;

#define CHECK(expr)                                                                  \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess) {                                                          \
      std::fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(_e));                \
      return 1;                                                                      \
    }                                                                                \
  } while (0)

static float median(std::vector<float> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char** argv) {
  if (argc != 7) {
    std::fprintf(stderr, "usage: %s left_w left_h right_w right_h prims.bin repeats\n", argv[0]);
    return 2;
  }
  const int lw = std::atoi(argv[1]), lh = std::atoi(argv[2]), rw = std::atoi(argv[3]), rh = std::atoi(argv[4]), reps = std::atoi(argv[6]);
  if (lw < 1 || lh < 1 || rw < 1 || rh < 1 || lw > kDrawMaxDim || lh > kDrawMaxDim || rw > kDrawMaxDim || rh > kDrawMaxDim || reps < 1) return 2;
  std::vector<int32_t> prims;
  if (FILE* f = std::fopen(argv[5], "rb")) {
    int32_t rec[kDrawWords];
    while (std::fread(rec, sizeof(rec), 1, f) == 1) prims.insert(prims.end(), rec, rec + kDrawWords);
    std::fclose(f);
  } else {
    std::fprintf(stderr, "cannot open %s\n", argv[5]);
    return 2;
  }
  const long long n = (long long)(prims.size() / kDrawWords);
  for (long long i = 0; i < n; i++) {  // the checks of nidreg_draw that keep the kernels inside their buffers
    const int32_t* r = &prims[size_t(i) * kDrawWords];
    const bool line = r[0] == kDrawLine;
    const auto c = [](int32_t v) { return v >= kDrawCoordMin && v <= kDrawCoordMax; };
    if ((!line && r[0] != kDrawRing && r[0] != kDrawDisc) || !c(r[1]) || !c(r[2]) || (line && (!c(r[3]) || !c(r[4]))) || (!line && (r[3] < 0 || r[3] > kDrawMaxRadius))) return 2;
  }
  if (n < 1 || n > kDrawMaxPrims) return 2;
  const int cw = 2 * lw;
  const size_t npix = size_t(cw) * size_t(lh);
  uint8_t *d_left, *d_right, *d_out;
  uint32_t* d_owner;
  int32_t* d_prims;
  CHECK(hipMalloc(&d_left, size_t(lw) * lh));
  CHECK(hipMalloc(&d_right, size_t(rw) * rh));
  CHECK(hipMalloc(&d_out, npix * 3));
  CHECK(hipMalloc(&d_owner, npix * sizeof(uint32_t)));
  CHECK(hipMalloc(&d_prims, prims.size() * sizeof(int32_t)));
  CHECK(hipMemset(d_left, 90, size_t(lw) * lh));
  CHECK(hipMemset(d_right, 160, size_t(rw) * rh));
  CHECK(hipMemcpy(d_prims, prims.data(), prims.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  hipEvent_t ev[4];
  for (auto& e : ev) CHECK(hipEventCreate(&e));
  std::vector<float> t_zero, t_prims, t_compose, t_all;
  for (int it = 0; it < reps + 2; it++) {  // two warm-up rounds
    CHECK(hipEventRecord(ev[0], nullptr));
    CHECK(hipMemsetAsync(d_owner, 0, npix * sizeof(uint32_t), nullptr));
    CHECK(hipEventRecord(ev[1], nullptr));
    hipLaunchKernelGGL(k_draw_prims, dim3(unsigned(n)), dim3(kDrawWave), 0, nullptr, d_prims, cw, lh, d_owner);
    CHECK(hipGetLastError());
    CHECK(hipEventRecord(ev[2], nullptr));
    hipLaunchKernelGGL(k_draw_compose, dim3(unsigned((npix + kDrawThreads - 1) / kDrawThreads)), dim3(kDrawThreads), 0, nullptr, d_left, lw, lh, d_right, rw, rh, cw, d_owner, d_prims, d_out);
    CHECK(hipGetLastError());
    CHECK(hipEventRecord(ev[3], nullptr));
    CHECK(hipEventSynchronize(ev[3]));
    if (it < 2) continue;
    float a, b, c, d;
    CHECK(hipEventElapsedTime(&a, ev[0], ev[1]));
    CHECK(hipEventElapsedTime(&b, ev[1], ev[2]));
    CHECK(hipEventElapsedTime(&c, ev[2], ev[3]));
    CHECK(hipEventElapsedTime(&d, ev[0], ev[3]));
    t_zero.push_back(a), t_prims.push_back(b), t_compose.push_back(c), t_all.push_back(d);
  }
  std::printf("{\"primitives\": %lld, \"repeats\": %d, \"zero_owner_ms\": %.4f, \"k_draw_prims_ms\": %.4f, \"k_draw_compose_ms\": %.4f, \"sequence_ms\": %.4f}\n", n, reps, median(t_zero),
              median(t_prims), median(t_compose), median(t_all));
  return 0;
}
