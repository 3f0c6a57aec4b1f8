// SPLINE (NIDCost) kernels + projection utility.  Built with -ffp-contract=off like every other
// translation unit (csrc/Makefile): the fusions wanted are explicit fma calls, so a point gets the same arithmetic
// whichever unrolled slot / chunk / GPU processes it.
#include "nid_launch_impl.hpp"

namespace nidreg {

hipError_t launch_spline_hist(const PassArgs& a) {
  if (a.nchunks == 0) return hipSuccess;
  return a.rec64 ? spline_hist_rec<Rec64>(a, nullptr) : spline_hist_rec<Rec32>(a, nullptr);
}
hipError_t launch_spline_grad(const PassArgs& a) {
  if (a.nchunks == 0) return hipSuccess;
  return a.rec64 ? spline_grad_rec<Rec64>(a, nullptr) : spline_grad_rec<Rec32>(a, nullptr);
}
int occupancy_spline_hist(const PassArgs& a) { return a.rec64 ? occupancy_of(spline_hist_rec<Rec64>, a) : occupancy_of(spline_hist_rec<Rec32>, a); }
int occupancy_spline_grad(const PassArgs& a) { return a.rec64 ? occupancy_of(spline_grad_rec<Rec64>, a) : occupancy_of(spline_grad_rec<Rec32>, a); }
hipError_t launch_project(int model, const double* intr, const double* dist, const double* p3, long long n, double* uv, double* jac, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const CamParams<double> cam = make_cam(model, intr, dist);
  const unsigned grid = unsigned((n + 255) / 256);
  return with_model(model, hipErrorInvalidValue, [&](auto M) {
    hipLaunchKernelGGL(k_project<M>, dim3(grid), dim3(256), 0, stream, p3, n, cam, uv, jac);
    return hipGetLastError();
  });
}

// the same projection code on the HOST (nid_device.hpp's scalar math is __host__ __device__): for callers that project a
// handful of points at a time -- estimate_camera_fov inverts the projection at three pixels with NelderMead<2>, ~240 probes
// of ONE point (src/vlcal/common/estimate_fov.cpp:17-51), host work in the reference as well
int project_host(int model, const double* intr, const double* dist, const double* p3, long long n, double* uv, double* jac) {
  const CamParams<double> cam = make_cam(model, intr, dist);
  return with_model(model, -1, [&](auto M) {
    for (long long i = 0; i < n; i++) {
      double u, v, du[3], dv[3];
      project_jac<M, double>(cam, p3[3 * i], p3[3 * i + 1], p3[3 * i + 2], u, v, du, dv);
      uv[2 * i] = u, uv[2 * i + 1] = v;
      if (jac)
        for (int k = 0; k < 3; k++) jac[6 * i + k] = du[k], jac[6 * i + 3 + k] = dv[k];
    }
    return 0;
  });
}

}  // namespace nidreg


#ifdef NID_STAMP
// development aid (tools/stage_times.py, an instrumented build loaded through NIDREG_LIB): the stage stamps of the last launch
extern "C" int nidreg_debug_stage_stamps(unsigned long long* out, int words) {
  return int(hipMemcpyFromSymbol(out, HIP_SYMBOL(nidreg::g_stage), size_t(words) * sizeof(unsigned long long)));
}
extern "C" int nidreg_debug_wg_stamps(unsigned long long* out, int words) {
  return int(hipMemcpyFromSymbol(out, HIP_SYMBOL(nidreg::g_stamp), size_t(words) * sizeof(unsigned long long)));
}
#endif
