// nid_launch_impl.hpp -- bodies of the launch wrappers.  nid_kernels_f64.hip, nid_kernels_f64_exact.hip and nid_kernels_fused.hip
// each include the whole file and instantiate only the static templates their entry points use.
#pragma once
#include <mutex>
#include <utility>
#include <vector>

#include "nid_kernels.hpp"
#include "nid_launch.hpp"

namespace nidreg {

static PoseParams<double> make_pose(const PassArgs& a) {
  PoseParams<double> p;
  for (int i = 0; i < 9; i++) p.R[i] = a.R[i];
  for (int i = 0; i < 3; i++) p.t[i] = a.t[i];
  return p;
}
static IsoParams<double> make_iso(const double* T) {  // rows 0..2 of the 4x4
  IsoParams<double> p;
  for (int i = 0; i < 12; i++) p.m[i] = T[i];
  return p;
}

// A kernel that needs more than 64 KB of dynamic LDS must be told so once per (kernel, device); doing it on every
// launch put a runtime call on the critical path of each evaluation of the headline configuration.
template <typename K>
static hipError_t ensure_lds(K kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return hipSuccess;
  static std::mutex mu;
  static std::vector<std::pair<const void*, std::pair<int, size_t>>> done;  // (kernel, (device, bytes granted))
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const void* key = reinterpret_cast<const void*>(kernel);
  std::lock_guard<std::mutex> lk(mu);
  for (const auto& d : done)
    if (d.first == key && d.second.first == dev && d.second.second >= bytes) return hipSuccess;
  e = hipFuncSetAttribute(key, hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes));
  if (e == hipSuccess) done.push_back(std::make_pair(key, std::make_pair(dev, bytes)));
  return e;
}

// One workgroup per chunk of a's table; with `occ` nothing is launched: *occ = workgroups of this kernel that fit on one CU at once
// (`args`, and the pose and camera the passes build for them, are then unused).
template <typename K, typename... Args>
static hipError_t launch_chunks(K k, int threads, size_t lds, const PassArgs& a, int* occ, const Args&... args) {
  const hipError_t e = ensure_lds(k, lds);
  if (e != hipSuccess) return e;
  if (occ) return hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, reinterpret_cast<const void*>(k), threads, lds);
  hipLaunchKernelGGL(k, dim3(a.nchunks), dim3(threads), lds, a.stream, args...);
  return hipGetLastError();
}
// the last kernel argument: MultiDyn by value in the MULTI instantiations, an empty struct in the others
template <bool MULTI>
static typename multi_dyn_of<MULTI>::type dyn_of(const PassArgs& a) {
  if constexpr (MULTI) return a.dyn;
  else return NoMultiDyn();
}
// what an occupancy_* entry point makes of its pass (0 on error)
template <typename Pass>
static int occupancy_of(Pass pass, const PassArgs& a) {
  int n = 0;
  return pass(a, &n) == hipSuccess ? n : 0;
}

// The three passes: each picks its kernel instantiation from `a` and launches it -- or, with `occ`, reports the occupancy of the
// straight-line single-pair instantiation (MULTI = SEG = false), which is what the planner sizes its tables by.
template <typename Rec>
static hipError_t spline_hist_rec(const PassArgs& a, int* occ) {
  const PoseParams<double> pose = make_pose(a);
  const CamParams<double> cam = make_cam(a.model, a.intr, a.dist);
  return with_model(a.model, hipErrorInvalidValue, [&](auto M) {
    return with_bool(a.wide, [&](auto WIDE) {  // B = 256, GW = 1, 32 copies, 512 threads (see k_spline_hist)
      return with_bool(!occ && a.seg, [&](auto SEG) {  // the table has chunks that run across column-group boundaries (nid_kernels.hpp Segments)
        return with_bool(!occ && a.multi, [&](auto MULTI) {
          return launch_chunks(k_spline_hist<M, Rec, WIDE, MULTI, SEG>, WIDE ? kWideThreads : kThreads, a.lds_hist, a, occ, static_cast<const Rec*>(a.pts), a.chunks, a.gend,
                               a.img, a.pitch, a.W, a.H, pose, cam, a.B, a.GW, a.cshift, a.magic, a.hist, a.prio, a.multi, dyn_of<MULTI>(a));
        });
      });
    });
  });
}

template <typename Rec>
static hipError_t spline_grad_rec(const PassArgs& a, int* occ) {
  const PoseParams<double> pose = make_pose(a);
  const CamParams<double> cam = make_cam(a.model, a.intr, a.dist);
  return with_model(a.model, hipErrorInvalidValue, [&](auto M) {
    return with_bool(a.GW == 1, [&](auto GW1) {
      return with_bool(!occ && a.seg, [&](auto SEG) {
        return with_bool(!occ && a.multi, [&](auto MULTI) {
          if constexpr (SEG && !GW1) {
            return hipErrorInvalidValue;  // multi-segment tables are built for the single-column kernels only
          } else {
            return launch_chunks(k_spline_grad<M, Rec, GW1, MULTI, SEG>, kThreads, a.lds_grad, a, occ, static_cast<const Rec*>(a.pts), a.chunks, a.gend, a.img, a.pitch, a.W,
                                 a.H, pose, cam, a.B, a.GW, a.cshift, a.inv_unit, a.hist, a.phi_q, a.scal, a.gt, a.partials, unsigned(a.nslots), a.q[0], a.q[1], a.q[2], a.q[3], a.out,
                                 a.out_host, a.tag, a.counter, a.prio, a.multi, dyn_of<MULTI>(a));
          }
        });
      });
    });
  });
}

template <typename Rec>
static hipError_t nearest_hist_rec(const PassArgs& a, int* occ) {
  const IsoParams<double> iso = make_iso(a.iso);
  const CamParams<double> cam = make_cam(a.model, a.intr, a.dist);
  return with_model(a.model, hipErrorInvalidValue, [&](auto M) {
    return with_bool(!occ && a.seg, [&](auto SEG) {
      return with_bool(!occ && a.multi, [&](auto MULTI) {
        return launch_chunks(k_nearest_hist<M, Rec, MULTI, SEG>, kThreads, a.lds_hist, a, occ, static_cast<const Rec*>(a.pts), a.chunks, a.gend, a.img, a.pitch, a.W, a.H, iso,
                             cam, a.B, a.GW, a.cshift, a.cos_fov, a.nfast, a.hist, a.multi, dyn_of<MULTI>(a));
      });
    });
  });
}

}  // namespace nidreg
