// nidreg_pose.hip -- C ABI of the initial guess (include/nidreg.h: nidreg_estimate_directions, nidreg_ransac_sample_pairs,
// nidreg_estimate_rotation_ransac): vlcal::estimate_direction on the host (shared with nidreg_estimate_camera_fov) and the
// rotation RANSAC of PoseEstimation on the device (kernels: nid_pose_kernels.hpp).  The reprojection least squares that follows
// (estimate_pose.cpp:148-177) is host work in the reference and lives in pose.py.
#include "nid_pose_kernels.hpp"
#include "nid_launch.hpp"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

namespace nidreg {

/* vlcal::estimate_direction (src/vlcal/common/estimate_fov.cpp:17-34): the bearing that projects onto the pixel (pu, pv), found
 * by NelderMead<2> (include/dfo/nelder_mead.hpp:32-113, defaults) over two rotation angles, on the device's scalar projection
 * code compiled for the host (project_host).  ~80 projections of ONE point: host work in the reference and here. */
void estimate_direction_host(int model_id, const double* intr5, const double* dist8, double pu, double pv, double* dir3) {
  // AngleAxis(x0, X) * AngleAxis(x1, Y) * UnitZ through quaternions, as Eigen evaluates it (estimate_fov.cpp:19-21)
  auto to_dir = [](const double* x, double* d) {
    const double aw = std::cos(0.5 * x[0]), ax = std::sin(0.5 * x[0]);
    const double bw = std::cos(0.5 * x[1]), by = std::sin(0.5 * x[1]);
    const double qw = aw * bw, qx = ax * bw, qy = aw * by, qz = ax * by;
    const double ux = 2.0 * qy, uy = -2.0 * qx, uz = 0.0;  // 2 (vec x ez)
    d[0] = qw * ux + (qy * uz - qz * uy);
    d[1] = qw * uy + (qz * ux - qx * uz);
    d[2] = (1.0 + qw * uz) + (qx * uy - qy * ux);
  };
  auto f = [&](const double* x) {
    double d[3], uv[2];
    to_dir(x, d);
    if (project_host(model_id, intr5, dist8, d, 1, uv, nullptr) != 0) return std::numeric_limits<double>::max();
    const double e = (pu - uv[0]) * (pu - uv[0]) + (pv - uv[1]) * (pv - uv[1]);
    return std::isfinite(e) ? e : std::numeric_limits<double>::max();
  };
  // NelderMead<2>: rows (y, x0, x1), init_step 0.1, (alpha, gamma, rho) = (1, 2, 0.5), 1024 iterations, variance threshold 1e-5
  std::array<std::array<double, 3>, 3> x;
  for (int i = 0; i < 3; i++) {
    x[size_t(i)] = {0.0, 0.0, 0.0};
    if (i > 0) x[size_t(i)][size_t(i)] += 0.1;
    x[size_t(i)][0] = f(&x[size_t(i)][1]);
  }
  for (int it = 0; it < 1024; it++) {
    std::stable_sort(x.begin(), x.end(), [](const std::array<double, 3>& a, const std::array<double, 3>& b) { return a[0] < b[0]; });
    double var = 0.0;
    for (int k = 1; k < 3; k++) {
      const double m = ((x[0][size_t(k)] + x[1][size_t(k)]) + x[2][size_t(k)]) / 3.0;
      double v = 0.0;
      for (int i = 0; i < 3; i++) v += (x[size_t(i)][size_t(k)] - m) * (x[size_t(i)][size_t(k)] - m);
      var += v;
    }
    if (var < 1e-5) break;
    std::array<double, 3> xo, xr;
    for (int k = 1; k < 3; k++) xo[size_t(k)] = (x[0][size_t(k)] + x[1][size_t(k)]) / 2.0;
    xo[0] = f(&xo[1]);
    for (int k = 1; k < 3; k++) xr[size_t(k)] = xo[size_t(k)] + 1.0 * (xo[size_t(k)] - x[2][size_t(k)]);
    xr[0] = f(&xr[1]);
    if (x[0][0] <= xr[0] && xr[0] < x[1][0]) {
      x[2] = xr;
    } else if (xr[0] < x[0][0]) {
      std::array<double, 3> xe;
      for (int k = 1; k < 3; k++) xe[size_t(k)] = xo[size_t(k)] + 2.0 * (xo[size_t(k)] - x[2][size_t(k)]);
      xe[0] = f(&xe[1]);
      x[2] = xe[0] < xr[0] ? xe : xr;
    } else {
      std::array<double, 3> xc;
      for (int k = 1; k < 3; k++) xc[size_t(k)] = xo[size_t(k)] + 0.5 * (xo[size_t(k)] - x[2][size_t(k)]);
      xc[0] = f(&xc[1]);
      if (xc[0] < x[2][0]) {
        x[2] = xc;
      } else {
        for (int j = 1; j < 3; j++) {
          for (int k = 1; k < 3; k++) x[size_t(j)][size_t(k)] = x[0][size_t(k)] + 0.5 * (x[size_t(j)][size_t(k)] - x[0][size_t(k)]);
          x[size_t(j)][0] = f(&x[size_t(j)][1]);
        }
      }
    }
  }
  // result.x = x[0] of the LAST SORT INSIDE the loop (nelder_mead.hpp:97-98): after 1024 iterations without convergence the
  // reference does not sort again, and neither does this
  to_dir(&x[0][1], dir3);
}

namespace {

hipError_t launch_ransac_score(int model, const double* d_corr, int n, int tile, int ntiles, const double* d_Rs, int iterations, const CamParams<double>& cam, double thresh_sq,
                               int* d_counts) {
  const unsigned grid = blocks_for(iterations, kPoseTileH) * unsigned(ntiles);
  const size_t lds = size_t(5) * size_t(tile) * sizeof(double);  // <= 40 KB
  return with_model(model, hipErrorInvalidValue, [&](auto M) {
    return launch(k_ransac_score<M>, grid, kPoseThreads, lds, nullptr, d_corr, n, tile, ntiles, d_Rs, iterations, cam, thresh_sq, d_counts);
  });
}

hipError_t launch_ransac_flags(int model, const double* d_corr, int n, const double* d_Rs, const pose_u64* d_best, const CamParams<double>& cam, double thresh_sq,
                               unsigned char* d_flags, double* d_R_out) {
  return with_model(model, hipErrorInvalidValue, [&](auto M) {
    return launch(k_ransac_flags<M>, blocks_for(n, kPoseThreads), kPoseThreads, 0, nullptr, d_corr, n, d_Rs, d_best, cam, thresh_sq, d_flags, d_R_out);
  });
}

}  // namespace
}  // namespace nidreg

using namespace nidreg;

extern "C" {

int nidreg_estimate_directions(int model_id, const double* intrinsics, const double* distortion, const double* uv, int64_t n, double* dirs3) {
  if (model_id < 0 || model_id > 5 || !intrinsics || !distortion || n < 0 || (n > 0 && (!uv || !dirs3))) return fail(NIDREG_ERR_INVALID, "nidreg_estimate_directions: bad argument");
  double intr5[5], dist8[8];
  std::memcpy(intr5, intrinsics, sizeof(intr5));
  std::memcpy(dist8, distortion, sizeof(dist8));
  // pixels are independent: contiguous slices over at most 16 host threads (the reference's loop is sequential, estimate_pose.cpp:48-51)
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const int64_t nthreads = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(16, int64_t(hw)), n / 8));
  auto work = [&](int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; i++) estimate_direction_host(model_id, intr5, dist8, uv[2 * i], uv[2 * i + 1], dirs3 + 3 * i);
  };
  if (nthreads == 1) {
    work(0, n);
    return NIDREG_OK;
  }
  std::vector<std::thread> pool;
  for (int64_t t = 0; t < nthreads; t++) pool.emplace_back(work, n * t / nthreads, n * (t + 1) / nthreads);
  for (auto& t : pool) t.join();
  return NIDREG_OK;
}

int nidreg_ransac_sample_pairs(uint64_t seed, int64_t n, int iterations, int32_t* pairs) {
  if (n < 2 || n > 2147483647LL || iterations < 0 || (iterations > 0 && !pairs)) return fail(NIDREG_ERR_INVALID, "nidreg_ransac_sample_pairs: bad argument");
  for (int k = 0; k < iterations; k++) {
    int i, j;
    ransac_pair(pose_u64(seed), pose_u64(k), pose_u64(n), i, j);
    pairs[2 * k] = i, pairs[2 * k + 1] = j;
  }
  return NIDREG_OK;
}

int nidreg_estimate_rotation_ransac(int model_id, const double* intrinsics, const double* distortion, int device_id, const double* kpts2, const double* dirs_camera3,
                                    const double* dirs_lidar3, int64_t n, int iterations, double error_thresh, uint64_t seed, const int32_t* sample_pairs, double* R9,
                                    int32_t* best_iteration, int32_t* best_inliers, uint8_t* inlier_flags, int32_t* counts) {
  if (model_id < 0 || model_id > 5 || !intrinsics || !distortion || !kpts2 || !dirs_camera3 || !dirs_lidar3 || !R9 || !best_iteration || !best_inliers)
    return fail(NIDREG_ERR_INVALID, "nidreg_estimate_rotation_ransac: null argument or unknown camera model");
  if (iterations <= 0 || n < 2 || n > 2147483647LL) return fail(NIDREG_ERR_INVALID, "nidreg_estimate_rotation_ransac: iterations must be positive and 2 <= n <= INT_MAX");
  const int N = int(n);
  const int tile = std::min(kPoseTileC, (N + 63) / 64 * 64);
  const int ntiles = (N + tile - 1) / tile;
  if (int64_t((iterations + kPoseTileH - 1) / kPoseTileH) * ntiles > 2147483647LL)
    return fail(NIDREG_ERR_INVALID, "nidreg_estimate_rotation_ransac: iterations x correspondences beyond one grid");
  if (sample_pairs)
    for (int64_t k = 0; k < 2 * int64_t(iterations); k++)
      if (sample_pairs[k] < 0 || sample_pairs[k] >= N) return fail(NIDREG_ERR_INVALID, "nidreg_estimate_rotation_ransac: sample_pairs index out of range");
  if (const int rc = use_device("nidreg_estimate_rotation_ransac", device_id)) return rc;

  // one upload: correspondences as five arrays (u, v, LiDAR bearing x, y, z), then the two bearing arrays as given
  const size_t sn = size_t(N), it = size_t(iterations);
  std::vector<double> in(11 * sn);
  for (size_t i = 0; i < sn; i++) {
    in[i] = kpts2[2 * i], in[sn + i] = kpts2[2 * i + 1];
    for (size_t c = 0; c < 3; c++) in[(2 + c) * sn + i] = dirs_lidar3[3 * i + c];
  }
  std::memcpy(in.data() + 5 * sn, dirs_camera3, 3 * sn * sizeof(double));
  std::memcpy(in.data() + 8 * sn, dirs_lidar3, 3 * sn * sizeof(double));
  // one result block: [0] the winner's key, [1..9] its rotation, then the counts and the flags
  const size_t off_counts = 10 * sizeof(double), off_flags = off_counts + it * sizeof(int), res_bytes = off_flags + sn;
  DeviceBuf d_in, d_Rs, d_pairs_in, d_res;
  HIP_TRY(d_in.alloc(in.size() * sizeof(double)));
  HIP_TRY(d_Rs.alloc(9 * it * sizeof(double)));
  HIP_TRY(d_res.alloc(res_bytes));
  HIP_TRY(hipMemcpy(d_in.as<void>(), in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice));
  if (sample_pairs) {
    HIP_TRY(d_pairs_in.alloc(2 * it * sizeof(int)));
    HIP_TRY(hipMemcpy(d_pairs_in.as<void>(), sample_pairs, 2 * it * sizeof(int), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemsetAsync(d_res.as<void>(), 0, off_flags, nullptr));  // key 0 and zero counts
  char* const res = d_res.as<char>();
  pose_u64* const d_best = reinterpret_cast<pose_u64*>(res);
  double* const d_R_out = reinterpret_cast<double*>(res) + 1;
  int* const d_counts = reinterpret_cast<int*>(res + off_counts);
  unsigned char* const d_flags = reinterpret_cast<unsigned char*>(res + off_flags);
  const double* const d_corr = d_in.as<double>();
  const CamParams<double> cam = make_cam(model_id, intrinsics, distortion);
  const double thresh_sq = error_thresh * error_thresh;
  const unsigned hgrid = blocks_for(iterations, kPoseThreads);
  HIP_TRY(launch(k_ransac_hypotheses, hgrid, kPoseThreads, 0, nullptr, d_corr + 5 * sn, d_corr + 8 * sn, N, iterations, seed, d_pairs_in.as<int>(), d_Rs.as<double>()));
  HIP_TRY(launch_ransac_score(model_id, d_corr, N, tile, ntiles, d_Rs.as<double>(), iterations, cam, thresh_sq, d_counts));
  HIP_TRY(launch(k_ransac_best, hgrid, kPoseThreads, 0, nullptr, d_counts, iterations, d_best));
  HIP_TRY(launch_ransac_flags(model_id, d_corr, N, d_Rs.as<double>(), d_best, cam, thresh_sq, d_flags, d_R_out));
  std::vector<unsigned char> out(res_bytes);
  HIP_TRY(hipMemcpy(out.data(), d_res.as<void>(), res_bytes, hipMemcpyDeviceToHost));  // (synchronises the null stream)
  pose_u64 key;
  std::memcpy(&key, out.data(), sizeof(key));
  std::memcpy(R9, out.data() + sizeof(double), 9 * sizeof(double));
  *best_iteration = int32_t(0xffffffffu - unsigned(key & 0xffffffffULL));
  *best_inliers = int32_t(key >> 32);
  if (counts) std::memcpy(counts, out.data() + off_counts, it * sizeof(int));
  if (inlier_flags) std::memcpy(inlier_flags, out.data() + off_flags, sn);
  return NIDREG_OK;
}

}  // extern "C"
