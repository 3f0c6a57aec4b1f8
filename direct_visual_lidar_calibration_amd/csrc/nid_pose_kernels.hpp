// nid_pose_kernels.hpp -- the rotation RANSAC of PoseEstimation::estimate_rotation_ransac
// (src/vlcal/common/estimate_pose.cpp:40-145) as four kernels:
//   k_ransac_hypotheses  one thread per hypothesis: draw (or take) two correspondences and compute the least-squares
//                        rotation between the two bearing pairs (find_rotation, :55-83) in closed form.
//   k_ransac_score       the hot loop (:114-123), hypotheses x correspondences projections through the camera model.  A
//                        workgroup of 256 threads stages a tile of correspondences (u, v and the LiDAR bearing: 5 doubles,
//                        stored as five arrays) once in dynamic LDS and scores kPoseTileH hypotheses against it, one wave per
//                        hypothesis, lanes over correspondences; the lane counts are summed with wave shuffles and lane 0
//                        adds the tile's count to the hypothesis (a plain store when one tile holds all correspondences).
//   k_ransac_best        the winner (:125-130): largest count, ties to the lowest iteration, as ONE 64-bit atomicMax of
//                        (count << 32) | (0xffffffff - k).  (The reference's `omp critical` keeps whichever thread came first.)
//   k_ransac_flags       the inlier flags of the winning rotation (:135-142) and the result header.
// Compiled with -ffp-contract=off; the projection is the exact-order project<MODEL> the NEAREST / render kernels use, and the
// inlier test is ONE inlined function, so a hypothesis' count and the flags of the winner are the same decisions.
#pragma once
#include "nid_device.hpp"

namespace nidreg {

typedef unsigned long long pose_u64;

constexpr int kPoseThreads = 256;  // four waves
constexpr int kPoseTileC = 1024;   // correspondences per tile at most (5 x 8 KB of LDS)
constexpr int kPoseTileH = 16;     // hypotheses per workgroup: four per wave

// ---- sampling: a counter-based generator of (seed, k) -- splitmix64 rounds -- so that hypothesis k draws the same two
// DISTINCT correspondences whatever grid or thread runs it; the same function on the host (nidreg_ransac_sample_pairs).
// (The reference draws with replacement from mt19937 streams that depend on omp_get_max_threads(), estimate_pose.cpp:90-108;
// a pair that names one correspondence twice is a rank-1 problem whose rotation is arbitrary.)
NID_HD pose_u64 pose_mix(pose_u64 z) {
  z += 0x9e3779b97f4a7c15ULL;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}
NID_HD pose_u64 pose_mulhi(pose_u64 a, pose_u64 b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return pose_u64((static_cast<unsigned __int128>(a) * b) >> 64);
#endif
}
// n >= 2: i uniform in [0, n), j uniform in [0, n) \ {i}
NID_HD void ransac_pair(pose_u64 seed, pose_u64 k, pose_u64 n, int& i, int& j) {
  const pose_u64 h0 = pose_mix(pose_mix(seed) + k);
  const pose_u64 h1 = pose_mix(h0);
  const pose_u64 a = pose_mulhi(h0, n);
  pose_u64 b = pose_mulhi(h1, n - 1);
  if (b >= a) b++;
  i = int(a);
  j = int(b);
}

// ---- rotation: R = U diag(1, 1, det U det V) V^T of the SVD of A B^T = a1 b1^T + a2 b2^T (camera bearings a, LiDAR bearings
// b; estimate_pose.cpp:68-81).  For unit vectors a1 + a2 is orthogonal to a1 - a2 (and likewise for b), so
//   A B^T = 1/2 [(a1 + a2)(b1 + b2)^T + (a1 - a2)(b1 - b2)^T]
// IS a singular value decomposition: singular vectors (a+^, b+^) and (a-^, b-^), third singular value 0, and the third pair
// fixed by the determinant rule, (a+^ x a-^)(b+^ x b-^)^T.  Coincident or opposite bearings (a- = 0 or a+ = 0) have no such
// rotation: the result is NaN and the hypothesis counts no inlier.
NID_HD void pose_unit(double* v) {
  const double n2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
  const double s = 1.0 / sqrt(n2);  // n2 = 0: inf, 0 * inf = NaN
  v[0] *= s, v[1] *= s, v[2] *= s;
}
NID_HD void two_vector_rotation(const double* a1, const double* a2, const double* b1, const double* b2, double* R) {
  double ap[3], am[3], bp[3], bm[3];
  for (int c = 0; c < 3; c++) {
    ap[c] = a1[c] + a2[c], am[c] = a1[c] - a2[c];
    bp[c] = b1[c] + b2[c], bm[c] = b1[c] - b2[c];
  }
  pose_unit(ap), pose_unit(am), pose_unit(bp), pose_unit(bm);
  const double ac[3] = {ap[1] * am[2] - ap[2] * am[1], ap[2] * am[0] - ap[0] * am[2], ap[0] * am[1] - ap[1] * am[0]};
  const double bc[3] = {bp[1] * bm[2] - bp[2] * bm[1], bp[2] * bm[0] - bp[0] * bm[2], bp[0] * bm[1] - bp[1] * bm[0]};
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) R[3 * r + c] = (ap[r] * bp[c] + am[r] * bm[c]) + ac[r] * bc[c];
}

__global__ __launch_bounds__(kPoseThreads) void k_ransac_hypotheses(
  const double* __restrict__ dirs_camera, const double* __restrict__ dirs_lidar, int n, int iterations, pose_u64 seed, const int* __restrict__ pairs_in, double* __restrict__ Rs) {
  const int k = int(blockIdx.x) * kPoseThreads + int(threadIdx.x);
  if (k >= iterations) return;
  int i, j;
  if (pairs_in) {
    i = pairs_in[2 * k], j = pairs_in[2 * k + 1];  // (range-checked on the host)
  } else {
    ransac_pair(seed, pose_u64(k), pose_u64(n), i, j);
  }
  double R[9];
  two_vector_rotation(dirs_camera + 3 * size_t(i), dirs_camera + 3 * size_t(j), dirs_lidar + 3 * size_t(i), dirs_lidar + 3 * size_t(j), R);
  for (int r = 0; r < 9; r++) Rs[9 * size_t(k) + r] = R[r];
}

// (kp - project(R d_lidar)).squaredNorm() < thresh^2 (estimate_pose.cpp:117-120); false when the projection is not finite
template <int MODEL>
__device__ __forceinline__ bool pose_inlier(const CamParams<double>& cam, const double* R, double ku, double kv, double x, double y, double z, double thresh_sq) {
  const double cx = (R[0] * x + R[1] * y) + R[2] * z;
  const double cy = (R[3] * x + R[4] * y) + R[5] * z;
  const double cz = (R[6] * x + R[7] * y) + R[8] * z;
  double u, v;
  project<MODEL, double, double, false>(cam, cx, cy, cz, u, v);
  const double du = ku - u, dv = kv - v;
  return du * du + dv * dv < thresh_sq;
}

// corr: five arrays of n doubles (u, v, x, y, z).  Workgroup b scores hypotheses [ht * kPoseTileH, +kPoseTileH) against
// correspondences [ct * tile, +tile) with ht = b / ntiles, ct = b % ntiles; dynamic LDS = 5 * tile doubles.
template <int MODEL>
__global__ __launch_bounds__(kPoseThreads) void k_ransac_score(
  const double* __restrict__ corr, int n, int tile, int ntiles, const double* __restrict__ Rs, int iterations, CamParams<double> cam, double thresh_sq, int* __restrict__ counts) {
  extern __shared__ double pose_lds[];
  const int ht = int(blockIdx.x) / ntiles, ct = int(blockIdx.x) % ntiles;
  const int c0 = ct * tile;
  const int m = min(tile, n - c0);
  for (int a = 0; a < 5; a++)
    for (int i = int(threadIdx.x); i < m; i += kPoseThreads) pose_lds[a * tile + i] = corr[size_t(a) * size_t(n) + size_t(c0 + i)];
  __syncthreads();
  const double* su = pose_lds;
  const double* sv = pose_lds + tile;
  const double* sx = pose_lds + 2 * tile;
  const double* sy = pose_lds + 3 * tile;
  const double* sz = pose_lds + 4 * tile;
  const int wave = int(threadIdx.x) >> 6, lane = int(threadIdx.x) & 63;
  for (int hh = wave; hh < kPoseTileH; hh += kPoseThreads / 64) {
    const int k = ht * kPoseTileH + hh;
    if (k >= iterations) break;  // (the same for every lane of the wave)
    double R[9];
    for (int r = 0; r < 9; r++) R[r] = Rs[9 * size_t(k) + r];
    int c = 0;
    for (int j = lane; j < m; j += 64) c += pose_inlier<MODEL>(cam, R, su[j], sv[j], sx[j], sy[j], sz[j], thresh_sq) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) {
      if (ntiles == 1)
        counts[k] = c;
      else
        atomicAdd(&counts[k], c);
    }
  }
}

__global__ __launch_bounds__(kPoseThreads) void k_ransac_best(const int* __restrict__ counts, int iterations, pose_u64* __restrict__ best) {
  const int k = int(blockIdx.x) * kPoseThreads + int(threadIdx.x);
  pose_u64 key = 0;
  if (k < iterations) key = (pose_u64(unsigned(counts[k])) << 32) | pose_u64(0xffffffffu - unsigned(k));
  for (int o = 32; o > 0; o >>= 1) {
    const pose_u64 other = __shfl_xor(key, o);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(best, key);
}

// flags[j] of the winner; workgroup 0 also writes the winning rotation behind the key (R_out: 9 doubles)
template <int MODEL>
__global__ __launch_bounds__(kPoseThreads) void k_ransac_flags(
  const double* __restrict__ corr, int n, const double* __restrict__ Rs, const pose_u64* __restrict__ best, CamParams<double> cam, double thresh_sq, unsigned char* __restrict__ flags,
  double* __restrict__ R_out) {
  const unsigned k = 0xffffffffu - unsigned(*best & 0xffffffffULL);
  double R[9];
  for (int r = 0; r < 9; r++) R[r] = Rs[9 * size_t(k) + r];
  if (blockIdx.x == 0 && threadIdx.x < 9) R_out[threadIdx.x] = R[threadIdx.x];
  const int j = int(blockIdx.x) * kPoseThreads + int(threadIdx.x);
  if (j >= n) return;
  const size_t N = size_t(n);
  flags[j] = pose_inlier<MODEL>(cam, R, corr[j], corr[N + j], corr[2 * N + j], corr[3 * N + j], corr[4 * N + j], thresh_sq) ? 1 : 0;
}

}  // namespace nidreg
