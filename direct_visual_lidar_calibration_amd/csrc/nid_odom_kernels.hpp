// nid_odom_kernels.hpp -- the device side of vlcal::DynamicPointCloudIntegrator (src/vlcal/preprocess/dynamic_point_cloud_integrator.cpp):
// continuous-time GICP of one scan against a running model, and the deskewed insert of the whole raw scan into the voxel table.
//   k_odom_knn           kNN among the M sampled points of a scan (KdTree2::knn_search, :57-64), brute force: one lane per query,
//                        the cloud streamed through LDS in tiles of 64 points, every lane's k best kept sorted by ascending
//                        (d^2, index) in LDS (slot-major: conflict-free).
//   k_odom_cov           CloudCovarianceEstimation::estimate(points, neighbors) (cloud_covariance_estimation.cpp:77-112): the
//                        covariance of a neighbour list (divided by k - 1) and its PLANE regularisation (:133-148).
//                        V diag(1e-3, 1, 1) V^-1 = I - 0.999 n n^T with n the eigenvector of the smallest eigenvalue, so only n
//                        is computed: the closed-form symmetric 3x3 solver of Eigen's computeDirect (shift by the mean eigenvalue,
//                        scale by the largest coefficient, trigonometric roots, cross products for the kernel of A - lambda I of
//                        the better separated end); where that end is the largest eigenvalue, n comes from the 2 x 2 problem in
//                        its eigenvector's orthogonal complement.
//   k_odom_model_insert  iVox::insert (ivox.cpp:122-166): a hash of 1 m voxels (the integrator's packed
//                        64-bit key), each voxel an ordered list of points with their covariances in chained blocks of 64 from a
//                        pool.  LinearContainer::insert's rule (:29-50) is sequential -- a point enters iff its squared distance to
//                        EVERY point already in its voxel is > thresh --, so the scan's points arrive grouped by voxel (ascending
//                        index inside a group) and ONE wave walks one group in order, its lanes testing a candidate against a block.
//                        Every voxel a scan offers a point to is stamped with the insert's count (:164), a refused point included.
//   k_odom_evict         the LRU pass of iVox::insert (:168-178): every voxel whose stamp lies below the horizon leaves.  The table
//                        is open addressing with linear probing, so nothing is erased in place: one thread per old slot moves a
//                        survivor (head, tail, count and stamp kept) into a second, zeroed table of the same size, or walks a
//                        leaving voxel's chain and pushes its blocks onto the free stack odom_alloc_block pops from; the host
//                        then swaps the two tables.  No tombstones, and the new table holds no more voxels than the old one, so
//                        odom_find's invariant holds after every pass.  Which slot or block id a voxel gets may differ from run
//                        to run, as before; no result depends on either.  NOT built: the "too many voxels" branch (:181-197),
//                        which takes 2^32 - 1 voxels and cannot be reached with a table of at most 2^25 slots.
//   k_odom_linearize     IntegratedCT_GICPFactor_::update_correspondences + linearize (integrated_ct_gicp_factor_impl.hpp:70-177):
//                        per source point the pose of its time index, the nearest model point over the 7 face-neighbour voxels
//                        (iVox::nearest_neighbor_search, ivox.cpp:207-245), the Mahalanobis matrix, and the point's terms of H_00,
//                        H_01, H_11, b_0, b_1, the error and the inlier count.  With the eviction on (the Touch instantiation) every
//                        neighbour voxel the search finds in the table is stamped with the current count (:223).
//   k_odom_error         ::error (:40-67) on the stored correspondences and Mahalanobis matrices at other poses.
//   k_odom_sum           the per-wave partials of the two kernels above, summed in wave order.
//   k_odom_deskew        voxelgrid_task (dynamic_point_cloud_integrator.cpp:123-155) up to the voxel insert: the raw
//                        sensor_msgs/PointCloud2 records decoded, the pose interpolateRt(T_begin, T_end, time / max_time) evaluated
//                        PER POINT and applied; the transformed frame then goes through the integrator's own passes.
// No floating-point atomics anywhere: sums are wave reductions with a fixed tree and per-wave partials added in wave order, so
// every result has the same bits from run to run.  All arithmetic is fp64, compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nid_voxel_kernels.hpp"

namespace nidreg {

constexpr int kOdomMaxK = 32;          // neighbours per point
constexpr int kOdomWave = 64;          // every kernel here runs workgroups of one wave
constexpr int kOdomBlockPoints = 64;   // points per pool block
constexpr int kOdomSums = 122;         // H_00 (36) H_01 (36) H_11 (36) b_0 (6) b_1 (6) error count
constexpr int kOdomPoseDoubles = 84;   // per time-table entry: R (9, row-major) t (3) d pose / d pose_0 (36) d pose / d pose_1 (36)

struct OdomBlock {  // structure of arrays: lane l of the walking wave reads point l
  double p[3][kOdomBlockPoints];
  double c[6][kOdomBlockPoints];  // xx xy xz yy yz zz
};
struct OdomVoxel {
  vox_u64 key;  // packed voxel + 1; 0 = empty
  int head, tail;  // first and last block of the chain
  int count;       // points in the voxel
  int last_lru_count;  // the count of the last insert that offered it a point, or after which a search found it (ivox.cpp:164, :223)
};

// the integrator's packed key of floor(p / res); false outside [-2^20, 2^20) on an axis or for a non-finite coordinate
__host__ __device__ inline bool odom_key(double x, double y, double z, double res, vox_u64& key) {
  const double fx = floor(x / res), fy = floor(y / res), fz = floor(z / res);
  const double L = double(kVoxAxisLimit);
  if (!(fx >= -L && fx < L && fy >= -L && fy < L && fz >= -L && fz < L)) return false;
  key = (vox_u64((long long)fx + kVoxAxisLimit) | (vox_u64((long long)fy + kVoxAxisLimit) << 21) | (vox_u64((long long)fz + kVoxAxisLimit) << 42)) + 1ULL;
  return true;
}

__device__ inline int odom_find(const OdomVoxel* table, unsigned mask, vox_u64 key) {
  // every voxel in the table owns a block and the table has >= 2 x max_blocks slots, so it is never more than half full and the
  // probe meets an empty slot; the bound only keeps a corrupted table from spinning
  unsigned h = unsigned(vox_mix(key)) & mask;
  for (unsigned probes = 0; probes <= mask; probes++) {
    const vox_u64 k = table[h].key;
    if (k == key) return int(h);
    if (k == 0) return -1;
    h = (h + 1) & mask;
  }
  return -1;
}

// ---- kNN ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kOdomWave) void k_odom_knn(const double* pts /* M x 3 */, int M, int k, int* nbr /* M x k */) {
  __shared__ double tile[3][kOdomWave];
  __shared__ double bd[kOdomMaxK][kOdomWave];
  __shared__ int bi[kOdomMaxK][kOdomWave];
  const int t = threadIdx.x, i = blockIdx.x * kOdomWave + t;
  const bool live = i < M;
  double qx = 0.0, qy = 0.0, qz = 0.0;
  if (live) qx = pts[3 * i], qy = pts[3 * i + 1], qz = pts[3 * i + 2];
  int have = 0;
  for (int j0 = 0; j0 < M; j0 += kOdomWave) {
    __syncthreads();  // the previous tile has been read
    if (j0 + t < M) tile[0][t] = pts[3 * (j0 + t)], tile[1][t] = pts[3 * (j0 + t) + 1], tile[2][t] = pts[3 * (j0 + t) + 2];
    __syncthreads();
    const int cnt = M - j0 < kOdomWave ? M - j0 : kOdomWave;
    if (!live) continue;
    for (int jj = 0; jj < cnt; jj++) {
      const double dx = qx - tile[0][jj], dy = qy - tile[1][jj], dz = qz - tile[2][jj];
      const double d = (dx * dx + dy * dy) + dz * dz;
      int pos;
      if (have < k) pos = have++;
      else if (d < bd[k - 1][t]) pos = k - 1;
      else continue;
      while (pos > 0 && bd[pos - 1][t] > d) {  // (candidates come in ascending index: an equal distance stays behind the earlier one)
        bd[pos][t] = bd[pos - 1][t], bi[pos][t] = bi[pos - 1][t];
        pos--;
      }
      bd[pos][t] = d, bi[pos][t] = j0 + jj;
    }
  }
  if (live)
    for (int s = 0; s < k; s++) nbr[(long long)i * k + s] = bi[s][t];
}

// ---- covariance + PLANE regularisation ------------------------------------------------------------------------------------------
// unit vector of the kernel of the (singular) symmetric matrix m (lower triangle m00 m10 m11 m20 m21 m22): Eigen's extract_kernel;
// false when every cross product vanishes (rank <= 1)
__device__ inline bool odom_kernel_vec(double m00, double m10, double m11, double m20, double m21, double m22, double* v) {
  const double a0 = fabs(m00), a1 = fabs(m11), a2 = fabs(m22);
  const int i0 = (a0 >= a1 && a0 >= a2) ? 0 : (a1 >= a2 ? 1 : 2);
  const double col[3][3] = {{m00, m10, m20}, {m10, m11, m21}, {m20, m21, m22}};
  const double* r = col[i0];
  const double* p = col[(i0 + 1) % 3];
  const double* q = col[(i0 + 2) % 3];
  const double c0[3] = {r[1] * p[2] - r[2] * p[1], r[2] * p[0] - r[0] * p[2], r[0] * p[1] - r[1] * p[0]};
  const double c1[3] = {r[1] * q[2] - r[2] * q[1], r[2] * q[0] - r[0] * q[2], r[0] * q[1] - r[1] * q[0]};
  const double n0 = (c0[0] * c0[0] + c0[1] * c0[1]) + c0[2] * c0[2], n1 = (c1[0] * c1[0] + c1[1] * c1[1]) + c1[2] * c1[2];
  const double* c = n0 > n1 ? c0 : c1;
  const double nn = n0 > n1 ? n0 : n1;
  if (!(nn > 0.0) || !isfinite(nn)) return false;
  const double s = sqrt(nn);
  v[0] = c[0] / s, v[1] = c[1] / s, v[2] = c[2] / s;
  return true;
}

// the unit eigenvector of the smallest eigenvalue of the symmetric matrix (lower triangle); always finite for finite input
__device__ inline void odom_smallest_eigvec(double a00, double a10, double a11, double a20, double a21, double a22, double* n) {
  n[0] = 1.0, n[1] = 0.0, n[2] = 0.0;  // what computeDirect returns for a multiple of the identity: the identity's first column
  const double shift = (a00 + a11 + a22) / 3.0;
  double m00 = a00 - shift, m11 = a11 - shift, m22 = a22 - shift, m10 = a10, m20 = a20, m21 = a21;
  double scale = fmax(fmax(fabs(m00), fabs(m11)), fmax(fabs(m22), fmax(fabs(m10), fmax(fabs(m20), fabs(m21)))));
  if (!(scale > 0.0) || !isfinite(scale)) return;
  m00 /= scale, m11 /= scale, m22 /= scale, m10 /= scale, m20 /= scale, m21 /= scale;
  // computeRoots
  const double c0 = m00 * m11 * m22 + 2.0 * m10 * m20 * m21 - m00 * m21 * m21 - m11 * m20 * m20 - m22 * m10 * m10;
  const double c1 = m00 * m11 - m10 * m10 + m00 * m22 - m20 * m20 + m11 * m22 - m21 * m21;
  const double c2 = m00 + m11 + m22;
  const double c2_3 = c2 / 3.0;
  double a_3 = (c2 * c2_3 - c1) / 3.0;
  a_3 = a_3 > 0.0 ? a_3 : 0.0;
  const double half_b = 0.5 * (c0 + c2_3 * (2.0 * c2_3 * c2_3 - c1));
  double q = a_3 * a_3 * a_3 - half_b * half_b;
  q = q > 0.0 ? q : 0.0;
  const double rho = sqrt(a_3), theta = atan2(sqrt(q), half_b) / 3.0;
  const double ct = cos(theta), st = sin(theta), s3 = 1.7320508075688772;
  const double l0 = c2_3 - rho * (ct + s3 * st), l1 = c2_3 - rho * (ct - s3 * st), l2 = c2_3 + 2.0 * rho * ct;
  const double eps = 2.220446049250313e-16;
  if (!(l2 - l0 > eps)) return;
  const double d_hi = l2 - l1, d_lo = l1 - l0;
  double v[3];
  if (d_lo >= d_hi) {  // the smallest eigenvalue is the better separated end: its kernel directly
    if (odom_kernel_vec(m00 - l0, m10, m11 - l0, m20, m21, m22 - l0, v)) n[0] = v[0], n[1] = v[1], n[2] = v[2];
    return;
  }
  // The LARGEST eigenvalue is the better separated end.  The trigonometric roots lose digits where two of them are close (q above is a
  // difference of nearly equal numbers): l0 and l1 move with theta to first order, l2 only to second.  The kernel of A - l0 I then
  // carries an error of (error of l0) / (l1 - l0), 2e-6 for a strip of points 1000 times longer than wide, where LAPACK's
  // iteration has 1e-10.  So the well-separated eigenvector comes first, and the smallest one from the 2 x 2 problem in its
  // orthogonal complement, whose closed form has no such cancellation.
  if (!odom_kernel_vec(m00 - l2, m10, m11 - l2, m20, m21, m22 - l2, v)) return;
  double u[3];  // Eigen's unitOrthogonal of v, then w = v x u
  if (fabs(v[0]) > fabs(v[2]) || fabs(v[1]) > fabs(v[2])) {
    const double s = sqrt(v[0] * v[0] + v[1] * v[1]);
    u[0] = -v[1] / s, u[1] = v[0] / s, u[2] = 0.0;
  } else {
    const double s = sqrt(v[1] * v[1] + v[2] * v[2]);
    u[0] = 0.0, u[1] = -v[2] / s, u[2] = v[1] / s;
  }
  const double w[3] = {v[1] * u[2] - v[2] * u[1], v[2] * u[0] - v[0] * u[2], v[0] * u[1] - v[1] * u[0]};
  const double mu[3] = {(m00 * u[0] + m10 * u[1]) + m20 * u[2], (m10 * u[0] + m11 * u[1]) + m21 * u[2], (m20 * u[0] + m21 * u[1]) + m22 * u[2]};
  const double mw[3] = {(m00 * w[0] + m10 * w[1]) + m20 * w[2], (m10 * w[0] + m11 * w[1]) + m21 * w[2], (m20 * w[0] + m21 * w[1]) + m22 * w[2]};
  // [a b; b c] = [u w]^T A [u w]; its smaller eigenvalue is (a + c) / 2 - r, the eigenvector (b, -h - r) or (h - r, b): the one whose
  // difference adds magnitudes
  const double a = (u[0] * mu[0] + u[1] * mu[1]) + u[2] * mu[2], b = (u[0] * mw[0] + u[1] * mw[1]) + u[2] * mw[2], c = (w[0] * mw[0] + w[1] * mw[1]) + w[2] * mw[2];
  const double h = 0.5 * (a - c), r = sqrt(h * h + b * b);
  double x = h >= 0.0 ? b : h - r, y = h >= 0.0 ? -h - r : b;
  const double s = sqrt(x * x + y * y);
  if (!(s > 0.0) || !isfinite(s)) {  // the two small eigenvalues coincide (a line of points): any unit vector orthogonal to v
    n[0] = u[0], n[1] = u[1], n[2] = u[2];
    return;
  }
  x /= s, y /= s;
  n[0] = x * u[0] + y * w[0], n[1] = x * u[1] + y * w[1], n[2] = x * u[2] + y * w[2];
}

__global__ __launch_bounds__(kOdomWave) void k_odom_cov(const double* pts, const int* nbr, int M, int k, double* normals /* M x 3 */, double* covs /* M x 6 */) {
  const int i = blockIdx.x * kOdomWave + threadIdx.x;
  if (i >= M) return;
  double sx = 0.0, sy = 0.0, sz = 0.0, cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
  for (int j = 0; j < k; j++) {
    const int idx = nbr[(long long)i * k + j];  // (validated on the host: 0 <= idx < M)
    const double x = pts[3 * idx], y = pts[3 * idx + 1], z = pts[3 * idx + 2];
    sx += x, sy += y, sz += z;
    cxx += x * x, cxy += x * y, cxz += x * z, cyy += y * y, cyz += y * z, czz += z * z;
  }
  const double kd = double(k), km1 = double(k - 1);
  const double mx = sx / kd, my = sy / kd, mz = sz / kd;
  // the lower triangle of (sum_cross - mean * sum_points^T) / (k - 1), which is what computeDirect reads
  const double a00 = (cxx - mx * sx) / km1, a10 = (cxy - my * sx) / km1, a11 = (cyy - my * sy) / km1;
  const double a20 = (cxz - mz * sx) / km1, a21 = (cyz - mz * sy) / km1, a22 = (czz - mz * sz) / km1;
  double n[3];
  odom_smallest_eigvec(a00, a10, a11, a20, a21, a22, n);
  normals[3 * i] = n[0], normals[3 * i + 1] = n[1], normals[3 * i + 2] = n[2];
  double* c = covs + 6LL * i;
  c[0] = 1.0 - 0.999 * (n[0] * n[0]), c[1] = -0.999 * (n[0] * n[1]), c[2] = -0.999 * (n[0] * n[2]);
  c[3] = 1.0 - 0.999 * (n[1] * n[1]), c[4] = -0.999 * (n[1] * n[2]), c[5] = 1.0 - 0.999 * (n[2] * n[2]);
}

// ---- the model --------------------------------------------------------------------------------------------------------------------
// counters: [0] blocks handed out by the bump counter (the pool's high-water mark), [1] voxels, [2] points, [3] set when the pool ran
// dry, [4] blocks on the free stack, [5] voxels evicted so far.  A block comes from the free stack first.  Pops happen only in k_odom_model_insert and pushes
// only in k_odom_evict, never in one launch, so the stack's entries below the counter do not change while blocks are popped: a
// compare-and-swap that only ever lowers the counter hands each entry to one wave, and never goes below zero.
__device__ inline int odom_alloc_block(int* next, int cap_blocks, vox_u64* counters, const int* free_stack) {
  vox_u64 n = __atomic_load_n(&counters[4], __ATOMIC_RELAXED);
  while (n > 0) {
    const vox_u64 seen = atomicCAS(&counters[4], n, n - 1);
    if (seen == n) {
      const int r = free_stack[n - 1];
      next[r] = -1;
      return r;
    }
    n = seen;
  }
  const vox_u64 b = atomicAdd(&counters[0], 1ULL);
  if (b >= vox_u64(cap_blocks)) {
    atomicMax(&counters[3], 1ULL);
    return -1;
  }
  next[b] = -1;
  return int(b);
}

// one wave per group: candidates order[g0 .. g1) (indices into pts / covs, ascending) all lie in the voxel `keys[group]`
__global__ __launch_bounds__(kOdomWave) void k_odom_model_insert(const double* pts, const double* covs, const int* order, const int* group_begin, const vox_u64* group_key, int groups,
                                                                 double thresh_sq, OdomVoxel* table, unsigned mask, OdomBlock* blocks, int* next, int cap_blocks, vox_u64* counters,
                                                                 const int* free_stack, int lru_count) {
  const int g = blockIdx.x, lane = threadIdx.x;
  if (g >= groups) return;
  const vox_u64 key = group_key[g];
  __shared__ int s_slot, s_ok;
  if (lane == 0) {  // groups have distinct keys: no other wave claims or touches this voxel
    // A NEW voxel takes its first block BEFORE it claims a slot: a voxel in the table always owns a block (so the table, of
    // >= 2 x max_blocks slots, stays at most half full), and a dry pool leaves no trace but the full flag.
    unsigned h = unsigned(vox_mix(key)) & mask;
    int ok = 0, fresh = -1;
    for (unsigned probes = 0; probes <= mask; probes++) {
      vox_u64 old = __atomic_load_n(&table[h].key, __ATOMIC_RELAXED);
      if (old == 0) {
        if (fresh < 0) {
          fresh = odom_alloc_block(next, cap_blocks, counters, free_stack);
          if (fresh < 0) break;  // (the full flag is set)
        }
        old = atomicCAS(&table[h].key, 0ULL, key);
        if (old == 0) {
          table[h].head = table[h].tail = fresh, table[h].count = 0;
          atomicAdd(&counters[1], 1ULL);
          ok = 1;
          break;
        }
      }
      if (old == key) {
        ok = 1;
        break;
      }
      h = (h + 1) & mask;
    }
    if (!ok) atomicMax(&counters[3], 1ULL);  // no block, or (never, by the sizing above) no slot: reported, not dropped silently
    else table[h].last_lru_count = lru_count;  // ivox.cpp:164 runs before LinearContainer::insert: a voxel whose candidates are all refused is stamped too
    s_slot = int(h), s_ok = ok;
  }
  __syncthreads();
  if (!s_ok) return;
  OdomVoxel* const vox = &table[s_slot];
  const int head = vox->head;
  int tail = vox->tail, count = vox->count;
  int added = 0;
  for (int c = group_begin[g]; c < group_begin[g + 1]; c++) {
    const int idx = order[c];
    const double x = pts[3 * idx], y = pts[3 * idx + 1], z = pts[3 * idx + 2];
    bool close = false;
    int b = head;
    for (int base = 0; base < count; base += kOdomBlockPoints, b = next[b]) {
      if (base + lane < count) {
        const double dx = blocks[b].p[0][lane] - x, dy = blocks[b].p[1][lane] - y, dz = blocks[b].p[2][lane] - z;
        close = close || ((dx * dx + dy * dy) + dz * dz <= thresh_sq);  // enters iff the smallest distance is > thresh
      }
    }
    if (__any(close)) continue;
    const int pos = count % kOdomBlockPoints;
    if (count > 0 && pos == 0) {  // the tail block is full: chain a fresh one
      if (lane == 0) {
        s_slot = odom_alloc_block(next, cap_blocks, counters, free_stack);
        if (s_slot >= 0) next[tail] = s_slot;
      }
      __syncthreads();
      const int fresh = s_slot;
      __syncthreads();
      if (fresh < 0) break;
      tail = fresh;
    }
    if (lane < 3) blocks[tail].p[lane][pos] = lane == 0 ? x : lane == 1 ? y : z;
    else if (lane < 9) blocks[tail].c[lane - 3][pos] = covs[6LL * idx + (lane - 3)];
    count++, added++;
    __syncthreads();  // the stored point (and the chain link) are visible to every lane of this wave before the next candidate is tested
  }
  if (lane == 0) {
    vox->tail = tail, vox->count = count;
    if (added) atomicAdd(&counters[2], vox_u64(added));
  }
}

// The LRU pass: one thread per slot of `old`.  `fresh` is zeroed, of the same size, and becomes the table.  A voxel stays iff
// last_lru_count >= horizon (ivox.cpp:172: strictly below the horizon leaves).
constexpr int kOdomEvictThreads = 256;
__global__ __launch_bounds__(kOdomEvictThreads) void k_odom_evict(const OdomVoxel* old, OdomVoxel* fresh, unsigned mask, const int* next, int cap_blocks, int* free_stack, vox_u64* counters,
                                                                  int horizon) {
  const unsigned slot = blockIdx.x * unsigned(kOdomEvictThreads) + threadIdx.x;
  if (slot > mask) return;
  const OdomVoxel v = old[slot];
  if (v.key == 0) return;
  if (v.last_lru_count < horizon) {
    // a chain holds max(1, ceil(count / 64)) blocks (a block is chained only for a point that enters it); the bounds keep a corrupted
    // chain from walking off the pool or overfilling the stack
    const int chain = v.count > 0 ? (v.count + kOdomBlockPoints - 1) / kOdomBlockPoints : 1;
    int b = v.head;
    for (int i = 0; i < chain && b >= 0 && b < cap_blocks; i++) {
      const int after = next[b];
      const vox_u64 at = atomicAdd(&counters[4], 1ULL);
      if (at < vox_u64(cap_blocks)) free_stack[at] = b;
      b = after;
    }
    atomicAdd(&counters[1], ~0ULL);  // minus one
    atomicAdd(&counters[5], 1ULL);
    if (v.count > 0) atomicAdd(&counters[2], 0ULL - vox_u64(v.count));
    return;
  }
  unsigned h = unsigned(vox_mix(v.key)) & mask;
  for (unsigned probes = 0; probes <= mask; probes++) {  // (keys are distinct and there are as many slots as in `old`: a slot is found)
    if (atomicCAS(&fresh[h].key, 0ULL, v.key) == 0) {
      fresh[h].head = v.head, fresh[h].tail = v.tail, fresh[h].count = v.count, fresh[h].last_lru_count = v.last_lru_count;
      return;
    }
    h = (h + 1) & mask;
  }
}

// ---- CT-GICP ------------------------------------------------------------------------------------------------------------------------
struct OdomModel {
  const OdomVoxel* table;
  unsigned mask;
  const OdomBlock* blocks;
  const int* next;
  double res;
};

// iVox::nearest_neighbor_search: the 7 voxels in the reference's order, `if (dist > min_dist) continue` (a tie goes to the later one).
// Touch: every voxel found is stamped with lru_count (:223), whether or not it holds the nearest point -- lanes that find the same
// voxel store the same value, so plain stores do; without Touch nothing is stored and the table is only read.
template <bool Touch>
__device__ inline bool odom_nearest(const OdomModel& m, int lru_count, double x, double y, double z, int* blk, int* pos, double* dist) {
  const double cx = floor(x / m.res), cy = floor(y / m.res), cz = floor(z / m.res);
  const double L = double(kVoxAxisLimit);
  const int off[7][3] = {{0, 0, 0}, {1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
  double best = 1.7976931348623157e308;
  bool found = false;
  if (!(cx >= -L - 1 && cx <= L && cy >= -L - 1 && cy <= L && cz >= -L - 1 && cz <= L)) return false;  // (also a non-finite point)
  for (int o = 0; o < 7; o++) {
    const double fx = cx + off[o][0], fy = cy + off[o][1], fz = cz + off[o][2];
    if (!(fx >= -L && fx < L && fy >= -L && fy < L && fz >= -L && fz < L)) continue;  // no voxel there: the model refuses such keys
    const vox_u64 key = (vox_u64((long long)fx + kVoxAxisLimit) | (vox_u64((long long)fy + kVoxAxisLimit) << 21) | (vox_u64((long long)fz + kVoxAxisLimit) << 42)) + 1ULL;
    const int h = odom_find(m.table, m.mask, key);
    if (h < 0) continue;
    if constexpr (Touch) const_cast<OdomVoxel*>(m.table)[h].last_lru_count = lru_count;
    const int count = m.table[h].count;
    int b = m.table[h].head;
    for (int base = 0; base < count; base += kOdomBlockPoints, b = m.next[b]) {
      const int cnt = count - base < kOdomBlockPoints ? count - base : kOdomBlockPoints;
      for (int l = 0; l < cnt; l++) {
        const double dx = x - m.blocks[b].p[0][l], dy = y - m.blocks[b].p[1][l], dz = z - m.blocks[b].p[2][l];
        const double d = (dx * dx + dy * dy) + dz * dz;
        if (d > best) continue;
        best = d, *blk = b, *pos = l, found = true;
      }
    }
  }
  *dist = best;
  return found;
}

__device__ inline double odom_wave_sum(double v) {  // a fixed tree: the same bits every run
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, kOdomWave);
  return v;
}

// q = R p + t, e = q - target
__device__ inline void odom_residual(const double* P /* R t */, const double* p, const double* target, double* e) {
  for (int r = 0; r < 3; r++) e[r] = (((P[3 * r] * p[0] + P[3 * r + 1] * p[1]) + P[3 * r + 2] * p[2]) + P[9 + r]) - target[r];
}
__device__ inline double odom_point_error(const double* Mh /* 3 x 3 */, const double* e, double* me) {
  for (int r = 0; r < 3; r++) me[r] = (Mh[3 * r] * e[0] + Mh[3 * r + 1] * e[1]) + Mh[3 * r + 2] * e[2];
  return 0.5 * ((e[0] * me[0] + e[1] * me[1]) + e[2] * me[2]);
}

// per source point: found[i], target[i] (3), mahal[i] (9, row-major) are stored for k_odom_error; partials[wave][kOdomSums]
template <bool Touch>
__global__ __launch_bounds__(kOdomWave) void k_odom_linearize(const double* pts, const double* covs, const int* time_index, int M, const double* poses /* K x kOdomPoseDoubles */, OdomModel model,
                                                              double max_dist_sq, int* found, double* target, double* mahal, double* partials, int lru_count) {
  const int lane = threadIdx.x, i = blockIdx.x * kOdomWave + lane;
  double H0[3][6], H1[3][6], Mh[9], e[3], me[3], err = 0.0, cnt = 0.0;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 6; c++) H0[r][c] = H1[r][c] = 0.0;
  for (int r = 0; r < 9; r++) Mh[r] = 0.0;
  e[0] = e[1] = e[2] = me[0] = me[1] = me[2] = 0.0;
  if (i < M) {
    const double* P = poses + (long long)time_index[i] * kOdomPoseDoubles;
    const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    const double zero[3] = {0.0, 0.0, 0.0};
    double q[3];
    odom_residual(P, p, zero, q);
    int blk = 0, pos = 0;
    double dist = 0.0;
    const bool ok = odom_nearest<Touch>(model, lru_count, q[0], q[1], q[2], &blk, &pos, &dist) && !(dist > max_dist_sq);
    double tg[3] = {0.0, 0.0, 0.0};
    if (ok) {
      const OdomBlock& B = model.blocks[blk];
      tg[0] = B.p[0][pos], tg[1] = B.p[1][pos], tg[2] = B.p[2][pos];
      const double* ca = covs + 6LL * i;
      const double CA[3][3] = {{ca[0], ca[1], ca[2]}, {ca[1], ca[3], ca[4]}, {ca[2], ca[4], ca[5]}};
      const double CB[3][3] = {{B.c[0][pos], B.c[1][pos], B.c[2][pos]}, {B.c[1][pos], B.c[3][pos], B.c[4][pos]}, {B.c[2][pos], B.c[4][pos], B.c[5][pos]}};
      double RC[3][3], S[3][3];
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) RC[r][c] = (P[3 * r] * CA[0][c] + P[3 * r + 1] * CA[1][c]) + P[3 * r + 2] * CA[2][c];
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) S[r][c] = CB[r][c] + ((RC[r][0] * P[3 * c] + RC[r][1] * P[3 * c + 1]) + RC[r][2] * P[3 * c + 2]);
      // the inverse by cofactors
      const double k00 = S[1][1] * S[2][2] - S[1][2] * S[2][1], k01 = S[1][0] * S[2][2] - S[1][2] * S[2][0], k02 = S[1][0] * S[2][1] - S[1][1] * S[2][0];
      const double det = (S[0][0] * k00 - S[0][1] * k01) + S[0][2] * k02;
      Mh[0] = k00 / det, Mh[1] = (S[0][2] * S[2][1] - S[0][1] * S[2][2]) / det, Mh[2] = (S[0][1] * S[1][2] - S[0][2] * S[1][1]) / det;
      Mh[3] = (S[1][2] * S[2][0] - S[1][0] * S[2][2]) / det, Mh[4] = (S[0][0] * S[2][2] - S[0][2] * S[2][0]) / det, Mh[5] = (S[0][2] * S[1][0] - S[0][0] * S[1][2]) / det;
      Mh[6] = k02 / det, Mh[7] = (S[0][1] * S[2][0] - S[0][0] * S[2][1]) / det, Mh[8] = (S[0][0] * S[1][1] - S[0][1] * S[1][0]) / det;
      odom_residual(P, p, tg, e);
      err = odom_point_error(Mh, e, me);
      cnt = 1.0;
      // d(R p + t) / d pose = [R (-hat p), R], then the chain through the pose of this time index
      double A[3][6];
      for (int r = 0; r < 3; r++) {
        A[r][0] = P[3 * r + 2] * p[1] - P[3 * r + 1] * p[2];
        A[r][1] = P[3 * r] * p[2] - P[3 * r + 2] * p[0];
        A[r][2] = P[3 * r + 1] * p[0] - P[3 * r] * p[1];
        A[r][3] = P[3 * r], A[r][4] = P[3 * r + 1], A[r][5] = P[3 * r + 2];
      }
      const double* D0 = P + 12;
      const double* D1 = P + 48;
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 6; c++) {
          double s0 = A[r][0] * D0[c], s1 = A[r][0] * D1[c];
          for (int j = 1; j < 6; j++) s0 += A[r][j] * D0[6 * j + c], s1 += A[r][j] * D1[6 * j + c];
          H0[r][c] = s0, H1[r][c] = s1;
        }
    }
    found[i] = ok ? 1 : 0;
    for (int r = 0; r < 3; r++) target[3LL * i + r] = tg[r];
    for (int r = 0; r < 9; r++) mahal[9LL * i + r] = Mh[r];
  }
  // this point's terms, reduced over the wave one entry at a time (an unmatched or absent lane adds zeros)
  double* out = partials + (long long)blockIdx.x * kOdomSums;
  double HM0[6][3], HM1[6][3];
  for (int a = 0; a < 6; a++)
    for (int c = 0; c < 3; c++) {
      HM0[a][c] = (H0[0][a] * Mh[c] + H0[1][a] * Mh[3 + c]) + H0[2][a] * Mh[6 + c];
      HM1[a][c] = (H1[0][a] * Mh[c] + H1[1][a] * Mh[3 + c]) + H1[2][a] * Mh[6 + c];
    }
  for (int a = 0; a < 6; a++)
    for (int b = 0; b < 6; b++) {
      const double h00 = odom_wave_sum((HM0[a][0] * H0[0][b] + HM0[a][1] * H0[1][b]) + HM0[a][2] * H0[2][b]);
      const double h01 = odom_wave_sum((HM0[a][0] * H1[0][b] + HM0[a][1] * H1[1][b]) + HM0[a][2] * H1[2][b]);
      const double h11 = odom_wave_sum((HM1[a][0] * H1[0][b] + HM1[a][1] * H1[1][b]) + HM1[a][2] * H1[2][b]);
      if (lane == 0) out[6 * a + b] = h00, out[36 + 6 * a + b] = h01, out[72 + 6 * a + b] = h11;
    }
  for (int a = 0; a < 6; a++) {
    const double b0 = odom_wave_sum((H0[0][a] * me[0] + H0[1][a] * me[1]) + H0[2][a] * me[2]);
    const double b1 = odom_wave_sum((H1[0][a] * me[0] + H1[1][a] * me[1]) + H1[2][a] * me[2]);
    if (lane == 0) out[108 + a] = b0, out[114 + a] = b1;
  }
  err = odom_wave_sum(err), cnt = odom_wave_sum(cnt);
  if (lane == 0) out[120] = err, out[121] = cnt;
}

// partials[wave][2]: the error and the count of matched points, from the stored correspondences
__global__ __launch_bounds__(kOdomWave) void k_odom_error(const double* pts, const int* time_index, int M, const double* poses /* K x 12 */, const int* found, const double* target,
                                                          const double* mahal, double* partials) {
  const int lane = threadIdx.x, i = blockIdx.x * kOdomWave + lane;
  double err = 0.0, cnt = 0.0;
  if (i < M && found[i]) {
    const double* P = poses + (long long)time_index[i] * 12;
    const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    double e[3], me[3];
    odom_residual(P, p, target + 3LL * i, e);
    err = odom_point_error(mahal + 9LL * i, e, me);
    cnt = 1.0;
  }
  err = odom_wave_sum(err), cnt = odom_wave_sum(cnt);
  if (lane == 0) partials[2LL * blockIdx.x] = err, partials[2LL * blockIdx.x + 1] = cnt;
}

__global__ __launch_bounds__(128) void k_odom_sum(const double* partials, int waves, int nvals, double* out) {
  const int v = threadIdx.x;
  if (v >= nvals) return;
  double s = 0.0;
  for (int w = 0; w < waves; w++) s += partials[(long long)w * nvals + v];
  out[v] = s;
}

// ---- deskew -------------------------------------------------------------------------------------------------------------------------
struct OdomDeskew {
  double R0[9], t0[3];  // T_begin
  double w[3];          // Logmap(R_begin^T R_end)
  double dt[3];         // t_end - t_begin
  double scale, shift;  // time of a point [s] = raw value * scale + shift; without a time field: (scale * index) / n
  double max_time;      // <= 0: every point at t = 0
  int ot;               // byte offset of the time field
};

// Pose3::interpolateRt(T_end, t) of T_begin: the rotation R_begin Expmap(t Logmap(R_begin^T R_end)), the translation interpolated
// linearly; then the point.  A non-finite coordinate stays non-finite (the integrator's check pass counts and skips it).
template <int XyzType, int IntType, int TimeType /* 0: no time field */>
__global__ __launch_bounds__(kVoxThreads) void k_odom_deskew(VoxCloud2 c, OdomDeskew d, double4* pts, double* inten) {
  const long long stride = (long long)gridDim.x * kVoxThreads;
  for (long long i = (long long)blockIdx.x * kVoxThreads + threadIdx.x; i < c.n; i += stride) {
    const unsigned char* rec = c.raw + i * c.step;
    const double x = vox_field<XyzType>(rec + c.ox), y = vox_field<XyzType>(rec + c.oy), z = vox_field<XyzType>(rec + c.oz);
    double time;
    if constexpr (TimeType == 0) time = (d.scale * double(i)) / double(c.n);
    else time = vox_field<TimeType>(rec + d.ot) * d.scale + d.shift;
    const double t = d.max_time > 0.0 ? time / d.max_time : 0.0;
    const double ax = t * d.w[0], ay = t * d.w[1], az = t * d.w[2];
    const double th2 = (ax * ax + ay * ay) + az * az;
    double E[9];
    if (th2 <= 2.220446049250313e-16) {  // SO3::Expmap near zero: I + hat(a)
      E[0] = 1.0, E[1] = -az, E[2] = ay, E[3] = az, E[4] = 1.0, E[5] = -ax, E[6] = -ay, E[7] = ax, E[8] = 1.0;
    } else {
      const double th = sqrt(th2), A = sin(th) / th, B = (1.0 - cos(th)) / th2;
      E[0] = 1.0 - B * (ay * ay + az * az), E[1] = B * (ax * ay) - A * az, E[2] = B * (ax * az) + A * ay;
      E[3] = B * (ax * ay) + A * az, E[4] = 1.0 - B * (ax * ax + az * az), E[5] = B * (ay * az) - A * ax;
      E[6] = B * (ax * az) - A * ay, E[7] = B * (ay * az) + A * ax, E[8] = 1.0 - B * (ax * ax + ay * ay);
    }
    double R[9];
    for (int r = 0; r < 3; r++)
      for (int k = 0; k < 3; k++) R[3 * r + k] = (d.R0[3 * r] * E[k] + d.R0[3 * r + 1] * E[3 + k]) + d.R0[3 * r + 2] * E[6 + k];
    const double px = ((R[0] * x + R[1] * y) + R[2] * z) + (d.t0[0] + t * d.dt[0]);
    const double py = ((R[3] * x + R[4] * y) + R[5] * z) + (d.t0[1] + t * d.dt[1]);
    const double pz = ((R[6] * x + R[7] * y) + R[8] * z) + (d.t0[2] + t * d.dt[2]);
    pts[i] = make_double4(px, py, pz, 0.0);
    inten[i] = vox_field<IntType>(rec + c.oi);
  }
}

}  // namespace nidreg
