// nidreg_odom.hip -- C ABI of the scan-to-model odometry (include/nidreg.h: nidreg_odom_*): the device side of
// vlcal::DynamicPointCloudIntegrator (kernels: nid_odom_kernels.hpp).  The handle owns the model -- the voxel table and the pool of
// point blocks -- and the current scan's sampled points with their correspondences; the optimiser itself runs on the host
// (direct_visual_lidar_calibration_amd/odometry.py) over the 12 x 12 system the linearisation returns.
#include "nid_odom_kernels.hpp"
#include "nid_device.hpp"
#include "nid_launch.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

struct nidreg_odom {
  int device = 0;
  double res = 1.0, thresh_sq = 0.0;
  int max_blocks = 0;      // the pool never grows past this
  int cap_blocks = 0;      // blocks allocated now
  int64_t table_cap = 0;   // slots, a power of two >= 2 x max_blocks (a voxel owns at least one block)
  int64_t blocks = 0, voxels = 0, points = 0;  // blocks: handed out by the bump counter, the free ones included (what the pool must hold)
  nidreg::DeviceBuf d_table, d_blocks, d_next, d_counters;
  // the LRU eviction (nidreg_odom_set_lru; lru_thresh = 0: off, and neither buffer below exists)
  int32_t lru_thresh = 0, lru_cycle = 10, lru_count = 0;
  int64_t free_blocks = 0, evicted = 0, passes = 0;
  nidreg::DeviceBuf d_spare, d_free;  // the table the next pass fills; the stack of free block ids (max_blocks entries)
  // the current scan (nidreg_odom_set_source)
  int m = 0, max_time_index = -1, src_cap = 0;
  bool linearized = false;
  nidreg::DeviceBuf d_pts, d_covs, d_tidx, d_found, d_target, d_mahal, d_partials, d_poses, d_out;
  int poses_cap = 0;
};

namespace nidreg {
namespace {

constexpr int kInitialBlocks = 1024;
constexpr int kCounters = 6;  // nid_odom_kernels.hpp: odom_alloc_block

unsigned waves_of(int n) { return unsigned(std::max(1, (n + kOdomWave - 1) / kOdomWave)); }

// room for `need` blocks: a larger pool with the blocks in use copied over
int pool_reserve(nidreg_odom* h, int64_t need) {
  need = std::min<int64_t>(need, h->max_blocks);
  if (need <= h->cap_blocks) return NIDREG_OK;
  const int cap = int(std::min<int64_t>(std::max<int64_t>(need, 2LL * h->cap_blocks), h->max_blocks));
  DeviceBuf blocks, next;
  HIP_TRY(blocks.alloc(size_t(cap) * sizeof(OdomBlock)));
  HIP_TRY(next.alloc(size_t(cap) * sizeof(int)));
  if (h->blocks > 0) {
    HIP_TRY(hipMemcpy(blocks.as<void>(), h->d_blocks.as<void>(), size_t(h->blocks) * sizeof(OdomBlock), hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(next.as<void>(), h->d_next.as<void>(), size_t(h->blocks) * sizeof(int), hipMemcpyDeviceToDevice));
  }
  HIP_TRY(hipStreamSynchronize(nullptr));
  h->d_blocks = std::move(blocks);
  h->d_next = std::move(next);
  h->cap_blocks = cap;
  return NIDREG_OK;
}

int check_points(const char* who, const double* points, int32_t m) {
  if (m < 0 || (m > 0 && !points)) return fail(NIDREG_ERR_INVALID, std::string(who) + ": negative point count or null points");
  return NIDREG_OK;
}

int covariances(const char* who, nidreg_odom* h, const double* points, int32_t m, int32_t k, const int32_t* neighbors_in, int32_t* neighbors_out, double* normals, double* covs) {
  if (!h) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null handle");
  if (const int rc = check_points(who, points, m)) return rc;
  if (k < 2 || k > kOdomMaxK) return fail(NIDREG_ERR_INVALID, std::string(who) + ": k must lie in 2.." + std::to_string(kOdomMaxK));
  if (m < k) return fail(NIDREG_ERR_INVALID, std::string(who) + ": fewer points (" + std::to_string(m) + ") than neighbours per point (" + std::to_string(k) + ")");
  if (!covs) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null covs");
  const size_t nk = size_t(m) * size_t(k);
  if (neighbors_in)
    for (size_t j = 0; j < nk; j++)
      if (neighbors_in[j] < 0 || neighbors_in[j] >= m) return fail(NIDREG_ERR_INVALID, std::string(who) + ": a neighbour index outside [0, m)");
  HIP_TRY(hipSetDevice(h->device));
  DeviceBuf d_pts, d_nbr, d_normals, d_covs;
  HIP_TRY(d_pts.alloc(size_t(m) * 24));
  HIP_TRY(d_nbr.alloc(nk * sizeof(int)));
  HIP_TRY(d_normals.alloc(size_t(m) * 24));
  HIP_TRY(d_covs.alloc(size_t(m) * 48));
  HIP_TRY(hipMemcpy(d_pts.as<void>(), points, size_t(m) * 24, hipMemcpyHostToDevice));
  if (neighbors_in) {
    HIP_TRY(hipMemcpy(d_nbr.as<void>(), neighbors_in, nk * sizeof(int), hipMemcpyHostToDevice));
  } else {
    HIP_TRY(launch(k_odom_knn, waves_of(m), kOdomWave, 0, nullptr, d_pts.as<const double>(), m, k, d_nbr.as<int>()));
  }
  HIP_TRY(launch(k_odom_cov, waves_of(m), kOdomWave, 0, nullptr, d_pts.as<const double>(), d_nbr.as<const int>(), m, k, d_normals.as<double>(), d_covs.as<double>()));
  if (neighbors_out) HIP_TRY(hipMemcpy(neighbors_out, d_nbr.as<void>(), nk * sizeof(int), hipMemcpyDeviceToHost));
  if (normals) HIP_TRY(hipMemcpy(normals, d_normals.as<void>(), size_t(m) * 24, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(covs, d_covs.as<void>(), size_t(m) * 48, hipMemcpyDeviceToHost));
  return NIDREG_OK;
}

OdomModel model_of(const nidreg_odom* h) {
  return OdomModel{h->d_table.as<const OdomVoxel>(), unsigned(h->table_cap - 1), h->d_blocks.as<const OdomBlock>(), h->d_next.as<const int>(), h->res};
}

int upload_poses(nidreg_odom* h, const char* who, const double* poses, int32_t num_poses, int doubles) {
  if (!h) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null handle");
  if (!poses || num_poses < 1) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null poses or an empty time table");
  if (h->max_time_index >= num_poses) return fail(NIDREG_ERR_INVALID, std::string(who) + ": the source has time index " + std::to_string(h->max_time_index) + ", the table " + std::to_string(num_poses) + " entries");
  HIP_TRY(hipSetDevice(h->device));
  if (h->poses_cap < num_poses) {
    HIP_TRY(h->d_poses.alloc(size_t(num_poses) * kOdomPoseDoubles * 8));
    h->poses_cap = num_poses;
  }
  HIP_TRY(hipMemcpy(h->d_poses.as<void>(), poses, size_t(num_poses) * size_t(doubles) * 8, hipMemcpyHostToDevice));
  return NIDREG_OK;
}

// the deskew kernel for the record's field types, all validated by the caller (time_datatype 0: no time field)
hipError_t deskew_launch(int32_t xyz_datatype, int32_t intensity_datatype, int32_t time_datatype, const VoxCloud2& c, const OdomDeskew& d, double4* pts, double* inten) {
  hipError_t e = hipErrorInvalidValue;
  with_int<kPcFloat32, kPcFloat64>(xyz_datatype, [&](auto X) {
    with_field_type(intensity_datatype, [&](auto I) {
      with_int<kPcUint32, kPcFloat32, kPcFloat64, 0>(time_datatype, [&](auto T) { e = launch(k_odom_deskew<X, I, T>, vox_grid(c.n), kVoxThreads, 0, nullptr, c, d, pts, inten); });
    });
  });
  return e;
}

}  // namespace
}  // namespace nidreg

using namespace nidreg;

extern "C" {

int nidreg_odom_create(int device_id, double voxel_resolution, double insertion_dist_thresh, int32_t max_blocks, nidreg_odom** out) {
  const char* const who = "nidreg_odom_create";
  if (!out) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null out");
  *out = nullptr;
  if (!(voxel_resolution > 0.0) || !std::isfinite(voxel_resolution)) return fail(NIDREG_ERR_INVALID, std::string(who) + ": voxel_resolution must be positive and finite");
  if (!(insertion_dist_thresh >= 0.0) || !std::isfinite(insertion_dist_thresh)) return fail(NIDREG_ERR_INVALID, std::string(who) + ": insertion_dist_thresh must be finite and >= 0");
  if (max_blocks < 1 || max_blocks > (1 << 24)) return fail(NIDREG_ERR_INVALID, std::string(who) + ": max_blocks must lie in 1..2^24");
  if (device_id < 0) return fail(NIDREG_ERR_INVALID, std::string(who) + ": device_id out of range");
  if (const int rc = use_device(who, device_id)) return rc;
  std::unique_ptr<nidreg_odom> h(new nidreg_odom());
  h->device = device_id;
  h->res = voxel_resolution;
  h->thresh_sq = insertion_dist_thresh * insertion_dist_thresh;
  h->max_blocks = max_blocks;
  h->table_cap = 1024;
  while (h->table_cap < 2LL * max_blocks) h->table_cap <<= 1;
  HIP_TRY(h->d_table.alloc(size_t(h->table_cap) * sizeof(OdomVoxel)));
  HIP_TRY(h->d_counters.alloc(kCounters * sizeof(vox_u64)));
  HIP_TRY(h->d_out.alloc(kOdomSums * 8));
  HIP_TRY(hipMemsetAsync(h->d_table.as<void>(), 0, size_t(h->table_cap) * sizeof(OdomVoxel), nullptr));
  HIP_TRY(hipMemsetAsync(h->d_counters.as<void>(), 0, kCounters * sizeof(vox_u64), nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  if (const int rc = pool_reserve(h.get(), kInitialBlocks)) return rc;
  *out = h.release();
  return NIDREG_OK;
}

void nidreg_odom_destroy(nidreg_odom* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(nullptr);
  delete h;
}

int nidreg_odom_knn_covariances(nidreg_odom* h, const double* points, int32_t m, int32_t k, int32_t* neighbors, double* normals, double* covs) {
  return covariances("nidreg_odom_knn_covariances", h, points, m, k, nullptr, neighbors, normals, covs);
}

int nidreg_odom_covariances(nidreg_odom* h, const double* points, int32_t m, int32_t k, const int32_t* neighbors, double* normals, double* covs) {
  if (!neighbors) return fail(NIDREG_ERR_INVALID, "nidreg_odom_covariances: null neighbors");
  return covariances("nidreg_odom_covariances", h, points, m, k, neighbors, nullptr, normals, covs);
}

int nidreg_odom_model_insert(nidreg_odom* h, const double* points, const double* covs, int32_t m) {
  const char* const who = "nidreg_odom_model_insert";
  if (!h) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null handle");
  if (const int rc = check_points(who, points, m)) return rc;
  if (m > 0 && !covs) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null covs");
  if (m == 0) return NIDREG_OK;
  // the scan's points grouped by voxel, ascending index inside a group (host work over ~10^4 points; the walk is the device's)
  std::vector<vox_u64> keys(static_cast<size_t>(m), 0ULL);
  for (int32_t i = 0; i < m; i++)
    if (!odom_key(points[3 * i], points[3 * i + 1], points[3 * i + 2], h->res, keys[size_t(i)]))
      return fail(NIDREG_ERR_INVALID, std::string(who) + ": point " + std::to_string(i) + " is not finite or lies outside the packed-key limit (the voxel index floor(coordinate / " +
                                        "voxel_resolution) must lie in [-1048576, 1048576) on every axis); nothing was inserted");
  std::vector<int> order(static_cast<size_t>(m), 0);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return keys[size_t(a)] < keys[size_t(b)]; });
  std::vector<int> gbegin;
  std::vector<vox_u64> gkey;
  for (int32_t c = 0; c < m; c++)
    if (c == 0 || keys[size_t(order[size_t(c)])] != gkey.back()) gbegin.push_back(c), gkey.push_back(keys[size_t(order[size_t(c)])]);
  const int groups = int(gkey.size());
  gbegin.push_back(m);
  HIP_TRY(hipSetDevice(h->device));
  // an upper bound of the blocks this call takes, less the free ones it pops first: a handle that recycles does not grow its pool for them
  if (const int rc = pool_reserve(h, h->blocks + std::max<int64_t>(0, int64_t(groups) + m / kOdomBlockPoints - h->free_blocks))) return rc;
  h->lru_count++;  // ivox.cpp:144
  DeviceBuf d_pts, d_covs, d_order, d_gbegin, d_gkey;
  HIP_TRY(d_pts.alloc(size_t(m) * 24));
  HIP_TRY(d_covs.alloc(size_t(m) * 48));
  HIP_TRY(d_order.alloc(size_t(m) * sizeof(int)));
  HIP_TRY(d_gbegin.alloc(size_t(groups + 1) * sizeof(int)));
  HIP_TRY(d_gkey.alloc(size_t(groups) * sizeof(vox_u64)));
  HIP_TRY(hipMemcpy(d_pts.as<void>(), points, size_t(m) * 24, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_covs.as<void>(), covs, size_t(m) * 48, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_order.as<void>(), order.data(), size_t(m) * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_gbegin.as<void>(), gbegin.data(), size_t(groups + 1) * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_gkey.as<void>(), gkey.data(), size_t(groups) * sizeof(vox_u64), hipMemcpyHostToDevice));
  HIP_TRY(launch(k_odom_model_insert, unsigned(groups), kOdomWave, 0, nullptr, d_pts.as<const double>(), d_covs.as<const double>(), d_order.as<const int>(), d_gbegin.as<const int>(),
                 d_gkey.as<const vox_u64>(), groups, h->thresh_sq, h->d_table.as<OdomVoxel>(), unsigned(h->table_cap - 1), h->d_blocks.as<OdomBlock>(), h->d_next.as<int>(), h->cap_blocks,
                 h->d_counters.as<vox_u64>(), h->d_free.as<const int>(), h->lru_count));
  // ivox.cpp:169-178: the horizon must be positive, and only every lru_cycle-th insert looks
  const int64_t horizon = int64_t(h->lru_count) - h->lru_thresh;
  const bool evict = h->lru_thresh > 0 && horizon > 0 && h->lru_count % h->lru_cycle == 0;
  if (evict) {
    HIP_TRY(hipMemsetAsync(h->d_spare.as<void>(), 0, size_t(h->table_cap) * sizeof(OdomVoxel), nullptr));
    HIP_TRY(launch(k_odom_evict, blocks_for(h->table_cap, kOdomEvictThreads), kOdomEvictThreads, 0, nullptr, h->d_table.as<const OdomVoxel>(), h->d_spare.as<OdomVoxel>(),
                   unsigned(h->table_cap - 1), h->d_next.as<const int>(), h->cap_blocks, h->d_free.as<int>(), h->d_counters.as<vox_u64>(), int(horizon)));
  }
  vox_u64 cnt[kCounters];
  HIP_TRY(hipMemcpy(cnt, h->d_counters.as<void>(), sizeof(cnt), hipMemcpyDeviceToHost));
  if (evict) {  // (the copy above waited for the pass)
    std::swap(h->d_table, h->d_spare);
    h->passes++;
  }
  h->blocks = int64_t(std::min<vox_u64>(cnt[0], vox_u64(h->cap_blocks)));
  h->voxels = int64_t(cnt[1]), h->points = int64_t(cnt[2]), h->free_blocks = int64_t(cnt[4]), h->evicted = int64_t(cnt[5]);
  if (cnt[3]) {
    cnt[0] = vox_u64(h->blocks), cnt[3] = 0;
    HIP_TRY(hipMemcpy(h->d_counters.as<void>(), cnt, 4 * sizeof(vox_u64), hipMemcpyHostToDevice));
    return fail(NIDREG_ERR_FULL, std::string(who) + ": the pool of " + std::to_string(h->max_blocks) + " point blocks is exhausted; points of this scan were left out of the model");
  }
  return NIDREG_OK;
}

int nidreg_odom_model_info(nidreg_odom* h, int64_t* info4) {
  if (!h || !info4) return fail(NIDREG_ERR_INVALID, "nidreg_odom_model_info: null argument");
  info4[0] = h->voxels, info4[1] = h->points, info4[2] = h->blocks - h->free_blocks, info4[3] = h->max_blocks;
  return NIDREG_OK;
}

int nidreg_odom_set_lru(nidreg_odom* h, int32_t lru_thresh, int32_t lru_cycle) {
  const char* const who = "nidreg_odom_set_lru";
  if (!h) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null handle");
  if (lru_thresh < 0) return fail(NIDREG_ERR_INVALID, std::string(who) + ": lru_thresh must be >= 0 (0: no eviction)");
  if (lru_cycle < 1) return fail(NIDREG_ERR_INVALID, std::string(who) + ": lru_cycle must be >= 1");
  // a model must not carry stamps from before the rule was set
  if (h->lru_count > 0) return fail(NIDREG_ERR_INVALID, std::string(who) + ": the model has been inserted into; the eviction rule is set before the first nidreg_odom_model_insert");
  if (lru_thresh > 0 && !h->d_spare.as<void>()) {
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->d_spare.alloc(size_t(h->table_cap) * sizeof(OdomVoxel)));
    HIP_TRY(h->d_free.alloc(size_t(h->max_blocks) * sizeof(int)));
  }
  h->lru_thresh = lru_thresh, h->lru_cycle = lru_cycle;
  return NIDREG_OK;
}

int nidreg_odom_lru_info(nidreg_odom* h, int64_t* info4) {
  if (!h || !info4) return fail(NIDREG_ERR_INVALID, "nidreg_odom_lru_info: null argument");
  info4[0] = h->lru_count, info4[1] = h->evicted, info4[2] = h->free_blocks, info4[3] = h->passes;
  return NIDREG_OK;
}

int nidreg_odom_model_get(nidreg_odom* h, int32_t* voxels /* points x 3 */, double* points /* points x 3 */, double* covs /* points x 6, nullable */) {
  const char* const who = "nidreg_odom_model_get";
  if (!h) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null handle");
  if (h->points == 0) return NIDREG_OK;
  if (!voxels || !points) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null voxels or points");
  HIP_TRY(hipSetDevice(h->device));
  std::vector<OdomVoxel> table(static_cast<size_t>(h->table_cap), OdomVoxel{});
  std::vector<int> next(static_cast<size_t>(h->blocks), 0);
  std::unique_ptr<OdomBlock[]> blocks(new OdomBlock[size_t(h->blocks)]);
  HIP_TRY(hipMemcpy(table.data(), h->d_table.as<void>(), table.size() * sizeof(OdomVoxel), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(next.data(), h->d_next.as<void>(), next.size() * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(blocks.get(), h->d_blocks.as<void>(), size_t(h->blocks) * sizeof(OdomBlock), hipMemcpyDeviceToHost));
  std::vector<const OdomVoxel*> used;
  for (const OdomVoxel& v : table)
    if (v.key && v.count > 0) used.push_back(&v);
  std::sort(used.begin(), used.end(), [](const OdomVoxel* a, const OdomVoxel* b) { return a->key < b->key; });
  int64_t j = 0;
  for (const OdomVoxel* v : used) {
    const vox_u64 key = v->key - 1;
    const int32_t vx = int32_t(int64_t(key & 0x1fffff) - kVoxAxisLimit), vy = int32_t(int64_t((key >> 21) & 0x1fffff) - kVoxAxisLimit), vz = int32_t(int64_t((key >> 42) & 0x1fffff) - kVoxAxisLimit);
    int b = v->head;
    for (int i = 0; i < v->count; i++, j++) {
      if (i > 0 && i % kOdomBlockPoints == 0) b = next[size_t(b)];
      if (b < 0 || b >= h->blocks || j >= h->points) return fail(NIDREG_ERR_INVALID, std::string(who) + ": the model's chains are inconsistent");
      const int l = i % kOdomBlockPoints;
      voxels[3 * j] = vx, voxels[3 * j + 1] = vy, voxels[3 * j + 2] = vz;
      for (int r = 0; r < 3; r++) points[3 * j + r] = blocks[size_t(b)].p[r][l];
      if (covs)
        for (int r = 0; r < 6; r++) covs[6 * j + r] = blocks[size_t(b)].c[r][l];
    }
  }
  return NIDREG_OK;
}

int nidreg_odom_set_source(nidreg_odom* h, const double* points, const double* covs, const int32_t* time_index, int32_t m) {
  const char* const who = "nidreg_odom_set_source";
  if (!h) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null handle");
  if (const int rc = check_points(who, points, m)) return rc;
  if (m > 0 && (!covs || !time_index)) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null covs or time_index");
  int max_index = -1;
  for (int32_t i = 0; i < m; i++) {
    if (time_index[i] < 0) return fail(NIDREG_ERR_INVALID, std::string(who) + ": a negative time index");
    max_index = std::max(max_index, time_index[i]);
  }
  HIP_TRY(hipSetDevice(h->device));
  h->m = 0, h->linearized = false;
  if (h->src_cap < m) {
    const size_t n = size_t(m), waves = waves_of(m);
    HIP_TRY(h->d_pts.alloc(n * 24));
    HIP_TRY(h->d_covs.alloc(n * 48));
    HIP_TRY(h->d_tidx.alloc(n * sizeof(int)));
    HIP_TRY(h->d_found.alloc(n * sizeof(int)));
    HIP_TRY(h->d_target.alloc(n * 24));
    HIP_TRY(h->d_mahal.alloc(n * 72));
    HIP_TRY(h->d_partials.alloc(waves * kOdomSums * 8));
    h->src_cap = m;
  }
  if (m > 0) {
    HIP_TRY(hipMemcpy(h->d_pts.as<void>(), points, size_t(m) * 24, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_covs.as<void>(), covs, size_t(m) * 48, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_tidx.as<void>(), time_index, size_t(m) * sizeof(int), hipMemcpyHostToDevice));
  }
  h->m = m, h->max_time_index = max_index;
  return NIDREG_OK;
}

int nidreg_odom_linearize(nidreg_odom* h, const double* poses, int32_t num_poses, double max_correspondence_dist_sq, double* out122) {
  const char* const who = "nidreg_odom_linearize";
  if (const int rc = upload_poses(h, who, poses, num_poses, kOdomPoseDoubles)) return rc;
  if (!out122) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null out");
  std::memset(out122, 0, kOdomSums * 8);
  h->linearized = true;
  if (h->m == 0) return NIDREG_OK;
  const unsigned waves = waves_of(h->m);
  HIP_TRY(with_bool(h->lru_thresh > 0, [&](auto Touch) {  // with the eviction on, the search stamps the voxels it finds; off, it stores nothing
    return launch(k_odom_linearize<Touch>, waves, kOdomWave, 0, nullptr, h->d_pts.as<const double>(), h->d_covs.as<const double>(), h->d_tidx.as<const int>(), h->m,
                  h->d_poses.as<const double>(), model_of(h), max_correspondence_dist_sq, h->d_found.as<int>(), h->d_target.as<double>(), h->d_mahal.as<double>(), h->d_partials.as<double>(),
                  h->lru_count);
  }));
  HIP_TRY(launch(k_odom_sum, 1, 128, 0, nullptr, h->d_partials.as<const double>(), int(waves), kOdomSums, h->d_out.as<double>()));
  HIP_TRY(hipMemcpy(out122, h->d_out.as<void>(), kOdomSums * 8, hipMemcpyDeviceToHost));
  return NIDREG_OK;
}

int nidreg_odom_error(nidreg_odom* h, const double* poses12, int32_t num_poses, double* out2) {
  const char* const who = "nidreg_odom_error";
  if (const int rc = upload_poses(h, who, poses12, num_poses, 12)) return rc;
  if (!out2) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null out");
  if (!h->linearized) return fail(NIDREG_ERR_INVALID, std::string(who) + ": no correspondences yet (nidreg_odom_linearize sets them)");
  out2[0] = out2[1] = 0.0;
  if (h->m == 0) return NIDREG_OK;
  const unsigned waves = waves_of(h->m);
  HIP_TRY(launch(k_odom_error, waves, kOdomWave, 0, nullptr, h->d_pts.as<const double>(), h->d_tidx.as<const int>(), h->m, h->d_poses.as<const double>(), h->d_found.as<const int>(),
                 h->d_target.as<const double>(), h->d_mahal.as<const double>(), h->d_partials.as<double>()));
  HIP_TRY(launch(k_odom_sum, 1, 128, 0, nullptr, h->d_partials.as<const double>(), int(waves), 2, h->d_out.as<double>()));
  HIP_TRY(hipMemcpy(out2, h->d_out.as<void>(), 16, hipMemcpyDeviceToHost));
  return NIDREG_OK;
}

int nidreg_odom_correspondences(nidreg_odom* h, int32_t* found, double* target, double* mahalanobis) {
  const char* const who = "nidreg_odom_correspondences";
  if (!h) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null handle");
  if (!h->linearized) return fail(NIDREG_ERR_INVALID, std::string(who) + ": no correspondences yet (nidreg_odom_linearize sets them)");
  if (h->m == 0) return NIDREG_OK;
  HIP_TRY(hipSetDevice(h->device));
  if (found) HIP_TRY(hipMemcpy(found, h->d_found.as<void>(), size_t(h->m) * sizeof(int), hipMemcpyDeviceToHost));
  if (target) HIP_TRY(hipMemcpy(target, h->d_target.as<void>(), size_t(h->m) * 24, hipMemcpyDeviceToHost));
  if (mahalanobis) HIP_TRY(hipMemcpy(mahalanobis, h->d_mahal.as<void>(), size_t(h->m) * 72, hipMemcpyDeviceToHost));
  return NIDREG_OK;
}

int nidreg_odom_deskew_insert(nidreg_integrator* integrator, const void* data, int64_t num_points, int32_t point_step, int32_t x_offset, int32_t y_offset, int32_t z_offset, int32_t xyz_datatype,
                              int32_t intensity_offset, int32_t intensity_datatype, int32_t time_offset, int32_t time_datatype, double time_scale, double time_shift, double max_time,
                              const double* begin12, const double* rotvec3, const double* dtrans3, int64_t* num_skipped) {
  const char* const who = "nidreg_odom_deskew_insert";
  if (num_skipped) *num_skipped = 0;
  if (!begin12 || !rotvec3 || !dtrans3) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null pose");
  for (int i = 0; i < 12; i++)
    if (!std::isfinite(begin12[i])) return fail(NIDREG_ERR_INVALID, std::string(who) + ": a pose entry is not finite");
  for (int i = 0; i < 3; i++)
    if (!std::isfinite(rotvec3[i]) || !std::isfinite(dtrans3[i])) return fail(NIDREG_ERR_INVALID, std::string(who) + ": a pose entry is not finite");
  if (!std::isfinite(time_scale) || !std::isfinite(time_shift) || std::isnan(max_time)) return fail(NIDREG_ERR_INVALID, std::string(who) + ": the time map is not finite");
  if (time_datatype != 0) {
    if (time_datatype != kPcUint32 && time_datatype != kPcFloat32 && time_datatype != kPcFloat64)
      return fail(NIDREG_ERR_INVALID, std::string(who) + ": the time field must be UINT32, FLOAT32 or FLOAT64 (or 0: no time field), got datatype " + std::to_string(time_datatype));
    const int time_bytes = time_datatype == kPcFloat64 ? 8 : 4;
    if (time_offset < 0 || time_offset > point_step - time_bytes) return fail(NIDREG_ERR_INVALID, std::string(who) + ": the time field lies outside the point_step bytes of a record");
  }
  VoxCloud2 c;
  double4* d_pts = nullptr;
  double* d_int = nullptr;
  if (const int rc = integrator_stage_cloud2(integrator, who, data, num_points, point_step, x_offset, y_offset, z_offset, xyz_datatype, intensity_offset, intensity_datatype, &c, &d_pts, &d_int))
    return rc;
  if (num_points == 0) return NIDREG_OK;
  OdomDeskew d;
  for (int i = 0; i < 9; i++) d.R0[i] = begin12[i];
  for (int i = 0; i < 3; i++) d.t0[i] = begin12[9 + i], d.w[i] = rotvec3[i], d.dt[i] = dtrans3[i];
  d.scale = time_scale, d.shift = time_shift, d.max_time = max_time, d.ot = time_offset;
  HIP_TRY(deskew_launch(xyz_datatype, intensity_datatype, time_datatype, c, d, d_pts, d_int));
  return integrator_insert_staged(integrator, who, num_points, num_skipped);
}

}  // extern "C"
