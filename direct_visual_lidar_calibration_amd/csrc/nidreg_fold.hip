// nidreg_fold.hip -- C ABI of the folds of a device-resident cloud (include/nidreg.h: nidreg_cloud_fold_ids, nidreg_cloud_fold): a
// flag pass (nid_fold_kernels.hpp), then the selection's exclusive scan of per-tile counts and its gather into a new device cloud
// (launch_select_scan / launch_select_scatter, nidreg_select.hip).  Built -ffp-contract=off like every translation unit: the cube
// of a point is floor(p / cell), one division and nothing fused around it.
#include "nidreg_internal.hpp"
#include "nid_fold_kernels.hpp"

namespace {

// what both entry points refuse before anything else is looked at; NULL: acceptable
const char* fold_args_refusal(double cell, int num_folds) {
  if (num_folds < 1 || num_folds > kFoldMax) return "num_folds must lie in [1, 1024]";
  if (!(cell >= 0.0) || std::isinf(cell)) return "cell must be finite and >= 0 (0: per-point folds)";
  return nullptr;
}

}  // namespace

extern "C" {

int nidreg_cloud_fold_ids(const nidreg_cloud* cloud, uint64_t seed, double cell, int num_folds, int32_t* folds_out, int64_t* sizes_out) {
  const char* const who = "nidreg_cloud_fold_ids";
  if (const char* why = fold_args_refusal(cell, num_folds)) return fail(NIDREG_ERR_INVALID, std::string(who) + ": " + why);
  if (!cloud) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null cloud");
  const int64_t n = cloud->n;
  if (!folds_out && n > 0) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null folds_out");
  if (n == 0) {
    if (sizes_out) std::fill(sizes_out, sizes_out + num_folds, int64_t(0));
    return NIDREG_OK;
  }
  HIP_TRY(hipSetDevice(cloud->device));
  const int64_t ntiles = (n + kFoldTile - 1) / kFoldTile;
  const int nblocks = int(std::min<int64_t>(ntiles, kFoldIdBlocks));
  ScratchArena& arena = ScratchArena::of(cloud->device);
  std::lock_guard<ScratchArena> guard(arena);
  const auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
  const size_t b_ids = al(size_t(n) * sizeof(int32_t)), b_count = al(size_t(nblocks) * num_folds * sizeof(int)), b_sizes = al(size_t(num_folds) * sizeof(long long));
  HIP_TRY(arena.reserve(b_ids + b_count + b_sizes + 4096));
  int32_t* const d_ids = static_cast<int32_t*>(arena.carve(b_ids));
  int* const d_count = static_cast<int*>(arena.carve(b_count));
  long long* const d_sizes = static_cast<long long*>(arena.carve(b_sizes));
  if (!d_ids || !d_count || !d_sizes) return fail(NIDREG_ERR_HIP, std::string(who) + ": scratch arena exhausted");
  HIP_TRY(launch(k_fold_ids, unsigned(nblocks), kFoldThreads, 0, nullptr, cloud->d_pts.as<double>(), n, seed, cell, num_folds, d_ids, d_count));
  if (sizes_out) HIP_TRY(launch(k_fold_sizes, blocks_for(num_folds, kFoldThreads), kFoldThreads, 0, nullptr, d_count, nblocks, num_folds, d_sizes));
  HIP_TRY(hipMemcpy(folds_out, d_ids, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost));  // (synchronises the null stream)
  if (sizes_out) {
    static_assert(sizeof(long long) == sizeof(int64_t), "k_fold_sizes writes the caller's int64_t");
    HIP_TRY(hipMemcpy(sizes_out, d_sizes, size_t(num_folds) * sizeof(int64_t), hipMemcpyDeviceToHost));
  }
  return NIDREG_OK;
}

int nidreg_cloud_fold(const nidreg_cloud* cloud, uint64_t seed, double cell, int num_folds, int fold, int complement, nidreg_cloud** out, int32_t* indices_out, int64_t* count_out) {
  const char* const who = "nidreg_cloud_fold";
  if (!out || !count_out) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null out / count_out");
  *out = nullptr;
  *count_out = 0;
  if (const char* why = fold_args_refusal(cell, num_folds)) return fail(NIDREG_ERR_INVALID, std::string(who) + ": " + why);
  if (fold < 0 || fold >= num_folds) return fail(NIDREG_ERR_INVALID, std::string(who) + ": fold must lie in [0, num_folds)");
  if (!cloud) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null cloud");
  const int64_t n = cloud->n;

  HIP_TRY(hipSetDevice(cloud->device));
  std::unique_ptr<nidreg_cloud> c(new nidreg_cloud());
  c->device = cloud->device;
  int total = 0;
  if (n > 0) {
    const int ntiles = int((n + kFoldTile - 1) / kFoldTile);
    ScratchArena& arena = ScratchArena::of(cloud->device);
    std::lock_guard<ScratchArena> guard(arena);
    const auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t b_flag = al(size_t(n)), b_count = al(3 * size_t(ntiles) * sizeof(int)), b_offset = al((size_t(ntiles) + 3) * sizeof(int)),
                 b_idx = indices_out ? al(size_t(n) * sizeof(int32_t)) : 0;
    HIP_TRY(arena.reserve(b_flag + b_count + b_offset + b_idx + 4096));
    unsigned char* const d_flag = static_cast<unsigned char*>(arena.carve(b_flag));
    int* const d_count = static_cast<int*>(arena.carve(b_count));
    int* const d_offset = static_cast<int*>(arena.carve(b_offset));
    int32_t* const d_idx = indices_out ? static_cast<int32_t*>(arena.carve(b_idx)) : nullptr;
    if (!d_flag || !d_count || !d_offset || (indices_out && !d_idx)) return fail(NIDREG_ERR_HIP, std::string(who) + ": scratch arena exhausted");
    HIP_TRY(launch(k_fold_flags, unsigned(ntiles), kFoldThreads, 0, nullptr, cloud->d_pts.as<double>(), n, seed, cell, num_folds, fold, complement ? 1 : 0, d_flag, d_count));
    HIP_TRY(launch_select_scan(d_count, ntiles, d_offset));
    HIP_TRY(hipMemcpy(&total, d_offset + ntiles, sizeof(int), hipMemcpyDeviceToHost));  // (synchronises the null stream)
    if (total < 0 || int64_t(total) > n) return fail(NIDREG_ERR_HIP, std::string(who) + ": the scan counted " + std::to_string(total) + " of " + std::to_string(n) + " points");
    const size_t m1 = size_t(std::max(total, 1));
    HIP_TRY(c->d_pts.alloc(m1 * 32));
    HIP_TRY(c->d_int.alloc(m1 * 8));
    if (total > 0) {
      HIP_TRY(launch_select_scatter(d_flag, d_offset, ntiles, cloud->d_pts.as<double>(), cloud->d_int.as<double>(), (long long)n, d_idx, c->d_pts.as<double>(), c->d_int.as<double>()));
      if (indices_out) HIP_TRY(hipMemcpy(indices_out, d_idx, size_t(total) * sizeof(int32_t), hipMemcpyDeviceToHost));
      HIP_TRY(hipStreamSynchronize(nullptr));  // the scratch is freed on return
    }
  } else {
    HIP_TRY(c->d_pts.alloc(32));
    HIP_TRY(c->d_int.alloc(8));
  }
  c->n = total;  // (sel_kept stays -1: nidreg_cloud_select_counts refuses a fold cloud)
  *count_out = total;
  *out = c.release();
  return NIDREG_OK;
}

}  // extern "C"
