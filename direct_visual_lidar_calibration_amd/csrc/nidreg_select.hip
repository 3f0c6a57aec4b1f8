// nidreg_select.hip -- C ABI of masks and range gates (include/nidreg.h: nidreg_mask_*, nidreg_cloud_select, nidreg_cloud_size):
// ViewCulling::cull as every handle construction runs it (launch_cull, unchanged), then a flag pass, an exclusive scan of the
// per-tile counts and a gather into a new device cloud (kernels and the selection rule: nid_select_kernels.hpp).  Built
// -ffp-contract=off like nid_build.hip: the range gate's (x x + y y) + z z is the expression a host restatement evaluates.
#include "nidreg_internal.hpp"
#include "nid_select_kernels.hpp"

struct nidreg_mask {
  int device = 0;
  int W = 0, H = 0, margin = 0;
  DeviceBuf d_eroded;  // W x H bytes, rows W apart
};

namespace {

constexpr int kMaskMaxDim = 16384, kMaskMaxMargin = 64;

bool size_ok(int width, int height) { return width >= 1 && width <= kMaskMaxDim && height >= 1 && height <= kMaskMaxDim; }

}  // namespace

// the compaction behind another flag pass (nidreg_fold.hip; declared in nid_launch.hpp): the two kernels as nidreg_cloud_select launches them
namespace nidreg {

hipError_t launch_select_scan(const int* d_count, int ntiles, int* d_offset) {
  return launch(k_select_scan, 1, kSelectThreads, 0, nullptr, d_count, ntiles, d_offset);
}

hipError_t launch_select_scatter(const unsigned char* d_flag, const int* d_offset, int ntiles, const double* d_pts, const double* d_int, long long n, int32_t* d_idx_out, double* d_pts_out,
                                 double* d_int_out) {
  return launch(k_select_scatter, unsigned(ntiles), kSelectThreads, 0, nullptr, d_flag, d_offset, d_pts, d_int, n, d_idx_out, d_pts_out, d_int_out);
}

}  // namespace nidreg

extern "C" {

int nidreg_mask_create(int device_id, const uint8_t* mask, int width, int height, int64_t row_stride, int margin, nidreg_mask** out) {
  const char* const who = "nidreg_mask_create";
  if (!out) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null out");
  *out = nullptr;
  if (!mask) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null mask");
  if (!size_ok(width, height)) return fail(NIDREG_ERR_INVALID, std::string(who) + ": width and height must lie in [1, 16384]");
  if (row_stride < width) return fail(NIDREG_ERR_INVALID, std::string(who) + ": a row stride below the width");
  if (margin < 0 || margin > kMaskMaxMargin) return fail(NIDREG_ERR_INVALID, std::string(who) + ": margin must lie in [0, 64]");
  if (device_id < 0) return fail(NIDREG_ERR_INVALID, std::string(who) + ": device_id out of range");  // (before the device count is asked for)
  if (const int rc = use_device(who, device_id)) return rc;
  std::unique_ptr<nidreg_mask> m(new nidreg_mask());
  m->device = device_id, m->W = width, m->H = height, m->margin = margin;
  const size_t bytes = size_t(width) * size_t(height);
  DeviceBuf d_src, d_rows;
  HIP_TRY(m->d_eroded.alloc(bytes));
  if (margin == 0) {  // the erosion over one pixel is the mask itself
    HIP_TRY(hipMemcpy2D(m->d_eroded.as<void>(), size_t(width), mask, size_t(row_stride), size_t(width), size_t(height), hipMemcpyHostToDevice));
  } else {
    HIP_TRY(d_src.alloc(bytes));
    HIP_TRY(d_rows.alloc(bytes));
    HIP_TRY(hipMemcpy2D(d_src.as<void>(), size_t(width), mask, size_t(row_stride), size_t(width), size_t(height), hipMemcpyHostToDevice));
    const unsigned grid = blocks_for(bytes, 256);
    HIP_TRY(launch(k_mask_erode, grid, 256, 0, nullptr, d_src.as<uint8_t>(), d_rows.as<uint8_t>(), width, height, margin, 1));
    HIP_TRY(launch(k_mask_erode, grid, 256, 0, nullptr, d_rows.as<uint8_t>(), m->d_eroded.as<uint8_t>(), width, height, margin, 0));
    HIP_TRY(hipStreamSynchronize(nullptr));  // the temporaries are freed on return
  }
  *out = m.release();
  return NIDREG_OK;
}

int nidreg_mask_get(const nidreg_mask* mask, uint8_t* eroded_out, int64_t row_stride) {
  if (!mask || !eroded_out) return fail(NIDREG_ERR_INVALID, "nidreg_mask_get: null argument");
  if (row_stride < mask->W) return fail(NIDREG_ERR_INVALID, "nidreg_mask_get: a row stride below the width");
  HIP_TRY(hipSetDevice(mask->device));
  HIP_TRY(hipMemcpy2D(eroded_out, size_t(row_stride), mask->d_eroded.as<void>(), size_t(mask->W), size_t(mask->W), size_t(mask->H), hipMemcpyDeviceToHost));
  return NIDREG_OK;
}

void nidreg_mask_destroy(nidreg_mask* mask) {
  if (!mask) return;
  (void)hipSetDevice(mask->device);
  delete mask;
}

int nidreg_cloud_size(const nidreg_cloud* cloud, int64_t* n) {
  if (!cloud || !n) return fail(NIDREG_ERR_INVALID, "nidreg_cloud_size: null argument");
  *n = cloud->n;
  return NIDREG_OK;
}

int nidreg_cloud_get(const nidreg_cloud* cloud, double* points_out, double* intensities_out) {
  if (!cloud) return fail(NIDREG_ERR_INVALID, "nidreg_cloud_get: null cloud");
  if (cloud->n == 0 || (!points_out && !intensities_out)) return NIDREG_OK;
  HIP_TRY(hipSetDevice(cloud->device));
  if (points_out) HIP_TRY(hipMemcpy(points_out, cloud->d_pts.as<void>(), size_t(cloud->n) * 32, hipMemcpyDeviceToHost));
  if (intensities_out) HIP_TRY(hipMemcpy(intensities_out, cloud->d_int.as<void>(), size_t(cloud->n) * 8, hipMemcpyDeviceToHost));
  return NIDREG_OK;
}

int nidreg_cloud_select_counts(const nidreg_cloud* selected, int64_t* counts3) {
  if (!selected || !counts3) return fail(NIDREG_ERR_INVALID, "nidreg_cloud_select_counts: null argument");
  if (selected->sel_kept < 0) return fail(NIDREG_ERR_INVALID, "nidreg_cloud_select_counts: the cloud does not come from nidreg_cloud_select");
  counts3[0] = selected->sel_kept, counts3[1] = selected->sel_masked, counts3[2] = selected->sel_ranged;
  return NIDREG_OK;
}

int nidreg_cloud_select(const nidreg_cloud* cloud, int model_id, const double* intrinsics, const double* distortion, int width, int height, const double* T_camera_lidar, double min_z,
                        int enable_depth_buffer_culling, const nidreg_mask* mask, double min_range, double max_range, nidreg_cloud** out, int32_t* indices_out, int64_t* count_out) {
  const char* const who = "nidreg_cloud_select";
  if (!out || !count_out) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null out / count_out");
  *out = nullptr;
  *count_out = 0;
  if (!cloud || !intrinsics || !distortion || !T_camera_lidar) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null argument");
  if (model_id < 0 || model_id > 5) return fail(NIDREG_ERR_INVALID, std::string(who) + ": unknown camera model");
  if (!size_ok(width, height)) return fail(NIDREG_ERR_INVALID, std::string(who) + ": width and height must lie in [1, 16384]");
  if (mask && (mask->W != width || mask->H != height))
    return fail(NIDREG_ERR_INVALID, std::string(who) + ": the mask is " + std::to_string(mask->W) + "x" + std::to_string(mask->H) + ", the image " + std::to_string(width) + "x" + std::to_string(height));
  if (mask && mask->device != cloud->device) return fail(NIDREG_ERR_INVALID, std::string(who) + ": the mask and the cloud live on different devices");
  if (!(min_range >= 0.0) || !(max_range >= min_range)) return fail(NIDREG_ERR_INVALID, std::string(who) + ": 0 <= min_range <= max_range expected (neither may be NaN)");
  const int64_t n = cloud->n;
  const double min2 = min_range * min_range, max2 = max_range * max_range;

  HIP_TRY(hipSetDevice(cloud->device));
  std::unique_ptr<nidreg_cloud> c(new nidreg_cloud());
  c->device = cloud->device;
  int total = 0;
  int sums[3] = {0, 0, 0};  // selected, kept by the cull, of those removed by the mask
  if (n > 0) {
    const int ntiles = int((n + kSelectTile - 1) / kSelectTile);
    // scratch from the per-device construction arena (nid_launch.hpp): a selection precedes every handle construction of a masked
    // calibration, and hipMalloc / hipFree of the temporaries would cost more than the kernels
    ScratchArena& arena = ScratchArena::of(cloud->device);
    std::lock_guard<ScratchArena> guard(arena);
    const auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t b_pix = al(size_t(n) * sizeof(int)), b_zbuf = al(size_t(width) * height * sizeof(unsigned int)), b_keep = al(size_t(n)), b_flag = al(size_t(n)),
                 b_count = al(3 * size_t(ntiles) * sizeof(int)), b_offset = al((size_t(ntiles) + 3) * sizeof(int)), b_idx = indices_out ? al(size_t(n) * sizeof(int32_t)) : 0;
    HIP_TRY(arena.reserve(b_pix + b_zbuf + b_keep + b_flag + b_count + b_offset + b_idx + 4096));
    int* const d_pix = static_cast<int*>(arena.carve(b_pix));
    unsigned int* const d_zbuf = static_cast<unsigned int*>(arena.carve(b_zbuf));
    unsigned char* const d_keep = static_cast<unsigned char*>(arena.carve(b_keep));
    unsigned char* const d_flag = static_cast<unsigned char*>(arena.carve(b_flag));
    int* const d_count = static_cast<int*>(arena.carve(b_count));
    int* const d_offset = static_cast<int*>(arena.carve(b_offset));
    int32_t* const d_idx = indices_out ? static_cast<int32_t*>(arena.carve(b_idx)) : nullptr;
    if (!d_pix || !d_zbuf || !d_keep || !d_flag || !d_count || !d_offset || (indices_out && !d_idx)) return fail(NIDREG_ERR_HIP, std::string(who) + ": scratch arena exhausted");
    // the cull exactly as nidreg_view_culling and build_records_device run it
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_zbuf), 0x7f800000, size_t(width) * height, nullptr));
    HIP_TRY(launch_cull(model_id, intrinsics, distortion, cloud->d_pts.as<double>(), 4, n, T_camera_lidar, width, height, min_z, enable_depth_buffer_culling ? 1 : 0, d_pix,
                        d_zbuf, d_keep, nullptr));
    HIP_TRY(launch(k_select_flags, unsigned(ntiles), kSelectThreads, 0, nullptr, d_keep, d_pix, mask ? mask->d_eroded.as<uint8_t>() : nullptr, cloud->d_pts.as<double>(), n, min2, max2,
                   d_flag, d_count));
    HIP_TRY(launch_select_scan(d_count, ntiles, d_offset));
    HIP_TRY(hipMemcpy(sums, d_offset + ntiles, sizeof(sums), hipMemcpyDeviceToHost));  // (synchronises the null stream)
    total = sums[0];
    if (total < 0 || int64_t(total) > n) return fail(NIDREG_ERR_HIP, std::string(who) + ": the scan counted " + std::to_string(total) + " of " + std::to_string(n) + " points");
    const size_t m1 = size_t(std::max(total, 1));
    HIP_TRY(c->d_pts.alloc(m1 * 32));
    HIP_TRY(c->d_int.alloc(m1 * 8));
    if (total > 0) {
      HIP_TRY(launch_select_scatter(d_flag, d_offset, ntiles, cloud->d_pts.as<double>(), cloud->d_int.as<double>(), n, d_idx, c->d_pts.as<double>(), c->d_int.as<double>()));
      if (indices_out) HIP_TRY(hipMemcpy(indices_out, d_idx, size_t(total) * sizeof(int32_t), hipMemcpyDeviceToHost));
      HIP_TRY(hipStreamSynchronize(nullptr));  // the scratch is freed on return
    }
  } else {
    HIP_TRY(c->d_pts.alloc(32));
    HIP_TRY(c->d_int.alloc(8));
  }
  c->n = total;
  c->sel_kept = sums[1], c->sel_masked = sums[2], c->sel_ranged = int64_t(sums[1]) - sums[2] - sums[0];
  *count_out = total;
  *out = c.release();
  return NIDREG_OK;
}

}  // extern "C"
