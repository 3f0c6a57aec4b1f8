// nidreg_render.hip -- C ABI of the two point-to-image consumers next to the NID path
// (include/nidreg.h: nidreg_colorizer_*, nidreg_generate_lidar_image).  Host side only: device
// residency and launches; the kernels are in nid_render_kernels.hpp.  No CPU compute path.
#include "nid_device.hpp"
#include "nid_launch.hpp"

#include <cstring>
#include <memory>
#include <string>

using namespace nidreg;

struct nidreg_colorizer {
  int device = 0, model = 0, W = 0, H = 0;
  double intr[5] = {0, 0, 0, 0, 0}, dist[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double min_nz = 0.0;
  long long n = 0, stride_d = 4;
  DeviceBuf d_pts;     // double[n * stride_d]
  DeviceBuf d_icolor;  // float[4 n]; empty: (1,1,1,1)
  DeviceBuf d_out;     // float[4 n]
  DeviceBuf d_img;     // uint8_t[W * H]
  hipStream_t stream = nullptr;
};

namespace {

void colorizer_free(nidreg_colorizer* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamDestroy(c->stream);  // (idle: nidreg_colorizer_update synchronises it before it returns)
  delete c;
}

}  // namespace

extern "C" {

int nidreg_colorizer_create(int device_id, int model_id, const double* intrinsics, const double* distortion, int width, int height, const uint8_t* image, int64_t image_row_stride,
                            int64_t num_points, const double* points, int64_t point_stride, const float* intensity_colors, double min_nz, nidreg_colorizer** out) {
  if (!out) return fail(NIDREG_ERR_INVALID, "nidreg_colorizer_create: null out");
  *out = nullptr;
  if (model_id < 0 || model_id > 5 || !intrinsics || !distortion || width < 1 || height < 1 || !image || num_points < 0 || (num_points > 0 && !points))
    return fail(NIDREG_ERR_INVALID, "nidreg_colorizer_create: bad argument");
  const int64_t stride = point_stride > 0 ? point_stride : 32;
  if (stride % 8 != 0 || stride < 32) return fail(NIDREG_ERR_INVALID, "nidreg_colorizer_create: point_stride must be a multiple of 8, at least 32");
  const int64_t rs = image_row_stride > 0 ? image_row_stride : width;
  if (rs < width) return fail(NIDREG_ERR_INVALID, "nidreg_colorizer_create: image_row_stride < width");
  if (const int rc = use_device("nidreg_colorizer_create", device_id)) return rc;
  std::unique_ptr<nidreg_colorizer, void (*)(nidreg_colorizer*)> c(new nidreg_colorizer(), colorizer_free);
  c->device = device_id;
  c->model = model_id;
  c->W = width;
  c->H = height;
  c->min_nz = min_nz;
  c->n = num_points;
  c->stride_d = stride / 8;
  std::memcpy(c->intr, intrinsics, sizeof(c->intr));
  std::memcpy(c->dist, distortion, sizeof(c->dist));
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  const size_t n = size_t(num_points);
  HIP_TRY(c->d_img.alloc(size_t(width) * height));
  HIP_TRY(hipMemcpy2D(c->d_img.as<void>(), size_t(width), image, size_t(rs), size_t(width), size_t(height), hipMemcpyHostToDevice));
  if (n > 0) {
    HIP_TRY(c->d_pts.alloc(n * size_t(stride)));
    HIP_TRY(hipMemcpy(c->d_pts.as<void>(), points, n * size_t(stride), hipMemcpyHostToDevice));
    HIP_TRY(c->d_out.alloc(n * 4 * sizeof(float)));
    if (intensity_colors) {
      HIP_TRY(c->d_icolor.alloc(n * 4 * sizeof(float)));
      HIP_TRY(hipMemcpy(c->d_icolor.as<void>(), intensity_colors, n * 4 * sizeof(float), hipMemcpyHostToDevice));
    }
  }
  *out = c.release();
  return NIDREG_OK;
}

int nidreg_colorizer_update(nidreg_colorizer* c, const double* T_camera_lidar, double blend_weight, float* colors_out) {
  if (!c || !T_camera_lidar) return fail(NIDREG_ERR_INVALID, "nidreg_colorizer_update: null argument");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(launch_colorize(c->model, c->intr, c->dist, c->d_pts.as<double>(), c->stride_d, c->n, T_camera_lidar, c->d_img.as<uint8_t>(), c->W, c->H, c->min_nz, c->d_icolor.as<float>(),
                          blend_weight, c->d_out.as<float>(), c->stream));
  if (colors_out && c->n > 0) HIP_TRY(hipMemcpyAsync(colors_out, c->d_out.as<void>(), size_t(c->n) * 4 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return NIDREG_OK;
}

const float* nidreg_colorizer_device_colors(nidreg_colorizer* c) { return c ? c->d_out.as<float>() : nullptr; }

void nidreg_colorizer_destroy(nidreg_colorizer* c) { colorizer_free(c); }

int nidreg_generate_lidar_image(int model_id, const double* intrinsics, const double* distortion, int device_id, int width, int height, double min_nz, const double* points,
                                int64_t point_stride, const double* intensities, int64_t num_points, const double* T_camera_lidar, double* intensity_image, int32_t* index_image) {
  if (model_id < 0 || model_id > 5 || !intrinsics || !distortion || width < 1 || height < 1 || num_points < 0 || num_points > 2147483647LL || !T_camera_lidar ||
      (num_points > 0 && (!points || !intensities)) || (!intensity_image && !index_image))
    return fail(NIDREG_ERR_INVALID, "nidreg_generate_lidar_image: bad argument");
  const int64_t stride = point_stride > 0 ? point_stride : 32;
  if (stride % 8 != 0 || stride < 32) return fail(NIDREG_ERR_INVALID, "nidreg_generate_lidar_image: point_stride must be a multiple of 8, at least 32");
  if (const int rc = use_device("nidreg_generate_lidar_image", device_id)) return rc;
  const size_t n = size_t(num_points), npix = size_t(width) * size_t(height);
  DeviceBuf d_pts, d_int, d_pix, d_idx, d_iimg, d_zmin;
  HIP_TRY(d_zmin.alloc(npix * sizeof(u64)));
  HIP_TRY(d_idx.alloc(npix * sizeof(int)));
  HIP_TRY(d_iimg.alloc(npix * sizeof(double)));
  if (n > 0) {
    HIP_TRY(d_pts.alloc(n * size_t(stride)));
    HIP_TRY(d_int.alloc(n * sizeof(double)));
    HIP_TRY(d_pix.alloc(n * sizeof(int)));
    HIP_TRY(hipMemcpy(d_pts.as<void>(), points, n * size_t(stride), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_int.as<void>(), intensities, n * sizeof(double), hipMemcpyHostToDevice));
  }
  HIP_TRY(launch_lidar_image(model_id, intrinsics, distortion, d_pts.as<double>(), stride / 8, d_int.as<double>(), num_points, T_camera_lidar, width, height, min_nz, d_pix.as<int>(),
                             d_zmin.as<u64>(), d_idx.as<int>(), d_iimg.as<double>(), nullptr));
  HIP_TRY(hipDeviceSynchronize());
  if (intensity_image) HIP_TRY(hipMemcpy(intensity_image, d_iimg.as<void>(), npix * sizeof(double), hipMemcpyDeviceToHost));
  if (index_image) HIP_TRY(hipMemcpy(index_image, d_idx.as<void>(), npix * sizeof(int), hipMemcpyDeviceToHost));
  return NIDREG_OK;
}

int nidreg_equalize_intensities(int device_id, double* intensities, int64_t num_points) {
  if (num_points < 0 || num_points > 4294967295LL || (num_points > 0 && !intensities)) return fail(NIDREG_ERR_INVALID, "nidreg_equalize_intensities: bad argument");
  if (num_points == 0) return NIDREG_OK;
  if (const int rc = use_device("nidreg_equalize_intensities", device_id)) return rc;
  DeviceBuf d;
  HIP_TRY(d.alloc(size_t(num_points) * sizeof(double)));
  HIP_TRY(hipMemcpy(d.as<void>(), intensities, size_t(num_points) * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(equalize_intensities_device(d.as<double>(), num_points, nullptr));
  HIP_TRY(hipMemcpy(intensities, d.as<void>(), size_t(num_points) * sizeof(double), hipMemcpyDeviceToHost));
  return NIDREG_OK;
}

}  // extern "C"
