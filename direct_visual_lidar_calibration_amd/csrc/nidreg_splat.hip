// nidreg_splat.hip -- C ABI of the headless viewer's renderer (include/nidreg.h: nidreg_splat_*) and the translation unit of its
// kernels (nid_splat_kernels.hpp; -ffp-contract=off and the exact-order projection, like nid_kernels_f64_exact.hip).  Not one of the
// evaluation kernels' sources: nidreg_kernel_build() does not cover it.  Host side: device residency and launches.  No CPU path.
#define NID_RENDER_FRONT_END_ONLY  // the non-template kernels of nid_render_kernels.hpp belong to nid_kernels_f64_exact.hip
#include "nid_splat_kernels.hpp"
#include "nid_host.hpp"

#include <memory>
#include <string>

using namespace nidreg;

struct nidreg_splat {
  int device = 0;
  long long n = 0, stride_d = 4;
  bool colored = false;
  size_t cap_pix = 0;   // pixels the per-draw buffers hold
  DeviceBuf d_pts;      // double[n * stride_d]
  DeviceBuf d_rgba;     // uint8_t[4 n]
  DeviceBuf d_zkey;     // u64[cap_pix]
  DeviceBuf d_bg;       // uint8_t[3 cap_pix]
  DeviceBuf d_rgb;      // uint8_t[3 cap_pix]
  DeviceBuf d_index;    // int[cap_pix]
  hipStream_t stream = nullptr;
};

namespace {

void splat_free(nidreg_splat* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamDestroy(s->stream);  // (idle: nidreg_splat_draw synchronises it before it returns)
  delete s;
}

}  // namespace

extern "C" {

int nidreg_splat_create(int device_id, int64_t num_points, const double* points, int64_t point_stride, nidreg_splat** out) {
  const char* const who = "nidreg_splat_create";
  if (!out) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null out");
  *out = nullptr;
  if (num_points < 0) return fail(NIDREG_ERR_INVALID, std::string(who) + ": negative num_points");
  if (num_points > 2147483647LL) return fail(NIDREG_ERR_INVALID, std::string(who) + ": more than 2^31 - 1 points (the index half of a depth key is 32 bits)");
  if (num_points > 0 && !points) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null points");
  const int64_t stride = point_stride > 0 ? point_stride : 32;
  if (stride % 8 != 0 || stride < 32) return fail(NIDREG_ERR_INVALID, std::string(who) + ": point_stride must be a multiple of 8, at least 32");
  if (const int rc = use_device(who, device_id)) return rc;
  std::unique_ptr<nidreg_splat, void (*)(nidreg_splat*)> s(new nidreg_splat(), splat_free);
  s->device = device_id;
  s->n = num_points;
  s->stride_d = stride / 8;
  HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  if (num_points > 0) {
    const size_t n = size_t(num_points);
    HIP_TRY(s->d_pts.alloc(n * size_t(stride)));
    HIP_TRY(hipMemcpy(s->d_pts.as<void>(), points, n * size_t(stride), hipMemcpyHostToDevice));
    HIP_TRY(s->d_rgba.alloc(n * 4));
  }
  *out = s.release();
  return NIDREG_OK;
}

int nidreg_splat_set_colors(nidreg_splat* s, const uint8_t* rgba) {
  if (!s || (s->n > 0 && !rgba)) return fail(NIDREG_ERR_INVALID, "nidreg_splat_set_colors: null argument");
  if (s->n > 0) {
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpy(s->d_rgba.as<void>(), rgba, size_t(s->n) * 4, hipMemcpyHostToDevice));
  }
  s->colored = true;
  return NIDREG_OK;
}

int nidreg_splat_draw(nidreg_splat* s, int model_id, const double* intrinsics, const double* distortion, int width, int height, double min_nz, const double* T_view_lidar, int radius,
                      const uint8_t* background_rgb, int64_t background_row_stride, int alpha, uint8_t* out_rgb, int32_t* out_index) {
  const char* const who = "nidreg_splat_draw";
  if (!s || !intrinsics || !distortion || !T_view_lidar || !out_rgb) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null argument");
  if (model_id < 0 || model_id > 5) return fail(NIDREG_ERR_INVALID, std::string(who) + ": unknown model");
  if (width < 1 || height < 1) return fail(NIDREG_ERR_INVALID, std::string(who) + ": width and height must be positive");
  if (int64_t(width) * int64_t(height) > 2147483647LL) return fail(NIDREG_ERR_INVALID, std::string(who) + ": width * height overflows int");
  if (radius < 0 || radius > kSplatMaxRadius) return fail(NIDREG_ERR_INVALID, std::string(who) + ": radius must lie in [0, " + std::to_string(kSplatMaxRadius) + "]");
  if (alpha < 0 || alpha > 255) return fail(NIDREG_ERR_INVALID, std::string(who) + ": alpha must lie in [0, 255]");
  const int64_t row = int64_t(width) * 3;
  const int64_t bg_stride = background_row_stride > 0 ? background_row_stride : row;
  if (background_rgb && bg_stride < row) return fail(NIDREG_ERR_INVALID, std::string(who) + ": background_row_stride below a row (3 * width bytes)");
  if (s->n > 0 && !s->colored) return fail(NIDREG_ERR_INVALID, std::string(who) + ": no colours set (nidreg_splat_set_colors)");
  HIP_TRY(hipSetDevice(s->device));
  const size_t npix = size_t(width) * size_t(height);
  if (npix > s->cap_pix) {
    s->cap_pix = 0;
    HIP_TRY(s->d_zkey.alloc(npix * sizeof(u64)));
    HIP_TRY(s->d_bg.alloc(npix * 3));
    HIP_TRY(s->d_rgb.alloc(npix * 3));
    HIP_TRY(s->d_index.alloc(npix * sizeof(int)));
    s->cap_pix = npix;
  }
  if (background_rgb)
    HIP_TRY(hipMemcpy2DAsync(s->d_bg.as<void>(), size_t(row), background_rgb, size_t(bg_stride), size_t(row), size_t(height), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemsetAsync(s->d_zkey.as<void>(), 0xff, npix * sizeof(u64), s->stream));  // kSplatEmpty, every draw
  if (s->n > 0) {
    const CamParams<double> cam = make_cam(model_id, intrinsics, distortion);
    IsoParams<double> iso;
    for (int k = 0; k < 12; k++) iso.m[k] = T_view_lidar[k];
    HIP_TRY(with_model(model_id, hipErrorInvalidValue, [&](auto M) {
      return launch(k_splat_depth<M>, blocks_for(s->n, 256), 256, 0, s->stream, s->d_pts.as<double>(), s->stride_d, s->n, iso, cam, width, height, min_nz, radius, s->d_zkey.as<u64>());
    }));
  }
  HIP_TRY(launch(k_splat_resolve, blocks_for(npix, 256), 256, 0, s->stream, s->d_zkey.as<u64>(), npix, s->d_rgba.as<uchar4>(), background_rgb ? s->d_bg.as<uint8_t>() : nullptr, alpha,
                 s->d_rgb.as<uint8_t>(), out_index ? s->d_index.as<int>() : nullptr));
  HIP_TRY(hipMemcpyAsync(out_rgb, s->d_rgb.as<void>(), npix * 3, hipMemcpyDeviceToHost, s->stream));
  if (out_index) HIP_TRY(hipMemcpyAsync(out_index, s->d_index.as<void>(), npix * sizeof(int), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return NIDREG_OK;
}

void nidreg_splat_destroy(nidreg_splat* s) { splat_free(s); }

}  // extern "C"
