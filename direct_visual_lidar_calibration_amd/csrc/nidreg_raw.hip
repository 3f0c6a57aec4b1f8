// nidreg_raw.hip -- C ABI of the raw image encodings (include/nidreg.h: nidreg_image_to_mono8) and the translation unit of their
// kernels (nid_raw_kernels.hpp).  Stateless, like nidreg_draw: validation (all of it BEFORE the device is touched), upload of the
// message's bytes as they lie, one launch, the copy back.  No CPU path for the arithmetic.
#include "nid_host.hpp"
#include "nid_raw_kernels.hpp"

using namespace nidreg;

namespace {

constexpr int kRawMaxDim = 16384;
const char* const kRawList =
    "mono8, mono16, rgb8, bgr8, rgba8, bgra8, rgb16, bgr16, rgba16, bgra16, yuv422, uyvy, yuv422_yuy2, yuyv and bayer_{rggb,bggr,gbrg,grbg}{8,16} are";

thread_local PhaseClock<3> g_raw_clock;  // of this thread's last nidreg_image_to_mono8: upload, kernel, copy back

struct RawEncoding {
  const char* name;
  int sample_bytes;  // 1 or 2
  int samples;       // per pixel, as stored
  int channels;      // 0: a Bayer mosaic; 1: the sample at index r; 3: luma of the samples at indices r, g, b
  int r, g, b;       // sample indices inside the pixel; for a mosaic r, g = the parity of the red pixels' column and row
};

// the letters of a Bayer name are the colours of row 0 (columns 0, 1), then row 1 (columns 0, 1)
const RawEncoding kRawEncodings[] = {
    {"mono8", 1, 1, 1, 0, 0, 0},       {"mono16", 2, 1, 1, 0, 0, 0},      {"rgb8", 1, 3, 3, 0, 1, 2},        {"bgr8", 1, 3, 3, 2, 1, 0},         {"rgba8", 1, 4, 3, 0, 1, 2},
    {"bgra8", 1, 4, 3, 2, 1, 0},       {"rgb16", 2, 3, 3, 0, 1, 2},       {"bgr16", 2, 3, 3, 2, 1, 0},       {"rgba16", 2, 4, 3, 0, 1, 2},       {"bgra16", 2, 4, 3, 2, 1, 0},
    {"yuv422", 1, 2, 1, 1, 0, 0},      {"uyvy", 1, 2, 1, 1, 0, 0},        {"yuv422_yuy2", 1, 2, 1, 0, 0, 0}, {"yuyv", 1, 2, 1, 0, 0, 0},         {"bayer_rggb8", 1, 1, 0, 0, 0, 0},
    {"bayer_bggr8", 1, 1, 0, 1, 1, 0}, {"bayer_gbrg8", 1, 1, 0, 0, 1, 0}, {"bayer_grbg8", 1, 1, 0, 1, 0, 0}, {"bayer_rggb16", 2, 1, 0, 0, 0, 0}, {"bayer_bggr16", 2, 1, 0, 1, 1, 0},
    {"bayer_gbrg16", 2, 1, 0, 0, 1, 0}, {"bayer_grbg16", 2, 1, 0, 1, 0, 0},
};

}  // namespace

extern "C" {

int nidreg_image_to_mono8(int device_id, const uint8_t* data, int64_t size, int width, int height, int64_t step, const char* encoding, int is_bigendian, uint8_t* out,
                          int64_t out_row_stride) {
  const std::string who = "nidreg_image_to_mono8";
  // every refusal comes before the device is touched, and nothing is written
  if (!encoding) return fail(NIDREG_ERR_INVALID, who + ": null encoding");
  const RawEncoding* e = nullptr;
  for (const RawEncoding& k : kRawEncodings)
    if (std::strcmp(k.name, encoding) == 0) e = &k;
  if (!e) return fail(NIDREG_ERR_INVALID, who + ": sensor_msgs/Image encoding '" + encoding + "' is not converted here (" + kRawList + ")");
  const std::string what = who + ": " + e->name + " image of " + std::to_string(width) + " x " + std::to_string(height) + ": ";
  if (!data || !out) return fail(NIDREG_ERR_INVALID, what + "null data or out");
  if (width < 1 || width > kRawMaxDim || height < 1 || height > kRawMaxDim) return fail(NIDREG_ERR_INVALID, what + "width and height must lie in [1, " + std::to_string(kRawMaxDim) + "]");
  if (e->channels == 0 && (width < 3 || height < 3)) return fail(NIDREG_ERR_INVALID, what + "a Bayer mosaic below 3 x 3 has no interior pixel and is not converted here");
  const int pixel_bytes = e->sample_bytes * e->samples;
  const int64_t row_bytes = int64_t(width) * pixel_bytes;
  if (step < row_bytes) return fail(NIDREG_ERR_INVALID, what + "step " + std::to_string(step) + " is below the " + std::to_string(row_bytes) + " bytes of a row");
  if (size < 0 || size / step < height)  // size < height * step, without the product
    return fail(NIDREG_ERR_INVALID, what + std::to_string(size) + " data bytes for " + std::to_string(height) + " rows of step " + std::to_string(step));
  if (out_row_stride != 0 && out_row_stride < width) return fail(NIDREG_ERR_INVALID, what + "out_row_stride " + std::to_string(out_row_stride) + " is below the width");
  const int64_t stride = out_row_stride > 0 ? out_row_stride : int64_t(width);
  if (const int rc = use_device(who.c_str(), device_id)) return rc;

  g_raw_clock.start();
  const size_t W = size_t(width), H = size_t(height);
  const int w4 = (width + 3) / 4;
  const size_t dev_stride = size_t(w4) * 4;  // device image: rows of whole 4-byte groups
  const size_t src_bytes = H * size_t(step);
  DeviceBuf d_src, d_out;
  HIP_TRY(d_src.alloc(src_bytes));
  HIP_TRY(d_out.alloc(dev_stride * H));
  HIP_TRY(hipMemcpy(d_src.as<void>(), data, src_bytes, hipMemcpyHostToDevice));
  g_raw_clock.lap(0);

  const unsigned grid = blocks_for((long long)w4 * height, kRawThreads);
  const int big = e->sample_bytes == 2 && is_bigendian != 0;  // 8-bit encodings ignore the flag
  const RawFormat f = {pixel_bytes, e->channels, e->r * e->sample_bytes, e->g * e->sample_bytes, e->b * e->sample_bytes, big};
  hipError_t launched = hipErrorInvalidValue;
  with_int<1, 2>(e->sample_bytes, [&](auto BYTES) {
    if (e->channels == 0)
      launched = launch(k_raw_bayer<BYTES>, grid, kRawThreads, 0, nullptr, d_src.as<uint8_t>(), step, e->r, e->g, big, width, w4, height, d_out.as<uint8_t>(), dev_stride);
    else
      launched = launch(k_raw_pixels<BYTES>, grid, kRawThreads, 0, nullptr, d_src.as<uint8_t>(), step, f, width, w4, height, d_out.as<uint8_t>(), dev_stride);
  });
  HIP_TRY(launched);
  HIP_TRY(hipStreamSynchronize(nullptr));
  g_raw_clock.lap(1);

  HIP_TRY(hipMemcpy2D(out, size_t(stride), d_out.as<void>(), dev_stride, W, H, hipMemcpyDeviceToHost));  // W bytes a row: the caller's padding stays
  g_raw_clock.lap(2);
  return NIDREG_OK;
}

int nidreg_image_get_timing(double* ms3) { return g_raw_clock.read("nidreg_image_get_timing", ms3); }

}  // extern "C"
