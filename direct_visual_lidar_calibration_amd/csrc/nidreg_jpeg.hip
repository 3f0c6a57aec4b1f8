// nidreg_jpeg.hip -- C ABI of the baseline JPEG decoder (include/nidreg.h: nidreg_jpeg_*) and the translation unit of its kernels
// (nid_jpeg_kernels.hpp).  Host side: validation and entropy decode (nid_jpeg_host.hpp, all of it BEFORE the device is touched),
// then upload of the quantised coefficients and tables, the launches, the copy back.  No CPU path for the arithmetic.
#include "nid_jpeg_host.hpp"
#include "nid_jpeg_kernels.hpp"
#include "nid_host.hpp"

using namespace nidreg;

namespace {

thread_local PhaseClock<4> g_jpeg_clock;  // of this thread's last nidreg_jpeg_decode_gray: entropy, upload, kernels, copy back

int refuse(const char* who, const std::string& reason) {
  return fail(NIDREG_ERR_INVALID, std::string(who) + ": JPEG images are not decoded here unless they are baseline 8-bit Huffman streams (" + reason + ")");
}

// parse (and decode the entropy data of) untrusted bytes; an allocation failure is a refusal like any other
int parse_stream(const char* who, const uint8_t* data, int64_t size, bool entropy, nidjpeg::Stream& s) {
  if (!data || size <= 0) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null or empty data");
  std::string reason;
  try {
    if (!nidjpeg::parse(data, size_t(size), entropy, s, reason)) return refuse(who, reason);
  } catch (const std::bad_alloc&) {
    return refuse(who, "no host memory for the coefficients of " + std::to_string(s.width) + " x " + std::to_string(s.height) + " pixels");
  }
  return NIDREG_OK;
}

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

extern "C" {

int nidreg_jpeg_info(const uint8_t* data, int64_t size, int32_t* width, int32_t* height, int32_t* components, int32_t* subsampling, int32_t* exif_orientation) {
  const char* const who = "nidreg_jpeg_info";
  nidjpeg::Stream s;
  if (const int rc = parse_stream(who, data, size, false, s)) return rc;
  if (width) *width = s.width;
  if (height) *height = s.height;
  if (components) *components = s.ncomp;
  if (subsampling) *subsampling = s.subsampling;
  if (exif_orientation) *exif_orientation = s.orientation;
  return NIDREG_OK;
}

int nidreg_jpeg_coefficients(const uint8_t* data, int64_t size, int component, int16_t* out, int64_t capacity, uint16_t* qtable_out) {
  const char* const who = "nidreg_jpeg_coefficients";
  if (!out || capacity < 0) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null out or negative capacity");
  nidjpeg::Stream s;
  if (const int rc = parse_stream(who, data, size, true, s)) return rc;
  if (component < 0 || component >= s.ncomp) return fail(NIDREG_ERR_INVALID, std::string(who) + ": component out of range");
  const nidjpeg::Component& k = s.comp[component];
  const size_t count = size_t(k.bw) * size_t(k.bh) * 64;
  if (size_t(capacity) < count) return fail(NIDREG_ERR_INVALID, std::string(who) + ": capacity below the component's " + std::to_string(count) + " coefficients");
  std::memcpy(out, s.coef.data() + k.block_offset * 64, count * sizeof(int16_t));
  if (qtable_out) std::memcpy(qtable_out, s.qt[k.tq], 64 * sizeof(uint16_t));
  return NIDREG_OK;
}

int nidreg_jpeg_decode_gray(int device_id, const uint8_t* data, int64_t size, int mode, uint8_t* out, int64_t row_stride) {
  const char* const who = "nidreg_jpeg_decode_gray";
  if (!out) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null out");
  if (mode != NIDREG_JPEG_GRAY_LUMA && mode != NIDREG_JPEG_GRAY_BGR) return fail(NIDREG_ERR_INVALID, std::string(who) + ": unknown mode");
  if (row_stride < 0) return fail(NIDREG_ERR_INVALID, std::string(who) + ": negative row_stride");
  g_jpeg_clock.start();
  nidjpeg::Stream s;
  if (const int rc = parse_stream(who, data, size, true, s)) return rc;
  const int64_t stride = row_stride > 0 ? row_stride : int64_t(s.width);
  if (stride < s.width) return fail(NIDREG_ERR_INVALID, std::string(who) + ": row_stride below the width");
  g_jpeg_clock.lap(0);
  if (const int rc = use_device(who, device_id)) return rc;

  // the planes the colour kernel needs: none for one component or the LUMA mode (the Y blocks go straight into the cropped image)
  const bool color = s.ncomp == 3 && mode == NIDREG_JPEG_GRAY_BGR;
  const int ncomp_used = color ? 3 : 1;
  const size_t W = size_t(s.width), H = size_t(s.height);
  const size_t out_stride = round_up(W, 8);  // device image: rows of whole 8-byte groups
  size_t used_blocks = 0;
  for (int c = 0; c < ncomp_used; c++) used_blocks += size_t(s.comp[c].bw) * size_t(s.comp[c].bh);

  // one upload block: the used components' coefficients (they come first in s.coef), then their tables, 64 entries each
  g_jpeg_clock.start();  // (use_device belongs to no phase)
  const size_t coef_bytes = used_blocks * 64 * sizeof(int16_t);
  DeviceBuf d_in, d_planes, d_out;
  HIP_TRY(d_in.alloc(coef_bytes + 3 * 64 * sizeof(uint16_t)));
  HIP_TRY(d_out.alloc(out_stride * H));
  size_t plane_off[3] = {0, 0, 0}, plane_bytes = 0;
  if (color) {
    for (int c = 0; c < 3; c++) {
      plane_off[c] = plane_bytes;
      plane_bytes += round_up(size_t(s.comp[c].bw) * 8 * size_t(s.comp[c].bh) * 8, 256);
    }
    HIP_TRY(d_planes.alloc(plane_bytes));
  }
  uint16_t tables[3][64];
  for (int c = 0; c < 3; c++) std::memcpy(tables[c], s.qt[s.comp[c < s.ncomp ? c : 0].tq], sizeof(tables[c]));
  HIP_TRY(hipMemcpy(d_in.as<void>(), s.coef.data(), coef_bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_in.as<uint8_t>() + coef_bytes, tables, sizeof(tables), hipMemcpyHostToDevice));
  g_jpeg_clock.lap(1);

  const uint16_t* const d_qt = reinterpret_cast<const uint16_t*>(d_in.as<uint8_t>() + coef_bytes);
  for (int c = 0; c < ncomp_used; c++) {
    const nidjpeg::Component& k = s.comp[c];
    const long long nblocks = (long long)k.bw * k.bh;
    uint8_t* const dst = color ? d_planes.as<uint8_t>() + plane_off[c] : d_out.as<uint8_t>();
    const long long dst_stride = color ? (long long)k.bw * 8 : (long long)out_stride;
    const int dst_rows = color ? k.bh * 8 : s.height;
    HIP_TRY(launch(k_jpeg_idct, blocks_for(nblocks, kJpegBlocksPerGroup), kJpegIdctThreads, 0, nullptr, d_in.as<int16_t>() + k.block_offset * 64, d_qt + 64 * c, nblocks, k.bw, dst, dst_stride,
                   dst_rows));
  }
  if (color) {
    JpegChroma g;
    g.cb = d_planes.as<uint8_t>() + plane_off[1];
    g.cr = d_planes.as<uint8_t>() + plane_off[2];
    g.stride = (long long)s.comp[1].bw * 8;
    g.dw = s.comp[1].dw, g.dh = s.comp[1].dh;
    g.hs = s.hmax, g.vs = s.vmax;
    g.fancy = s.hmax == 2 && s.comp[1].dw > 2;
    const int w4 = int(out_stride / 4);
    HIP_TRY(launch(k_jpeg_gray_bgr, blocks_for((long long)w4 * s.height, kJpegColorThreads), kJpegColorThreads, 0, nullptr, d_planes.as<uint8_t>() + plane_off[0],
                   (long long)s.comp[0].bw * 8, g, w4, s.height, d_out.as<uint8_t>(), out_stride));
  }
  HIP_TRY(hipStreamSynchronize(nullptr));
  g_jpeg_clock.lap(2);

  HIP_TRY(hipMemcpy2D(out, size_t(stride), d_out.as<void>(), out_stride, W, H, hipMemcpyDeviceToHost));  // W bytes a row: the caller's padding stays
  g_jpeg_clock.lap(3);
  return NIDREG_OK;
}

int nidreg_jpeg_get_timing(double* ms4) { return g_jpeg_clock.read("nidreg_jpeg_get_timing", ms4); }

}  // extern "C"
