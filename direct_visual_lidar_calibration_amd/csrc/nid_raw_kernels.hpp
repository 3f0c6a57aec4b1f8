// nid_raw_kernels.hpp -- raw sensor_msgs/Image encodings to 8-bit gray (include/nidreg.h: nidreg_image_to_mono8; host side:
// nidreg_raw.hip): Bayer mosaics, packed YUV 4:2:2, 8- and 16-bit mono and colour.  Everything is unsigned 32-bit integer
// arithmetic -- the largest sum, 4 * 65535 * 16384 + 2^15, is below 2^32 and above 2^31 --, no kernel uses an atomic or a second
// pass: the outputs equal the numpy restatement (tests/raw_image_oracle.py) bit for bit and are the same bytes from run to run.
//
// SOURCE  the message's bytes as stored: `height` rows of `step` bytes.  step may be odd and a 16-bit row may start at an odd
// address, so every sample is assembled from byte loads; no pointer is ever cast to a wider type.
// OUTPUT  one thread computes 4 adjacent pixels and writes them with ONE 4-byte store: `out` is 4-byte aligned and out_stride a
// multiple of 4 and at least 4 * w4.  The pixels past the image's width in a row's last group are computed from in-bounds samples
// (the column is clamped) and never copied to the caller.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nidreg {

constexpr int kRawThreads = 256;
constexpr uint32_t kLumaR = 4899u, kLumaG = 9617u, kLumaB = 1868u;  // OpenCV's 14-bit luma; they sum to 2^14

// how one pixel lies in a row of a mono, colour or packed-YUV image
struct RawFormat {
  int pixel_bytes;  // bytes from one pixel to the next
  int channels;     // 1: the sample at byte offset r is the gray value; 3: luma of the samples at byte offsets r, g, b
  int r, g, b;      // byte offsets inside the pixel
  int bigendian;    // 16-bit samples only: most significant byte first
};

template <int BYTES>
__device__ __forceinline__ uint32_t raw_sample(const uint8_t* __restrict__ p, int bigendian) {
  if (BYTES == 1) return p[0];
  const uint32_t a = p[0], b = p[1];
  return bigendian ? (a << 8) | b : (b << 8) | a;
}

// cv_bridge's last step, convertTo(CV_8U, 255 / 65535) in float32 with round-half-even, as the integer it equals for every v
__device__ __forceinline__ uint32_t raw_depth8(uint32_t v) { return (v + 128u) / 257u; }

// mono8, mono16, the eight colour encodings, yuv422 (uyvy) and yuv422_yuy2 (yuyv); BYTES = bytes per sample
template <int BYTES>
__global__ __launch_bounds__(kRawThreads) void k_raw_pixels(const uint8_t* __restrict__ src, long long step, RawFormat f, int width, int w4, int height, uint8_t* __restrict__ out,
                                                            long long out_stride) {
  const long long id = (long long)blockIdx.x * kRawThreads + threadIdx.x;
  if (id >= (long long)w4 * height) return;
  const int y = int(id / w4), x0 = int(id % w4) * 4;
  const uint8_t* const row = src + (long long)y * step;
  uint32_t packed = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint8_t* const px = row + (long long)min(x0 + k, width - 1) * f.pixel_bytes;
    uint32_t v = raw_sample<BYTES>(px + f.r, f.bigendian);
    if (f.channels == 3) v = (kLumaR * v + kLumaG * raw_sample<BYTES>(px + f.g, f.bigendian) + kLumaB * raw_sample<BYTES>(px + f.b, f.bigendian) + 8192u) >> 14;
    packed |= (BYTES == 2 ? raw_depth8(v) : v) << (8 * k);
  }
  *reinterpret_cast<uint32_t*>(out + (long long)y * out_stride + x0) = packed;
}

// Bayer mosaics to gray: the bilinear demosaic and the luma with ONE rounding.  (red_x, red_y) is the parity of the red pixels'
// column and row.  A pure gather: every output pixel evaluates the rule at (clamp(x, 1, W - 2), clamp(y, 1, H - 2)) -- a border
// pixel repeats its interior neighbour, and the phase of the pattern is that of the clamped coordinate --, so all 9 taps are
// inside the image (width, height >= 3: the host refuses smaller mosaics).
//   red / blue pixel of colour C, O the other:  (c_C 4p + c_g (l + r + u + d) + c_O (4 diagonals) + 2^15) >> 16
//   green pixel, Ch beside it, Cv above/below:  (c_Ch (l + r) + c_Cv (u + d) + c_g 2p + 2^14) >> 15
template <int BYTES>
__global__ __launch_bounds__(kRawThreads) void k_raw_bayer(const uint8_t* __restrict__ src, long long step, int red_x, int red_y, int bigendian, int width, int w4, int height,
                                                           uint8_t* __restrict__ out, long long out_stride) {
  const long long id = (long long)blockIdx.x * kRawThreads + threadIdx.x;
  if (id >= (long long)w4 * height) return;
  const int y = int(id / w4), x0 = int(id % w4) * 4;
  const int yc = min(max(y, 1), height - 2);
  const uint8_t* const mid = src + (long long)yc * step;
  const uint8_t* const up = mid - step;
  const uint8_t* const down = mid + step;
  const bool red_row = (yc & 1) == red_y;
  uint32_t packed = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int xc = min(max(x0 + k, 1), width - 2);
    const long long o = (long long)xc * BYTES;
    const uint32_t p = raw_sample<BYTES>(mid + o, bigendian);
    const uint32_t lr = raw_sample<BYTES>(mid + o - BYTES, bigendian) + raw_sample<BYTES>(mid + o + BYTES, bigendian);
    const uint32_t ud = raw_sample<BYTES>(up + o, bigendian) + raw_sample<BYTES>(down + o, bigendian);
    const bool red_col = (xc & 1) == red_x;
    uint32_t v;
    if (red_row == red_col) {  // a red pixel (both parities are red's) or a blue one (neither is)
      const uint32_t diag = raw_sample<BYTES>(up + o - BYTES, bigendian) + raw_sample<BYTES>(up + o + BYTES, bigendian) + raw_sample<BYTES>(down + o - BYTES, bigendian) +
                            raw_sample<BYTES>(down + o + BYTES, bigendian);
      const uint32_t c_own = red_row ? kLumaR : kLumaB, c_other = red_row ? kLumaB : kLumaR;
      v = (c_own * 4u * p + kLumaG * (lr + ud) + c_other * diag + 32768u) >> 16;
    } else {  // green: in a red row red lies beside it and blue above and below, in a blue row the other way round
      const uint32_t c_h = red_row ? kLumaR : kLumaB, c_v = red_row ? kLumaB : kLumaR;
      v = (c_h * lr + c_v * ud + kLumaG * 2u * p + 16384u) >> 15;
    }
    packed |= (BYTES == 2 ? raw_depth8(v) : v) << (8 * k);
  }
  *reinterpret_cast<uint32_t*>(out + (long long)y * out_stride + x0) = packed;
}

}  // namespace nidreg
