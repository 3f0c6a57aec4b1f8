// nid_jpeg_kernels.hpp -- the arithmetic half of the baseline JPEG decoder (include/nidreg.h: nidreg_jpeg_decode_gray; host side:
// nidreg_jpeg.hip, entropy decode: nid_jpeg_host.hpp): dequantisation, inverse DCT, chroma upsampling, YCbCr -> RGB and luma.
// Everything is integer arithmetic (int32, two's complement, wrapping) and no kernel uses an atomic: the outputs equal the numpy
// restatement (tests/jpeg_oracle.py) bit for bit and are the same bytes from run to run.
//
// The inverse DCT is libjpeg's jpeg_idct_islow (jidctint.c: CONST_BITS 13, PASS1_BITS 2; the column pass descales by 11, the row
// pass by 18, then 128 is added).  RANGE LIMIT: the result SATURATES to [0, 255], which is what the SIMD builds of libjpeg-turbo
// (every x86 OpenCV and Pillow) do; libjpeg's C table wraps modulo 1024 beyond +-512 instead.  Where the dequantised coefficients
// or the column pass's outputs leave int16, the SIMD code's 16-bit intermediates no longer hold what the C code's 32-bit ones do;
// there this decoder's result (int32 all the way) is its own and pinned to neither.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nidreg {

constexpr int kJpegIdctThreads = 64;  // one wave: 8 blocks, thread t = column (then row) t % 8 of block t / 8
constexpr int kJpegBlocksPerGroup = 8;
// LDS workspace: element (row r, column c) of block b at b * 72 + r * 9 + c.  The column pass writes, per r, bank (8 b + c + 9 r) % 32
// from lanes (b, c): 32 different banks per 32 lanes; the row pass reads, per c, bank (9 (8 b + r) + c) % 32 from lanes (b, r): 9 is
// odd, so again 32 different banks.  Neither pass conflicts.
constexpr int kJpegRowStride = 9, kJpegBlockStride = 72;
constexpr int kJpegColorThreads = 256;

typedef unsigned int jpeg_u32;

// one 8-point pass of jpeg_idct_islow, before the descale.  Unsigned arithmetic: wrapping, the int32 bits of the C code
__device__ __forceinline__ void jpeg_idct_pass(const jpeg_u32 in[8], jpeg_u32 out[8]) {
  jpeg_u32 z2 = in[2], z3 = in[6];
  jpeg_u32 z1 = (z2 + z3) * 4433u;
  jpeg_u32 tmp2 = z1 - z3 * 15137u;
  jpeg_u32 tmp3 = z1 + z2 * 6270u;
  z2 = in[0], z3 = in[4];
  jpeg_u32 tmp0 = (z2 + z3) << 13;
  jpeg_u32 tmp1 = (z2 - z3) << 13;
  const jpeg_u32 tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7], tmp1 = in[5], tmp2 = in[3], tmp3 = in[1];
  z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
  jpeg_u32 z4 = tmp1 + tmp3;
  const jpeg_u32 z5 = (z3 + z4) * 9633u;
  tmp0 *= 2446u, tmp1 *= 16819u, tmp2 *= 25172u, tmp3 *= 12299u;
  z1 *= jpeg_u32(-7373), z2 *= jpeg_u32(-20995), z3 *= jpeg_u32(-16069), z4 *= jpeg_u32(-3196);
  z3 += z5, z4 += z5;
  tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
  out[0] = tmp10 + tmp3, out[7] = tmp10 - tmp3;
  out[1] = tmp11 + tmp2, out[6] = tmp11 - tmp2;
  out[2] = tmp12 + tmp1, out[5] = tmp12 - tmp1;
  out[3] = tmp13 + tmp0, out[4] = tmp13 - tmp0;
}

__device__ __forceinline__ int jpeg_descale(jpeg_u32 v, int n) { return int(v + (1u << (n - 1))) >> n; }
__device__ __forceinline__ int jpeg_clamp(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Dequantise and inverse-transform `nblocks` blocks of one component (raster order over a grid `bw` blocks wide) into an 8-bit plane.
// A block row is ONE 8-byte store at out + y * out_stride + 8 bx: out is 8-byte aligned and out_stride a multiple of 8.  Rows from
// out_rows on and blocks that start at or right of out_stride are not stored: the component planes hold the whole grid, the Y plane
// of the LUMA mode is the cropped image itself (its stride rounded up to 8).
__global__ __launch_bounds__(kJpegIdctThreads) void k_jpeg_idct(const int16_t* __restrict__ coef, const uint16_t* __restrict__ qt, long long nblocks, int bw,
                                                                uint8_t* __restrict__ out, long long out_stride, int out_rows) {
  __shared__ int ws[kJpegBlocksPerGroup * kJpegBlockStride];
  __shared__ uint16_t sq[64];
  const int t = int(threadIdx.x), blk = t >> 3, c = t & 7;
  const long long b = (long long)blockIdx.x * kJpegBlocksPerGroup + blk;
  const bool live = b < nblocks;  // the tail group: its spare threads keep to the barriers and touch no memory
  sq[t] = qt[t];
  __syncthreads();
  jpeg_u32 in[8], o[8];
#pragma unroll
  for (int r = 0; r < 8; r++) in[r] = live ? jpeg_u32(int(coef[b * 64 + r * 8 + c])) * jpeg_u32(sq[r * 8 + c]) : 0u;
  jpeg_idct_pass(in, o);
#pragma unroll
  for (int r = 0; r < 8; r++) ws[blk * kJpegBlockStride + r * kJpegRowStride + c] = jpeg_descale(o[r], 11);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; k++) in[k] = jpeg_u32(ws[blk * kJpegBlockStride + c * kJpegRowStride + k]);
  jpeg_idct_pass(in, o);
  jpeg_u32 lo = 0, hi = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    lo |= jpeg_u32(jpeg_clamp(jpeg_descale(o[k], 18) + 128)) << (8 * k);
    hi |= jpeg_u32(jpeg_clamp(jpeg_descale(o[k + 4], 18) + 128)) << (8 * k);
  }
  if (!live) return;
  const long long x0 = (b % bw) * 8, y = (b / bw) * 8 + c;
  if (x0 >= out_stride || y >= out_rows) return;
  *reinterpret_cast<uint2*>(out + y * out_stride + x0) = make_uint2(lo, hi);
}

// the downsampled chroma planes and how they relate to the image
struct JpegChroma {
  const uint8_t* cb;
  const uint8_t* cr;
  long long stride;  // bytes a row (the component's whole block grid)
  int dw, dh;        // the component's downsampled size: the edges of the upsampling
  int hs, vs;        // 1 or 2: luma samples per chroma sample
  int fancy;         // libjpeg-turbo: triangle-filter upsampling only when dw > 2, else replication (uniform per launch)
};

// One upsampled chroma sample at image position (x, y), computed from the downsampled plane (libjpeg's jdsample.c):
//   h2v1 fancy: out[2i] = (3 in[i] + in[i-1] + 1) >> 2, out[2i+1] = (3 in[i] + in[i+1] + 2) >> 2;
//   h2v2 fancy: col[j] = 3 near[j] + far[j] (far: the row above for an even output row, below for an odd one),
//               out[2i] = (3 col[i] + col[i-1] + 8) >> 4, out[2i+1] = (3 col[i] + col[i+1] + 7) >> 4;
// neighbours beyond the component's downsampled size are the edge sample.
__device__ __forceinline__ int jpeg_chroma_at(const uint8_t* __restrict__ p, const JpegChroma& g, int x, int y) {
  if (g.hs == 1) return p[(long long)y * g.stride + x];
  const int i = min(x >> 1, g.dw - 1);
  const int r = g.vs == 2 ? (y >> 1) : y;
  const uint8_t* near = p + (long long)r * g.stride;
  if (!g.fancy) return near[i];
  const int j = (x & 1) ? min(i + 1, g.dw - 1) : max(i - 1, 0);
  if (g.vs == 1) return (3 * int(near[i]) + int(near[j]) + ((x & 1) ? 2 : 1)) >> 2;
  const int rf = (y & 1) ? min(r + 1, g.dh - 1) : max(r - 1, 0);
  const uint8_t* far = p + (long long)rf * g.stride;
  const int ci = 3 * int(near[i]) + int(far[i]), cj = 3 * int(near[j]) + int(far[j]);
  return (3 * ci + cj + ((x & 1) ? 7 : 8)) >> 4;
}

// The cv_bridge route: YCbCr -> RGB with libjpeg's 16-bit tables (jdcolor.c), each channel range-limited, then OpenCV's fixed-point
// luma (4899 R + 9617 G + 1868 B + 8192) >> 14.  One thread per 4 adjacent pixels, one 4-byte store: ystride and out_stride are
// multiples of 4 and at least 4 * w4; the pixels past the image's width in the last group are computed from in-bounds samples and
// never copied to the caller.
__global__ __launch_bounds__(kJpegColorThreads) void k_jpeg_gray_bgr(const uint8_t* __restrict__ yplane, long long ystride, JpegChroma g, int w4, int height,
                                                                     uint8_t* __restrict__ out, long long out_stride) {
  const long long id = (long long)blockIdx.x * kJpegColorThreads + threadIdx.x;
  if (id >= (long long)w4 * height) return;
  const int y = int(id / w4), x0 = int(id % w4) * 4;
  const jpeg_u32 y4 = *reinterpret_cast<const jpeg_u32*>(yplane + (long long)y * ystride + x0);
  jpeg_u32 packed = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int Y = int((y4 >> (8 * k)) & 255u);
    const int cb = jpeg_chroma_at(g.cb, g, x0 + k, y) - 128, cr = jpeg_chroma_at(g.cr, g, x0 + k, y) - 128;
    const int R = jpeg_clamp(Y + ((91881 * cr + 32768) >> 16));
    const int B = jpeg_clamp(Y + ((116130 * cb + 32768) >> 16));
    const int G = jpeg_clamp(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    packed |= jpeg_u32((4899 * R + 9617 * G + 1868 * B + 8192) >> 14) << (8 * k);
  }
  *reinterpret_cast<jpeg_u32*>(out + (long long)y * out_stride + x0) = packed;
}

}  // namespace nidreg
