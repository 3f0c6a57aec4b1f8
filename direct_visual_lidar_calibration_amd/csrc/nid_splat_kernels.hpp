// nid_splat_kernels.hpp -- a z-buffered point-splat renderer: what turns the colours of k_colorize (or any RGBA8 per point) into a
// picture without a GUI.  The reference draws its viewer (src/viewer.cpp, VisualLiDARVisualizer) through OpenGL; here every point is
// a (2r+1)^2 square of pixels, depth-tested, seen through any of the camera models:
//   k_splat_depth     per point: the front end of k_colorize / k_lidar_zmin (point_to_pixel: transform, FoV gate on the normalised
//                     3-vector, projection, truncating cast, in-image test), then ONE 64-bit atomicMin per covered pixel of
//                         key = (bits(float(squared distance)) << 32) | (0xFFFFFFFF - index)
//                     so the nearest point wins and, among points of equal float32 depth, the LARGEST index -- the tie direction
//                     generate_lidar_image ends with (nid_render_kernels.hpp).  A point whose centre is outside the image (q < 0)
//                     draws nothing, even where its square would reach in; a non-finite depth draws nothing.
//   k_splat_resolve   per pixel: the winner's colour over the background, in integers.
// One packed key gives ONE pass over the points: the zmin / argmax scheme of k_lidar_* needs two, which would double the atomic
// traffic -- (2r+1)^2 per point here.  The price is a float32 depth: two squared distances that differ in fp64 and round to the same
// float32 are equals, and the larger index wins even when it is the farther one in fp64.  That is enough for a picture (the relative
// step is 6e-8) and it is NOT what generate_lidar_image computes, which stays on its fp64 two-pass route.
// No floating point follows the depth key, so the picture is bit-reproducible and restated exactly in tests/viewer_oracle.py.
// Compiled with -ffp-contract=off and the exact-order projection, like nid_kernels_f64_exact.hip: pixel assignments equal the CPU's.
#pragma once
#include "nid_render_kernels.hpp"

namespace nidreg {

constexpr int kSplatMaxRadius = 8;
constexpr u64 kSplatEmpty = ~0ull;  // above every key: the depth field of a key is that of a finite float, below 0x7F800000

template <int MODEL>
__global__ __launch_bounds__(256) void k_splat_depth(
  const double* __restrict__ pts, long long stride_d, long long n, IsoParams<double> iso, CamParams<double> cam, int W, int H, double min_nz, int radius, u64* __restrict__ zkey) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* p = pts + i * stride_d;
  double cx, cy, cz;
  const int q = point_to_pixel<MODEL>(iso, cam, p[0], p[1], p[2], p[3], W, H, min_nz, cx, cy, cz);
  if (q < 0) return;
  const double sq = (cx * cx + cy * cy) + cz * cz;
  const float d = float(sq);  // round to nearest; sq >= 0, so the bit pattern of d is monotone
  if (!(d <= 3.402823466e+38f)) return;  // inf (sq beyond float) or NaN
  const u64 key = (u64(__float_as_uint(d)) << 32) | u64(0xFFFFFFFFu - uint32_t(i));
  const int px = q % W, py = q / W;
  const int x0 = max(px - radius, 0), x1 = min(px + radius, W - 1);
  const int y0 = max(py - radius, 0), y1 = min(py + radius, H - 1);
  for (int y = y0; y <= y1; y++) {
    u64* row = zkey + (long long)y * W;
    for (int x = x0; x <= x1; x++) {
      // keys only ever fall: a (possibly stale) value at or below ours means ours cannot win, and the atomic is saved
      if (row[x] > key) atomicMin(&row[x], key);
    }
  }
}

// rgba: 4 bytes per point; background: W * 3 bytes a row, or null (black); out_index nullable
__global__ __launch_bounds__(256) void k_splat_resolve(
  const u64* __restrict__ zkey, long long npix, const uchar4* __restrict__ rgba, const uint8_t* __restrict__ background, int alpha, uint8_t* __restrict__ out_rgb,
  int* __restrict__ out_index) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= npix) return;
  int b0 = 0, b1 = 0, b2 = 0;
  if (background) b0 = background[3 * q], b1 = background[3 * q + 1], b2 = background[3 * q + 2];
  const u64 key = zkey[q];
  int index = -1;
  if (key != kSplatEmpty) {
    index = int(0xFFFFFFFFu - uint32_t(key));
    const uchar4 c = rgba[index];
    const int a = (alpha * int(c.w) + 127) / 255;
    b0 = (b0 * (255 - a) + int(c.x) * a + 127) / 255;
    b1 = (b1 * (255 - a) + int(c.y) * a + 127) / 255;
    b2 = (b2 * (255 - a) + int(c.z) * a + 127) / 255;
  }
  out_rgb[3 * q] = uint8_t(b0), out_rgb[3 * q + 1] = uint8_t(b1), out_rgb[3 * q + 2] = uint8_t(b2);
  if (out_index) out_index[q] = index;
}

}  // namespace nidreg
