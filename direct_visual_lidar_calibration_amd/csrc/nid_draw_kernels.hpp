// nid_draw_kernels.hpp -- a 2-D primitive rasteriser: what draws the match picture of find_matches (the reference's
// <bag>_superglue.png, scripts/find_matches_superglue.py) and the residual picture of initial_guess_auto without OpenCV.
//   k_draw_prims     one wave per primitive, lanes striding over its steps (a line's k = 0..n, a ring's / disc's bounding square):
//                    a returnless 32-bit atomicMax(owner[pixel], index + 1) for every covered pixel INSIDE the canvas.  The owner
//                    words are zeroed before (hipMemsetAsync), so 0 = bare canvas and the primitive of the LARGEST index wins a
//                    pixel on every run, whatever the order the waves run in: the painter's rule of drawing them one after another.
//   k_draw_compose   per pixel: the canvas (left image; the right one resized beside it by exact integer bilinear interpolation)
//                    or, where a primitive owns the pixel, its colour.
// Integers only -- no floating point, no 64-bit and no float atomics -- so the picture is bit-reproducible and restated exactly in
// tests/draw_oracle.py.  The rules (include/nidreg.h, nidreg_draw, states them for the caller):
//   LINE  n = max(|dx|, |dy|); for k = 0..n the pixel (x0 + sgn(dx) ((2 k |dx| + n) / (2 n)), y0 + sgn(dy) ((2 k |dy| + n) / (2 n))): the
//         parallel DDA, every k on its own, defined FROM the first point (the pixel set of the reversed line may differ).  2 k |dx|
//         reaches 2^33 at the coordinate bound: 64-bit.
//   RING  4 d2 < (2 a + 1)^2 and (a == 0 or 4 d2 >= (2 a - 1)^2), d2 = dx^2 + dy^2;  DISC  4 d2 < (2 a + 1)^2.
//   resize  per axis, destination i of n_d from n_s: num = (2 i + 1) n_s - n_d, den = 2 n_d, i0 = floor(num / den), f = num - i0 den,
//         taps i0 and i0 + 1 clamped to [0, n_s - 1]; value (sum of taps x weights + den_x den_y / 2) / (den_x den_y) in 64 bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nidreg {

constexpr int kDrawLine = 0, kDrawRing = 1, kDrawDisc = 2;
constexpr int kDrawWords = 8;        // int32 per primitive: kind, x0, y0, a, b, rgb, 0, 0
constexpr int kDrawMaxRadius = 16;
constexpr int kDrawMaxDim = 16384;
constexpr int kDrawCoordMin = -32768, kDrawCoordMax = 32767;
constexpr long long kDrawMaxPrims = 1ll << 24;
constexpr int kDrawWave = 64;        // threads of k_draw_prims' workgroup: one wave, one primitive
constexpr int kDrawThreads = 256;    // k_draw_compose

__device__ __forceinline__ void draw_claim(uint32_t* __restrict__ owner, int cw, int ch, int x, int y, uint32_t tag) {
  if (x < 0 || y < 0 || x >= cw || y >= ch) return;  // dropped pixel by pixel, not per primitive
  atomicMax(owner + ((long long)y * cw + x), tag);    // (result unused: returnless)
}

// grid: one workgroup of kDrawWave threads per primitive (at most 2^24 of them), blockIdx.x its index
__global__ __launch_bounds__(kDrawWave) void k_draw_prims(const int32_t* __restrict__ prims, int cw, int ch, uint32_t* __restrict__ owner) {
  const long long p = blockIdx.x;
  const int32_t* r = prims + p * kDrawWords;
  const int kind = r[0], x0 = r[1], y0 = r[2], a = r[3], b = r[4];
  const uint32_t tag = uint32_t(p) + 1u;
  const int lane = threadIdx.x;
  if (kind == kDrawLine) {
    const int dx = a - x0, dy = b - y0;
    const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
    const int sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1;
    const int n = adx > ady ? adx : ady;
    if (n == 0) {
      if (lane == 0) draw_claim(owner, cw, ch, x0, y0, tag);
      return;
    }
    const unsigned long long n2 = 2ull * (unsigned long long)n;
    for (int k = lane; k <= n; k += kDrawWave) {
      const unsigned long long k2 = 2ull * (unsigned long long)k;
      const int qx = int((k2 * (unsigned long long)adx + (unsigned long long)n) / n2);
      const int qy = int((k2 * (unsigned long long)ady + (unsigned long long)n) / n2);
      draw_claim(owner, cw, ch, x0 + sx * qx, y0 + sy * qy, tag);
    }
    return;
  }
  // RING / DISC over the bounding square of side 2 a + 1
  const int side = 2 * a + 1;
  const int outer = side * side;                     // (2 a + 1)^2
  const int inner = (2 * a - 1) * (2 * a - 1);       // (2 a - 1)^2
  for (int c = lane; c < side * side; c += kDrawWave) {
    const int ox = c % side - a, oy = c / side - a;
    const int d4 = 4 * (ox * ox + oy * oy);
    if (d4 >= outer) continue;
    if (kind == kDrawRing && a != 0 && d4 < inner) continue;
    draw_claim(owner, cw, ch, x0 + ox, y0 + oy, tag);
  }
}

// the two taps and the weight of the second along one axis (header comment: resize)
__device__ __forceinline__ void draw_taps(int i, int n_d, int n_s, int& t0, int& t1, int& f) {
  const int num = (2 * i + 1) * n_s - n_d, den = 2 * n_d;  // |num| < 2^30 at the 16384 bound
  int i0 = num / den;
  if (num - i0 * den < 0) i0--;  // floor
  f = num - i0 * den;
  t0 = min(max(i0, 0), n_s - 1);
  t1 = min(max(i0 + 1, 0), n_s - 1);
}

// left: lw x lh (device copy, packed); right (nullable): rw x rh packed; out: lh x cw x 3, cw = lw or 2 lw
__global__ __launch_bounds__(kDrawThreads) void k_draw_compose(const uint8_t* __restrict__ left, int lw, int lh, const uint8_t* __restrict__ right, int rw, int rh, int cw,
                                                               const uint32_t* __restrict__ owner, const int32_t* __restrict__ prims, uint8_t* __restrict__ out) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (long long)cw * lh) return;
  const int x = int(q % cw), y = int(q / cw);
  uint8_t* o = out + 3 * q;
  const uint32_t tag = owner[q];
  if (tag) {
    const uint32_t rgb = uint32_t(prims[(long long)(tag - 1u) * kDrawWords + 5]);
    o[0] = uint8_t(rgb >> 16), o[1] = uint8_t(rgb >> 8), o[2] = uint8_t(rgb);
    return;
  }
  int v;
  if (x < lw) {
    v = left[(long long)y * lw + x];
  } else {
    int xa, xb, fx, ya, yb, fy;
    draw_taps(x - lw, lw, rw, xa, xb, fx);
    draw_taps(y, lh, rh, ya, yb, fy);
    const long long dx = 2ll * lw, dy = 2ll * lh;
    const uint8_t* ra = right + (long long)ya * rw;
    const uint8_t* rb = right + (long long)yb * rw;
    const long long top = (long long)ra[xa] * (dx - fx) + (long long)ra[xb] * fx;
    const long long bot = (long long)rb[xa] * (dx - fx) + (long long)rb[xb] * fx;
    v = int((top * (dy - fy) + bot * fy + dx * dy / 2) / (dx * dy));
  }
  o[0] = o[1] = o[2] = uint8_t(v);
}

}  // namespace nidreg
