// nid_select_kernels.hpp -- masks and range gates on a device-resident cloud (include/nidreg.h: nidreg_mask_create, nidreg_cloud_select;
// no counterpart in the reference, whose users edit the PNG or the PLY by hand).  A point is SELECTED iff
//   keep[i]                       ViewCulling::cull kept it (nid_cull_kernels.hpp, launched unchanged), and
//   eroded[pix[i]] != 0           the eroded mask is valid at the pixel k_cull_zbuf stored for it (no mask: always), and
//   min2 <= r2 <= max2            r2 = (x x + y y) + z z of the cloud's own LiDAR-frame coordinates, fp64, no contraction
// and the selected points are gathered, in input order, into a new cloud.  Four kernels:
//   k_mask_erode      minimum over 2R+1 bytes along one axis, window clipped to the image (outside counts as valid); run twice
//                     (rows, then columns) per mask, once, at creation
//   k_select_flags    one flag byte per point; every workgroup counts its tile of kSelectTile points: wave64 ballot + popcount
//                     per wave and round, summed through LDS (and, for the log, the points the cull kept and the mask removed)
//   k_select_scan     exclusive scan of the tile counts by ONE workgroup, kSelectThreads tiles per step with a carry, fixed order
//   k_select_scatter  rank = tile offset + selected points of the earlier (round, wave) slots of the tile (LDS) + set ballot bits
//                     below the lane (mbcnt); writes the int32 index, the 32-byte point and the 8-byte intensity
// No atomics and no workgroup waits for another: the launches are the synchronisation, and the result is the same bytes every run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nidreg.h"

namespace nidreg {

constexpr int kSelectThreads = 256;                              // four waves
constexpr int kSelectWaves = kSelectThreads / 64;
constexpr int kSelectRounds = 4;                                 // a thread visits one point per round: point = tile * kSelectTile + round * kSelectThreads + thread
constexpr int kSelectTile = kSelectThreads * kSelectRounds;      // points per workgroup
static_assert(kSelectTile == NIDREG_SELECT_TILE, "nidreg.h documents the tile of the compaction (tests size their clouds by it)");

// dst[y][x] = min of src over [x - R, x + R] (horizontal != 0) or [y - R, y + R] (horizontal == 0), clipped to the image.
// Both images are W x H bytes, rows W apart.
__global__ __launch_bounds__(256) void k_mask_erode(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int W, int H, int R, int horizontal) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)W * H) return;
  const int y = int(i / W), x = int(i - (long long)y * W);
  unsigned int m = 255u;
  if (horizontal) {
    const int lo = x - R < 0 ? 0 : x - R, hi = x + R > W - 1 ? W - 1 : x + R;
    const uint8_t* row = src + (long long)y * W;
    for (int k = lo; k <= hi; k++) m = min(m, (unsigned int)row[k]);
  } else {
    const int lo = y - R < 0 ? 0 : y - R, hi = y + R > H - 1 ? H - 1 : y + R;
    for (int k = lo; k <= hi; k++) m = min(m, (unsigned int)src[(long long)k * W + x]);
  }
  dst[i] = uint8_t(m);
}

// the selection rule for point i (i < n): what became of it.  pix[i] lies in [0, W * H) wherever keep[i] is set (k_cull_zbuf's in-image test)
enum : int { kSelCulled = 0, kSelMasked = 1, kSelRanged = 2, kSelSelected = 3 };
__device__ __forceinline__ int select_point(
  long long i, const unsigned char* __restrict__ keep, const int* __restrict__ pix, const uint8_t* __restrict__ eroded, const double* __restrict__ pts, double min2, double max2) {
  if (!keep[i]) return kSelCulled;
  if (eroded && eroded[pix[i]] == 0) return kSelMasked;
  const double* p = pts + 4 * i;
  const double x = p[0], y = p[1], z = p[2];
  const double r2 = (x * x + y * y) + z * z;
  return (r2 >= min2 && r2 <= max2) ? kSelSelected : kSelRanged;
}

// tile_count: three arrays of gridDim.x words -- the tile's selected points, the points the cull kept, and those of them the mask removed
__global__ __launch_bounds__(kSelectThreads) void k_select_flags(
  const unsigned char* __restrict__ keep, const int* __restrict__ pix, const uint8_t* __restrict__ eroded, const double* __restrict__ pts, long long n, double min2, double max2,
  unsigned char* __restrict__ flag, int* __restrict__ tile_count) {
  __shared__ int s_wave[3][kSelectWaves];
  const int tid = threadIdx.x, wave = tid >> 6;
  const long long base = (long long)blockIdx.x * kSelectTile;
  int selected = 0, kept = 0, masked = 0;  // (the same in every lane of a wave)
  for (int r = 0; r < kSelectRounds; r++) {
    const long long i = base + r * kSelectThreads + tid;
    const int what = i < n ? select_point(i, keep, pix, eroded, pts, min2, max2) : kSelCulled;
    if (i < n) flag[i] = what == kSelSelected ? 1 : 0;
    selected += __popcll(__ballot(what == kSelSelected));
    kept += __popcll(__ballot(what != kSelCulled));
    masked += __popcll(__ballot(what == kSelMasked));
  }
  if ((tid & 63) == 0) s_wave[0][wave] = selected, s_wave[1][wave] = kept, s_wave[2][wave] = masked;
  __syncthreads();
  if (tid < 3) {
    int sum = 0;
    for (int w = 0; w < kSelectWaves; w++) sum += s_wave[tid][w];
    tile_count[(long long)tid * gridDim.x + blockIdx.x] = sum;
  }
}

// offset[t] = count[0] + ... + count[t - 1] for t in [0, ntiles], so offset[ntiles] is the number of selected points; offset[ntiles + 1]
// and [ntiles + 2] receive the plain sums of the second and third array of k_select_flags' counts.  ONE workgroup, kSelectThreads
// tiles per step, the carry handed from step to step: a fixed order whatever the number of tiles.
__global__ __launch_bounds__(kSelectThreads) void k_select_scan(const int* __restrict__ count, int ntiles, int* __restrict__ offset) {
  __shared__ int s_wave[3][kSelectWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry[3] = {0, 0, 0};  // (the same in every thread)
  for (int base = 0; base < ntiles; base += kSelectThreads) {
    const int t = base + tid;
    int v[3], incl[3];
    for (int k = 0; k < 3; k++) {
      v[k] = t < ntiles ? count[(long long)k * ntiles + t] : 0;
      incl[k] = v[k];  // inclusive scan inside the wave
      for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl[k], d);
        if (lane >= d) incl[k] += up;
      }
      if (lane == 63) s_wave[k][wave] = incl[k];
    }
    __syncthreads();
    int before = 0;  // the selected points of this step's earlier waves
    for (int w = 0; w < wave; w++) before += s_wave[0][w];
    if (t < ntiles) offset[t] = carry[0] + before + (incl[0] - v[0]);
    for (int k = 0; k < 3; k++)
      for (int w = 0; w < kSelectWaves; w++) carry[k] += s_wave[k][w];
    __syncthreads();  // s_wave is rewritten by the next step
  }
  if (tid < 3) offset[ntiles + tid] = carry[tid];
}

__global__ __launch_bounds__(kSelectThreads) void k_select_scatter(
  const unsigned char* __restrict__ flag, const int* __restrict__ tile_offset, const double* __restrict__ pts, const double* __restrict__ intensities, long long n,
  int32_t* __restrict__ idx_out, double* __restrict__ pts_out, double* __restrict__ int_out) {
  __shared__ int s_cnt[kSelectRounds * kSelectWaves];
  const int tid = threadIdx.x, wave = tid >> 6;
  const long long base = (long long)blockIdx.x * kSelectTile;
  bool f[kSelectRounds];
  int below[kSelectRounds];
#pragma unroll
  for (int r = 0; r < kSelectRounds; r++) {
    const long long i = base + r * kSelectThreads + tid;
    f[r] = i < n && flag[i] != 0;
    const unsigned long long bits = __ballot(f[r]);
    below[r] = int(__builtin_amdgcn_mbcnt_hi((unsigned int)(bits >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)bits, 0u)));  // set bits below this lane
    if ((tid & 63) == 0) s_cnt[r * kSelectWaves + wave] = __popcll(bits);
  }
  __syncthreads();
  int slot_base = tile_offset[blockIdx.x];
#pragma unroll
  for (int r = 0; r < kSelectRounds; r++) {
    int before = 0;
    for (int w = 0; w < kSelectWaves; w++) {
      const int c = s_cnt[r * kSelectWaves + w];
      if (w < wave) before += c;
    }
    if (f[r]) {
      const long long i = base + r * kSelectThreads + tid;
      const long long o = (long long)slot_base + before + below[r];
      if (idx_out) idx_out[o] = int32_t(i);
      const double4 p = reinterpret_cast<const double4*>(pts)[i];
      reinterpret_cast<double4*>(pts_out)[o] = p;
      int_out[o] = intensities[i];
    }
    for (int w = 0; w < kSelectWaves; w++) slot_base += s_cnt[r * kSelectWaves + w];
  }
}

}  // namespace nidreg
