// nid_fold_kernels.hpp -- folds of a device-resident cloud (include/nidreg.h: nidreg_cloud_fold_ids, nidreg_cloud_fold; no counterpart
// in the reference, which has no way to ask how repeatable a calibration is).  The fold of point i is a pure function of
// (seed, cell, num_folds) and of i (cell == 0) or of the cell-metre cube the point lies in (cell > 0): integer arithmetic modulo
// 2^64 apart from the one division that finds the cube, so a numpy restatement gives the same fold for every point.
//   k_fold_flags   one flag byte per point (fold == the wanted one, or != it for the complement); every workgroup counts its tile
//                  of kSelectTile points with wave64 ballots, summed through LDS -- the flag pass of the selection's compaction
//                  (k_select_scan and k_select_scatter follow it unchanged, nidreg_select.hip)
//   k_fold_ids     the fold of every point, and how many points of the workgroup's tiles fall into each fold: per wave and round
//                  one ballot per distinct fold among the wave's 64 points, added by the wave's first lane to the wave's own row
//                  of LDS counters; the rows are summed at the end
//   k_fold_sizes   the workgroups' counts summed per fold, workgroup 0 first
// No atomics: a counter has one writer, and the sums run in a fixed order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nidreg.h"

namespace nidreg {

constexpr int kFoldThreads = 256;  // the selection's geometry (nid_select_kernels.hpp): four waves, four rounds, NIDREG_SELECT_TILE points per tile
constexpr int kFoldWaves = kFoldThreads / 64;
constexpr int kFoldRounds = 4;
constexpr int kFoldTile = kFoldThreads * kFoldRounds;
static_assert(kFoldTile == NIDREG_SELECT_TILE, "k_select_scan / k_select_scatter consume the flags and tile counts of k_fold_flags");
constexpr int kFoldMax = NIDREG_FOLD_MAX;
constexpr int kFoldIdBlocks = 1024;         // workgroups of k_fold_ids at the most: each walks tiles blockIdx.x, blockIdx.x + gridDim.x, ...
constexpr long long kFoldAxisLimit = 1 << 20;  // the integrator's packing (nid_voxel_kernels.hpp vox_classify): 21 bits per axis

__host__ __device__ inline uint64_t fold_mix64(uint64_t z) {  // splitmix64's finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

// the fold of point i (i < n).  pts: n x 4 doubles, read only when cell > 0
__device__ __forceinline__ int fold_of_point(long long i, const double* __restrict__ pts, uint64_t seed, double cell, int num_folds) {
  uint64_t key = uint64_t(i);
  if (cell > 0.0) {
    const double4 p = reinterpret_cast<const double4*>(pts)[i];
    key = (1ULL << 63) | uint64_t(i);  // a point outside the packing is folded on its own
    if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
      const double cx = floor(p.x / cell), cy = floor(p.y / cell), cz = floor(p.z / cell);
      const double L = double(kFoldAxisLimit);
      if (cx >= -L && cx < L && cy >= -L && cy < L && cz >= -L && cz < L)
        key = uint64_t((long long)cx + kFoldAxisLimit) | (uint64_t((long long)cy + kFoldAxisLimit) << 21) | (uint64_t((long long)cz + kFoldAxisLimit) << 42);
    }
  }
  const uint64_t h = fold_mix64(seed + 0x9E3779B97F4A7C15ULL * (key + 1ULL));
  return int(((h >> 32) * uint64_t(num_folds)) >> 32);
}

// tile_count: three arrays of gridDim.x words as k_select_scan reads them -- the tile's flagged points, then two arrays of zeros
__global__ __launch_bounds__(kFoldThreads) void k_fold_flags(
  const double* __restrict__ pts, long long n, uint64_t seed, double cell, int num_folds, int fold, int complement, unsigned char* __restrict__ flag, int* __restrict__ tile_count) {
  __shared__ int s_wave[kFoldWaves];
  const int tid = threadIdx.x, wave = tid >> 6;
  const long long base = (long long)blockIdx.x * kFoldTile;
  int selected = 0;  // (the same in every lane of a wave)
  for (int r = 0; r < kFoldRounds; r++) {
    const long long i = base + r * kFoldThreads + tid;
    const bool f = i < n && ((fold_of_point(i, pts, seed, cell, num_folds) == fold) != (complement != 0));
    if (i < n) flag[i] = f ? 1 : 0;
    selected += __popcll(__ballot(f));
  }
  if ((tid & 63) == 0) s_wave[wave] = selected;
  __syncthreads();
  if (tid < 3) {
    int sum = 0;
    if (tid == 0)
      for (int w = 0; w < kFoldWaves; w++) sum += s_wave[w];
    tile_count[(long long)tid * gridDim.x + blockIdx.x] = sum;
  }
}

// block_count: gridDim.x x num_folds words.  A tile has at most kFoldTile points and a workgroup at most INT_MAX of them: int counters
__global__ __launch_bounds__(kFoldThreads) void k_fold_ids(
  const double* __restrict__ pts, long long n, uint64_t seed, double cell, int num_folds, int32_t* __restrict__ ids, int* __restrict__ block_count) {
  __shared__ int s_cnt[kFoldWaves][kFoldMax];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int k = tid; k < num_folds; k += kFoldThreads)
    for (int w = 0; w < kFoldWaves; w++) s_cnt[w][k] = 0;
  __syncthreads();
  const long long ntiles = (n + kFoldTile - 1) / kFoldTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    for (int r = 0; r < kFoldRounds; r++) {
      const long long i = tile * kFoldTile + r * kFoldThreads + tid;
      int id = -1;
      if (i < n) {
        id = fold_of_point(i, pts, seed, cell, num_folds);
        ids[i] = id;
      }
      // one ballot per distinct fold among the wave's points: at most min(64, num_folds) turns
      unsigned long long todo = __ballot(id >= 0);
      while (todo) {
        const int k = __shfl(id, int(__ffsll((long long)todo)) - 1);
        const unsigned long long same = __ballot(id == k);
        if (lane == 0) s_cnt[wave][k] += __popcll(same);  // this wave's row: one writer
        todo &= ~same;
      }
    }
  }
  __syncthreads();
  for (int k = tid; k < num_folds; k += kFoldThreads) {
    int sum = 0;
    for (int w = 0; w < kFoldWaves; w++) sum += s_cnt[w][k];
    block_count[(long long)blockIdx.x * num_folds + k] = sum;
  }
}

__global__ __launch_bounds__(kFoldThreads) void k_fold_sizes(const int* __restrict__ block_count, int nblocks, int num_folds, long long* __restrict__ sizes) {
  const int k = blockIdx.x * kFoldThreads + threadIdx.x;
  if (k >= num_folds) return;
  long long sum = 0;
  for (int b = 0; b < nblocks; b++) sum += block_count[(long long)b * num_folds + k];
  sizes[k] = sum;
}

}  // namespace nidreg
