// nid_match_kernels.hpp -- keypoints and descriptor matching for find_matches (include/nidreg.h: nidreg_features_detect,
// nidreg_features_match; host side: nidreg_match.hip).  A classical stand-in for the reference's SuperGlue script
// (scripts/find_matches_superglue.py), NOT a port of it: FAST-9 corners over a 6/5 image pyramid, upright BRIEF-256 descriptors,
// mutual-best Hamming matching with a ratio test.  Everything is integer arithmetic on 8-bit pixels: the results equal the numpy
// restatement (tests/matching_oracle.py) bit for bit, and no kernel uses an atomic: every output has the same bytes from run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nid_brief_table.hpp"

namespace nidreg {

typedef unsigned long long match_u64;

constexpr int kFeatBorder = 16;      // per level: no keypoint closer than this to the level's edge (the descriptor's reach + 1)
constexpr int kFeatMaxLevels = 16;   // levels the key's level field and the 64-bit level-to-zero mapping are sized for
constexpr int kFeatMaxDim = 32768;   // width / height: x and y have 16 bits each in the key
constexpr int kFeatMaxRadius = 16;   // non-maximum suppression window radius
constexpr int kFeatTileW = 32, kFeatTileH = 8;  // FAST tile: 256 threads, (32 + 6) x (8 + 6) bytes of LDS
constexpr int kFeatThreads = 256;
constexpr int kMatchThreads = 64;    // one wave: one row descriptor per lane
constexpr int kMatchTile = 256;      // column descriptors per LDS tile: 8 KB
constexpr int kHammingNone = 257;    // "no such column": above every distance of 256-bit descriptors
constexpr match_u64 kFeatNoKey = ~0ULL;  // a pixel that is no keypoint: sorts behind every key

// the pyramid and what maps a level's pixel to level 0: x0 = ((2 x + 1) 6^l) / (2 5^l), clamped
struct FeatLevels {
  const uint8_t* smooth[kFeatMaxLevels];
  int w[kFeatMaxLevels], h[kFeatMaxLevels];
  match_u64 num[kFeatMaxLevels], den[kFeatMaxLevels];  // 6^l, 2 5^l
  int W0, H0;
};

__device__ const signed char kBriefTable[4 * kBriefPairs] = {NID_BRIEF_TABLE_VALUES};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- hole filling of the level-0 image (one pass; the host ping-pongs two image / mask pairs): an invalid pixel with a valid
// 3x3 neighbour becomes the mean of its valid neighbours, rounded half up, and valid
__global__ __launch_bounds__(kFeatThreads) void k_fill_pass(const uint8_t* __restrict__ img_in, const uint8_t* __restrict__ mask_in, uint8_t* __restrict__ img_out,
                                                            uint8_t* __restrict__ mask_out, int w, int h) {
  const int x = int(blockIdx.x) * kFeatTileW + int(threadIdx.x % kFeatTileW), y = int(blockIdx.y) * kFeatTileH + int(threadIdx.x / kFeatTileW);
  if (x >= w || y >= h) return;
  const size_t p = size_t(y) * size_t(w) + size_t(x);
  uint8_t v = img_in[p], m = mask_in[p];
  if (!m) {
    int sum = 0, cnt = 0;
    for (int dy = -1; dy <= 1; dy++)
      for (int dx = -1; dx <= 1; dx++) {
        const int xx = x + dx, yy = y + dy;
        if (xx < 0 || yy < 0 || xx >= w || yy >= h) continue;
        const size_t q = size_t(yy) * size_t(w) + size_t(xx);
        if (mask_in[q]) sum += img_in[q], cnt++;
      }
    if (cnt > 0) v = uint8_t((sum + cnt / 2) / cnt), m = 1;
  }
  img_out[p] = v, mask_out[p] = m;
}

// ---- level l + 1 from level l at ratio 6/5: destination centre x sits at source coordinate (12 x + 1) / 10, so the bilinear
// weights are tenths and the four taps combine as (sum + 50) / 100; taps beyond the source are clamped
__global__ __launch_bounds__(kFeatThreads) void k_pyr_down(const uint8_t* __restrict__ src, int sw, int sh, uint8_t* __restrict__ dst, int dw, int dh) {
  const int x = int(blockIdx.x) * kFeatTileW + int(threadIdx.x % kFeatTileW), y = int(blockIdx.y) * kFeatTileH + int(threadIdx.x / kFeatTileW);
  if (x >= dw || y >= dh) return;
  const int cx = 12 * x + 1, cy = 12 * y + 1;
  const int x0 = cx / 10, fx = cx % 10, y0 = cy / 10, fy = cy % 10;
  const int x1 = x0 + 1 < sw ? x0 + 1 : sw - 1, y1 = y0 + 1 < sh ? y0 + 1 : sh - 1;
  const int xa = x0 < sw ? x0 : sw - 1, ya = y0 < sh ? y0 : sh - 1;
  const uint8_t* r0 = src + size_t(ya) * size_t(sw);
  const uint8_t* r1 = src + size_t(y1) * size_t(sw);
  const int top = (10 - fx) * int(r0[xa]) + fx * int(r0[x1]);
  const int bot = (10 - fx) * int(r1[xa]) + fx * int(r1[x1]);
  dst[size_t(y) * size_t(dw) + size_t(x)] = uint8_t(((10 - fy) * top + fy * bot + 50) / 100);
}

// ---- the smoothed copy the descriptors read: the separable binomial [1 4 6 4 1] along x and along y -- the 5 x 5 kernel of weight
// 256 --, rounded once: (sum + 128) >> 8; borders replicate
__global__ __launch_bounds__(kFeatThreads) void k_smooth(const uint8_t* __restrict__ src, int w, int h, uint8_t* __restrict__ dst) {
  const int x = int(blockIdx.x) * kFeatTileW + int(threadIdx.x % kFeatTileW), y = int(blockIdx.y) * kFeatTileH + int(threadIdx.x / kFeatTileW);
  if (x >= w || y >= h) return;
  const int wt[5] = {1, 4, 6, 4, 1};
  int sum = 0;
#pragma unroll
  for (int j = 0; j < 5; j++) {
    const uint8_t* row = src + size_t(clampi(y + j - 2, 0, h - 1)) * size_t(w);
    int rs = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) rs += wt[i] * int(row[clampi(x + i - 2, 0, w - 1)]);
    sum += wt[j] * rs;
  }
  dst[size_t(y) * size_t(w) + size_t(x)] = uint8_t((sum + 128) >> 8);
}

// ---- FAST-9 score: the largest threshold t at which 9 contiguous pixels of the 16-pixel radius-3 circle are all >= centre + t
// (or all <= centre - t), i.e. the maximum over the 16 arcs of the minimum difference in the arc, brighter and darker apart;
// 0 where there is no such arc and outside the level's border.  Tile with a 3-pixel halo in LDS.
__device__ __forceinline__ int arc9_max_of_min(const int (&v)[16]) {
  int m2[16], m4[16], best = -256;
#pragma unroll
  for (int i = 0; i < 16; i++) m2[i] = min(v[i], v[(i + 1) & 15]);
#pragma unroll
  for (int i = 0; i < 16; i++) m4[i] = min(m2[i], m2[(i + 2) & 15]);
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const int m8 = min(m4[i], m4[(i + 4) & 15]);
    best = max(best, min(m8, v[(i + 8) & 15]));
  }
  return best;
}

__global__ __launch_bounds__(kFeatThreads) void k_fast_score(const uint8_t* __restrict__ img, int w, int h, uint8_t* __restrict__ score) {
  constexpr int LW = kFeatTileW + 6, LH = kFeatTileH + 6;
  __shared__ uint8_t tile[LH * LW];
  const int bx = int(blockIdx.x) * kFeatTileW, by = int(blockIdx.y) * kFeatTileH;
  for (int k = int(threadIdx.x); k < LW * LH; k += kFeatThreads) {
    const int lx = k % LW, ly = k / LW;
    tile[k] = img[size_t(clampi(by + ly - 3, 0, h - 1)) * size_t(w) + size_t(clampi(bx + lx - 3, 0, w - 1))];
  }
  __syncthreads();
  const int tx = int(threadIdx.x % kFeatTileW), ty = int(threadIdx.x / kFeatTileW);
  const int x = bx + tx, y = by + ty;
  if (x >= w || y >= h) return;
  int s = 0;
  if (x >= kFeatBorder && y >= kFeatBorder && x < w - kFeatBorder && y < h - kFeatBorder) {
    constexpr int ox[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    constexpr int oy[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
    const int c = tile[(ty + 3) * LW + tx + 3];
    int up[16], dn[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int d = int(tile[(ty + 3 + oy[i]) * LW + tx + 3 + ox[i]]) - c;
      up[i] = d, dn[i] = -d;
    }
    s = max(0, max(arc9_max_of_min(up), arc9_max_of_min(dn)));
  }
  score[size_t(y) * size_t(w) + size_t(x)] = uint8_t(s);
}

// ---- non-maximum suppression and the sort key: a pixel with score >= t survives when no pixel of its (2 r + 1)^2 window has a
// higher score and no earlier pixel in (y, x) order an equal one.  A survivor whose level-0 pixel is invalid in the caller's mask
// is dropped AFTER it has suppressed its neighbours.  key = (255 - score) << 40 | level << 32 | y << 16 | x: ascending keys are
// score descending, then level, y, x.  One key per pixel of the level (kFeatNoKey for the rest): the ORDER comes from the sort.
__device__ __forceinline__ int level_to_zero(int v, match_u64 num, match_u64 den, int size0) {
  const match_u64 q = (match_u64(2 * v + 1) * num) / den;
  return q < match_u64(size0) ? int(q) : size0 - 1;
}

__global__ __launch_bounds__(kFeatThreads) void k_nms_keys(const uint8_t* __restrict__ score, int w, int h, int level, int radius, int threshold, const uint8_t* __restrict__ mask0,
                                                           int W0, int H0, match_u64 num, match_u64 den, match_u64* __restrict__ keys) {
  const int x = int(blockIdx.x) * kFeatTileW + int(threadIdx.x % kFeatTileW), y = int(blockIdx.y) * kFeatTileH + int(threadIdx.x / kFeatTileW);
  if (x >= w || y >= h) return;
  const size_t p = size_t(y) * size_t(w) + size_t(x);
  const int s = score[p];
  match_u64 key = kFeatNoKey;
  if (s >= threshold) {
    bool keep = true;
    const int ylo = max(y - radius, 0), yhi = min(y + radius, h - 1), xlo = max(x - radius, 0), xhi = min(x + radius, w - 1);
    for (int yy = ylo; yy <= yhi && keep; yy++) {
      const uint8_t* row = score + size_t(yy) * size_t(w);
      const bool earlier_row = yy < y;
      for (int xx = xlo; xx <= xhi; xx++) {
        const int o = row[xx];
        if (o > s || (o == s && (earlier_row || (yy == y && xx < x)))) keep = false;
      }
    }
    if (keep && mask0) keep = mask0[size_t(level_to_zero(y, num, den, H0)) * size_t(W0) + size_t(level_to_zero(x, num, den, W0))] != 0;
    if (keep) key = (match_u64(255 - s) << 40) | (match_u64(level) << 32) | (match_u64(y) << 16) | match_u64(x);
  }
  keys[p] = key;
}

// number of keys ahead of the first kFeatNoKey in the SORTED array (*count zeroed by the host: stays 0 when there is none);
// exactly one thread finds the boundary
__global__ __launch_bounds__(kFeatThreads) void k_count_keys(const match_u64* __restrict__ keys, int total, int* __restrict__ count) {
  const int i = int(blockIdx.x) * kFeatThreads + int(threadIdx.x);
  if (i >= total) return;
  if (keys[i] != kFeatNoKey && (i + 1 == total || keys[i + 1] == kFeatNoKey)) *count = i + 1;
}

// ---- one workgroup per kept keypoint: thread k evaluates BRIEF test k on the smoothed level (bit k of word k / 32 = first sample
// < second sample; a wave's 64 tests are one ballot), thread 0 writes x0 y0 level score
__global__ __launch_bounds__(kBriefPairs) void k_describe(const match_u64* __restrict__ keys, FeatLevels lv, int32_t* __restrict__ kpts, uint32_t* __restrict__ desc) {
  const match_u64 key = keys[blockIdx.x];
  const int x = int(key & 0xffffULL), y = int((key >> 16) & 0xffffULL), level = int((key >> 32) & 0xffULL), s = 255 - int((key >> 40) & 0xffULL);
  const uint8_t* img = lv.smooth[level];
  const int w = lv.w[level];
  const int k = int(threadIdx.x);
  const int ax = kBriefTable[4 * k], ay = kBriefTable[4 * k + 1], bx = kBriefTable[4 * k + 2], by = kBriefTable[4 * k + 3];
  const int a = img[size_t(y + ay) * size_t(w) + size_t(x + ax)], b = img[size_t(y + by) * size_t(w) + size_t(x + bx)];
  const match_u64 bits = __ballot(a < b);
  if ((k & 63) == 0) {
    desc[8 * size_t(blockIdx.x) + size_t(k >> 5)] = uint32_t(bits & 0xffffffffULL);
    desc[8 * size_t(blockIdx.x) + size_t(k >> 5) + 1] = uint32_t(bits >> 32);
  }
  if (k == 0) {
    int32_t* o = kpts + 4 * size_t(blockIdx.x);
    o[0] = level_to_zero(x, lv.num[level], lv.den[level], lv.W0);
    o[1] = level_to_zero(y, lv.num[level], lv.den[level], lv.H0);
    o[2] = level, o[3] = s;
  }
}

// ---- for every row descriptor the best and second-best Hamming distance over all column descriptors; a tie goes to the lowest
// column (strict <).  One lane holds one row in 8 VGPRs; the wave walks column tiles staged in LDS, every lane reading the SAME
// address (a broadcast: no bank conflict); a pair costs 8 x (xor, popcount, add).  second = kHammingNone with one column.
__global__ __launch_bounds__(kMatchThreads) void k_hamming_best(const uint32_t* __restrict__ rows, int nr, const uint32_t* __restrict__ cols, int nc, int32_t* __restrict__ best,
                                                                int32_t* __restrict__ d_best, int32_t* __restrict__ d_second) {
  __shared__ uint4 tile[2 * kMatchTile];
  const int i = int(blockIdx.x) * kMatchThreads + int(threadIdx.x);
  uint4 r0 = make_uint4(0, 0, 0, 0), r1 = r0;
  if (i < nr) {
    const uint4* r = reinterpret_cast<const uint4*>(rows) + 2 * size_t(i);
    r0 = r[0], r1 = r[1];
  }
  int d1 = kHammingNone, d2 = kHammingNone, j1 = -1;
  const uint4* c4 = reinterpret_cast<const uint4*>(cols);
  for (int t0 = 0; t0 < nc; t0 += kMatchTile) {
    const int nt = min(kMatchTile, nc - t0);
    __syncthreads();
    for (int k = int(threadIdx.x); k < 2 * nt; k += kMatchThreads) tile[k] = c4[2 * size_t(t0) + size_t(k)];
    __syncthreads();
    for (int j = 0; j < nt; j++) {
      const uint4 a = tile[2 * j], b = tile[2 * j + 1];
      const int d = __popc(r0.x ^ a.x) + __popc(r0.y ^ a.y) + __popc(r0.z ^ a.z) + __popc(r0.w ^ a.w) + __popc(r1.x ^ b.x) + __popc(r1.y ^ b.y) + __popc(r1.z ^ b.z) +
                    __popc(r1.w ^ b.w);
      if (d < d1) {
        d2 = d1, d1 = d, j1 = t0 + j;
      } else if (d < d2) {
        d2 = d;
      }
    }
  }
  if (i < nr) best[i] = j1, d_best[i] = d1, d_second[i] = d2;
}

// row i -> column j is accepted when j is i's best, i is j's best, d1 <= max_distance and d1 * ratio_den < d2 * ratio_num
__global__ __launch_bounds__(kFeatThreads) void k_mutual(int nr, const int32_t* __restrict__ best01, const int32_t* __restrict__ d1, const int32_t* __restrict__ d2,
                                                         const int32_t* __restrict__ best10, int max_distance, long long ratio_num, long long ratio_den, int32_t* __restrict__ match01) {
  const int i = int(blockIdx.x) * kFeatThreads + int(threadIdx.x);
  if (i >= nr) return;
  const int j = best01[i];
  const bool ok = j >= 0 && best10[j] == i && d1[i] <= max_distance && (long long)d1[i] * ratio_den < (long long)d2[i] * ratio_num;
  match01[i] = ok ? j : -1;
}

}  // namespace nidreg
