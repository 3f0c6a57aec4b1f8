// nid_ouster_kernels.hpp -- Ouster lidar UDP packets (profiles LEGACY, RNG19_RFL8_SIG16_NIR16, RNG15_RFL8_NIR8) to 32-byte point
// records (include/nidreg.h: nidreg_ouster_decode, which states the layouts and the rules; host side: nidreg_ouster.hip).  One
// workgroup per COLUMN (grid: columns_per_packet x num_packets), one thread per pixel: H is 16, 32, 64 or 128 and the block is 128
// threads = two wave64, so no thread loops; at H = 16 most lanes only help with the staging loads.  The position is fp64 in the order
// the header gives, the translation unit is built with -ffp-contract=off and every sine and cosine comes from the two tables the host
// built with libm, so the records equal the numpy restatement (tests/ouster_oracle.py) bit for bit.  No atomics, no waiting between
// workgroups: a column's count of returns is two ballots and one sum, and a packet's is the sum of its columns' in a second, tiny
// kernel (k_ouster_sum_returns).
//
// SOURCE  the packets as the batcher laid them out: one every `stride` bytes, and inside a packet the 32-byte header of the
// non-legacy profiles and columns of 16 + 12 H + 4, 12 + 12 H or 12 + 4 H bytes, so a column starts at any byte address.  The
// workgroup loads the aligned dwords that cover its column -- coalesced, at most (3 + 16 + 12 * 128 + 4 + 3) / 4 = 390; the host pads
// the device copy so that the last one is inside it -- into LDS, and every field is then assembled from LDS bytes at (address & 3) +
// offset: no pointer into the packet is ever cast to a wider type.
// OUTPUT  a record is 8 dwords, a power of two: records laid into LDS one after the other would put dword j of every fourth pixel on
// one of the 32 banks a ds_write_b32 has (8-way conflicts).  LDS instead holds eight PLANES, dword j of pixel i at j * 132 + i: the
// 32 lanes of a half wave write consecutive dwords of one plane (no conflict, whatever the pitch), and on the way out flat dword f
// of the column's H * 8 reads plane f % 8 at pixel f / 8 -- a half wave covers 4 pixels x 8 planes, and with the pitch 132 = 4 mod 32
// those 32 addresses fall on 32 different banks.  The column then leaves as H * 8 contiguous dwords, coalesced stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nidreg {

constexpr int kOusterLegacy = 0, kOusterRng19 = 1, kOusterRng15 = 2;  // NIDREG_OUSTER_* of include/nidreg.h
constexpr int kOusterThreads = 128;                                     // the largest H
constexpr int kOusterRecordWords = 8;
constexpr int kOusterPlanePitch = 132;                                  // >= 128 and = 4 mod 32: see OUTPUT above
constexpr int kOusterMaxColumnBytes = 16 + 12 * 128 + 4;                // a LEGACY column of 128 pixels
constexpr int kOusterStageWords = (3 + kOusterMaxColumnBytes + 3) / 4;  // 390
constexpr uint32_t kOusterQuietNaN = 0x7FC00000u;

__host__ __device__ constexpr int ouster_packet_header_bytes(int profile) { return profile == kOusterLegacy ? 0 : 32; }
__host__ __device__ constexpr int ouster_column_header_bytes(int profile) { return profile == kOusterLegacy ? 16 : 12; }
__host__ __device__ constexpr int ouster_pixel_bytes(int profile) { return profile == kOusterRng15 ? 4 : 12; }
__host__ __device__ constexpr int ouster_column_bytes(int profile, int H) {
  return ouster_column_header_bytes(profile) + ouster_pixel_bytes(profile) * H + (profile == kOusterLegacy ? 4 : 0);
}
// LEGACY C (20 + 12 H), RNG19 64 + C (12 + 12 H), RNG15 64 + C (12 + 4 H): header and footer are 32 bytes each
__host__ __device__ constexpr int ouster_packet_bytes(int profile, int H, int C) { return (profile == kOusterLegacy ? 0 : 64) + C * ouster_column_bytes(profile, H); }

__device__ inline uint32_t ouster_u16(const uint8_t* p) { return uint32_t(p[0]) | uint32_t(p[1]) << 8; }
__device__ inline uint32_t ouster_u32(const uint8_t* p) { return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24; }

// src: 4-byte aligned, readable up to the dword that holds the last packet's last byte.  column_table: W x (cos E, sin E).
// beam_table: H x (cos A, sin A, cos P, sin P).  pose: 13 doubles, transform12 (rows of R | t, millimetres) then n.  records:
// num_packets x C x H x 8 dwords.  column_returns (nullable): num_packets x C counts.  Grid: (C, num_packets); block: kOusterThreads.
template <int PROFILE>
__global__ __launch_bounds__(kOusterThreads) void k_ouster_decode(const uint8_t* __restrict__ src, long long stride, int H, int W, const double* __restrict__ column_table,
                                                                   const double* __restrict__ beam_table, const double* __restrict__ pose, unsigned long long ts0,
                                                                   uint32_t* __restrict__ records, int32_t* __restrict__ column_returns) {
  __shared__ uint32_t s_column[kOusterStageWords + 1];
  __shared__ uint32_t s_planes[kOusterRecordWords * kOusterPlanePitch];
  __shared__ int s_counts[kOusterThreads / 64];

  const int t = threadIdx.x;
  const int c = blockIdx.x, C = gridDim.x;
  const long long p = blockIdx.y;
  const int column_bytes = ouster_column_bytes(PROFILE, H);
  const long long begin = p * stride + ouster_packet_header_bytes(PROFILE) + (long long)c * column_bytes;  // byte offset of the column in src
  const int shift = int(begin & 3);                                                                        // ... inside its first aligned dword
  const int words = (shift + column_bytes + 3) / 4;                                                        // <= kOusterStageWords
  const uint32_t* const aligned = reinterpret_cast<const uint32_t*>(src + (begin - shift));
  for (int w = t; w < words; w += kOusterThreads) s_column[w] = aligned[w];
  __syncthreads();

  const uint8_t* const col = reinterpret_cast<const uint8_t*>(s_column) + shift;  // LDS bytes of the column
  const unsigned long long timestamp = (unsigned long long)ouster_u32(col) | (unsigned long long)ouster_u32(col + 4) << 32;
  const int m = int(ouster_u16(col + 8));
  const bool valid = PROFILE == kOusterLegacy ? ouster_u32(col + 16 + 12 * H) == 0xFFFFFFFFu : (ouster_u16(col + 10) & 1u) != 0;
  const unsigned long long dt = timestamp - ts0;  // modulo 2^64
  const uint32_t time = dt > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(dt);

  const int i = t;
  bool hit = false;
  if (i < H) {
    const uint8_t* const px = col + ouster_column_header_bytes(PROFILE) + ouster_pixel_bytes(PROFILE) * i;
    uint32_t range, reflectivity, signal, near_ir;
    if (PROFILE == kOusterLegacy) {
      range = ouster_u32(px) & 0x000FFFFFu, reflectivity = ouster_u16(px + 4), signal = ouster_u16(px + 6), near_ir = ouster_u16(px + 8);
    } else if (PROFILE == kOusterRng19) {
      range = ouster_u32(px) & 0x0007FFFFu, reflectivity = px[4], signal = ouster_u16(px + 6), near_ir = ouster_u16(px + 8);
    } else {
      range = (ouster_u16(px) & 0x7FFFu) << 3, reflectivity = px[2], signal = 0, near_ir = uint32_t(px[3]) << 4;
    }
    hit = valid && m < W && range != 0;
    uint32_t r0, r1, r2, r3, r5, r6, r7;
    if (hit) {
      const double cosE = column_table[2 * m], sinE = column_table[2 * m + 1];
      const double* const B = beam_table + 4 * i;
      const double cosA = B[0], sinA = B[1], cosP = B[2], sinP = B[3];
      const double n = pose[12];
      const double cc = cosE * cosA - sinE * sinA;
      const double ss = sinE * cosA + cosE * sinA;
      const double d = double(range) - n;
      const double lx = d * (cc * cosP) + n * cosE;
      const double ly = d * (ss * cosP) + n * sinE;
      const double lz = d * sinP;
      const double X = ((pose[0] * lx + pose[1] * ly) + pose[2] * lz) + pose[3];
      const double Y = ((pose[4] * lx + pose[5] * ly) + pose[6] * lz) + pose[7];
      const double Z = ((pose[8] * lx + pose[9] * ly) + pose[10] * lz) + pose[11];
      r0 = __float_as_uint(float(X * 0.001)), r1 = __float_as_uint(float(Y * 0.001)), r2 = __float_as_uint(float(Z * 0.001));
      r3 = __float_as_uint(float(signal));
      r5 = reflectivity | uint32_t(i) << 16, r6 = near_ir, r7 = range;
    } else {
      r0 = r1 = r2 = kOusterQuietNaN;
      r3 = 0, r5 = uint32_t(i) << 16, r6 = 0, r7 = 0;
    }
    s_planes[0 * kOusterPlanePitch + i] = r0;
    s_planes[1 * kOusterPlanePitch + i] = r1;
    s_planes[2 * kOusterPlanePitch + i] = r2;
    s_planes[3 * kOusterPlanePitch + i] = r3;
    s_planes[4 * kOusterPlanePitch + i] = time;
    s_planes[5 * kOusterPlanePitch + i] = r5;
    s_planes[6 * kOusterPlanePitch + i] = r6;
    s_planes[7 * kOusterPlanePitch + i] = r7;
  }
  const unsigned long long mask = __ballot(hit);
  if ((t & 63) == 0) s_counts[t / 64] = __popcll(mask);
  __syncthreads();

  uint32_t* const out = records + (p * C + c) * (long long)(H * kOusterRecordWords);
  for (int f = t; f < H * kOusterRecordWords; f += kOusterThreads) out[f] = s_planes[(f % kOusterRecordWords) * kOusterPlanePitch + f / kOusterRecordWords];
  if (column_returns && t == 0) column_returns[p * C + c] = s_counts[0] + s_counts[1];
}

// returns[p] = the sum of packet p's C column counts; one thread per packet
__global__ void k_ouster_sum_returns(const int32_t* __restrict__ column_returns, int num_packets, int C, int32_t* __restrict__ returns) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= num_packets) return;
  int n = 0;
  for (int c = 0; c < C; c++) n += column_returns[p * C + c];
  returns[p] = n;
}

}  // namespace nidreg
