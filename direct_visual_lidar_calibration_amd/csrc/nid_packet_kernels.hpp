// nid_packet_kernels.hpp -- Velodyne data packets (VLP-16 / HDL-32E layout) to point records (include/nidreg.h:
// nidreg_velodyne_decode, which states the rules; host side: nidreg_packet.hip).  One workgroup per packet, one thread per return:
// 12 blocks x 32 slots = 384 threads = six wave64.  The position is fp64 in the order the header gives, the translation unit is built
// with -ffp-contract=off and the sines and cosines come from tables the host built with libm, so the records equal the numpy
// restatement (tests/velodyne_oracle.py) bit for bit.  No atomics: the per-packet count is six ballots and one sum.
//
// SOURCE  the packets as they lie in the message: 1206 data bytes every `stride` bytes, 1214 apart in a ROS1 message and 1216 in
// CDR, so a packet starts at any address.  The workgroup loads the aligned dwords that cover its packet -- coalesced, at most 303 of
// them; the host pads the device copy so that the last one is inside it -- into LDS, and every field is then assembled from LDS
// bytes at (address & 3) + offset: no pointer into the packet is ever cast to a wider type.
// OUTPUT  the 384 records x 5 float32 of a packet go through LDS (stride 5 dwords: odd, no bank conflict) and leave as 1920
// contiguous dwords, five coalesced stores a thread, instead of five stores 20 bytes apart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nidreg {

constexpr int kPacketBytes = 1206;    // 12 blocks of 100 bytes, the device's timestamp (4), return mode, product id
constexpr int kPacketBlocks = 12;
constexpr int kPacketSlots = 32;
constexpr int kPacketThreads = kPacketBlocks * kPacketSlots;  // 384: one thread per return
constexpr int kPacketRecordFloats = 5;                        // x y z intensity time
constexpr int kPacketStageWords = (3 + kPacketBytes + 3) / 4;  // 303: the aligned dwords that cover a packet at any address
constexpr int kAzimuthSteps = 36000;                          // 0.01 degree
constexpr uint32_t kPacketBlockFlag = 0xEEFFu;                // bytes FF EE
constexpr uint32_t kQuietNaN = 0x7FC00000u;

// one row of the laser table: cos_vert, sin_vert, cos_rot_corr, sin_rot_corr, vert_offset, horiz_offset, dist_corr, 0
constexpr int kLaserDoubles = 8;

// src: 4-byte aligned, readable up to the dword that holds the last packet's last byte.  cos_table / sin_table: kAzimuthSteps
// doubles each.  records: num_packets x 1920 floats.  returns (nullable): num_packets counts.  LASERS: 16 or 32.
template <int LASERS>
__global__ __launch_bounds__(kPacketThreads) void k_velodyne_decode(const uint8_t* __restrict__ src, long long stride, const double* __restrict__ packet_times,
                                                                     const double* __restrict__ lasers, const double* __restrict__ cos_table, const double* __restrict__ sin_table,
                                                                     double distance_resolution, double firing_period, double laser_period, float* __restrict__ records,
                                                                     int32_t* __restrict__ returns) {
  __shared__ uint32_t s_packet[kPacketStageWords + 1];
  __shared__ float s_records[kPacketThreads * kPacketRecordFloats];
  __shared__ int s_counts[kPacketThreads / 64];

  const int t = threadIdx.x;
  const long long p = blockIdx.x;
  const long long begin = p * stride;          // byte offset of the packet in src
  const int shift = int(begin & 3);            // ... inside its first aligned dword
  const int words = (shift + kPacketBytes + 3) / 4;
  const uint32_t* const aligned = reinterpret_cast<const uint32_t*>(src + (begin - shift));
  if (t < words) s_packet[t] = aligned[t];
  __syncthreads();

  const uint8_t* const pk = reinterpret_cast<const uint8_t*>(s_packet) + shift;  // LDS bytes of the packet
  const int b = t / kPacketSlots, s = t % kPacketSlots;
  const uint8_t* const blk = pk + 100 * b;
  const uint32_t flag = uint32_t(blk[0]) | uint32_t(blk[1]) << 8;
  const int a = int(uint32_t(blk[2]) | uint32_t(blk[3]) << 8);
  const uint32_t raw = uint32_t(blk[4 + 3 * s]) | uint32_t(blk[5 + 3 * s]) << 8;
  const uint32_t reflectivity = blk[6 + 3 * s];

  int l, k, az;
  if (LASERS == 16) {
    const int f = s / 16;
    l = s % 16;
    k = 2 * b + f;
    // the azimuth the block turns through: to the next block's, the last block reusing its predecessor's; the flags play no part
    const int b0 = b < kPacketBlocks - 1 ? b : kPacketBlocks - 2;
    const uint8_t* const q0 = pk + 100 * b0;
    const uint8_t* const q1 = q0 + 100;
    const int a0 = int(uint32_t(q0[2]) | uint32_t(q0[3]) << 8), a1 = int(uint32_t(q1[2]) | uint32_t(q1[3]) << 8);
    // the header's % is the FLOORED modulo: an azimuth field is any uint16 (nothing keeps a corrupted or unflagged block's below
    // 36000), so a1 - a0 lies in [-65535, 65535] and C++'s truncating % alone could leave diff, and with it the table index, negative
    const int diff = ((a1 - a0) % kAzimuthSteps + kAzimuthSteps) % kAzimuthSteps;     // [0, 35999]
    az = (a + (2 * diff * (l + 24 * f) + 48) / 96) % kAzimuthSteps;  // operands >= 0, the sum below 2^22: [0, 35999]
  } else {
    l = s;
    k = b;
    az = a % kAzimuthSteps;
  }

  const double time = packet_times[p] + (double(k) * firing_period + double(l) * laser_period);
  const bool hit = flag == kPacketBlockFlag && raw != 0;
  float x, y, z, intensity;
  if (hit) {
    const double* const L = lasers + kLaserDoubles * l;
    const double cos_v = L[0], sin_v = L[1], cos_rc = L[2], sin_rc = L[3], voff = L[4], hoff = L[5], dist_corr = L[6];
    const double C = cos_table[az], S = sin_table[az];
    const double d = double(raw) * distance_resolution + dist_corr;
    const double cr = C * cos_rc + S * sin_rc;
    const double sr = S * cos_rc - C * sin_rc;
    const double xy = d * cos_v - voff * sin_v;
    const double xv = xy * sr - hoff * cr;
    const double yv = xy * cr + hoff * sr;
    const double zv = d * sin_v + voff * cos_v;
    x = float(yv), y = float(-xv), z = float(zv);  // the driver's turn into the ROS frame
    intensity = float(reflectivity);
  } else {
    x = y = z = __uint_as_float(kQuietNaN);
    intensity = 0.0f;
  }
  float* const rec = s_records + kPacketRecordFloats * t;
  rec[0] = x, rec[1] = y, rec[2] = z, rec[3] = intensity, rec[4] = float(time);

  const unsigned long long mask = __ballot(hit);
  if ((t & 63) == 0) s_counts[t / 64] = __popcll(mask);
  __syncthreads();

  float* const out = records + p * (long long)(kPacketThreads * kPacketRecordFloats);
#pragma unroll
  for (int j = 0; j < kPacketRecordFloats; j++) out[j * kPacketThreads + t] = s_records[j * kPacketThreads + t];
  if (returns && t == 0) {
    int n = 0;
#pragma unroll
    for (int w = 0; w < kPacketThreads / 64; w++) n += s_counts[w];
    returns[p] = n;
  }
}

}  // namespace nidreg
