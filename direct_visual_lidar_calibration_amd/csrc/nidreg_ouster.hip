// nidreg_ouster.hip -- C ABI of the Ouster packet decode (include/nidreg.h: nidreg_ouster_decode) and the translation unit of its
// kernels (nid_ouster_kernels.hpp).  Stateless, like nidreg_velodyne_decode next door (nidreg_packet.hip): validation (all of it
// BEFORE the device is touched), ONE upload of column table + beam table + transform + the packets as the batcher laid them out, one
// launch (two with returns_per_packet), the copy back.  Nothing stays on a device between calls: the tables are the caller's, built
// from the sensor's metadata.  No CPU path for the arithmetic.
#include "nid_host.hpp"
#include "nid_ouster_kernels.hpp"

#include <cmath>

using namespace nidreg;

namespace {

constexpr int64_t kMaxPackets = 4096;   // two turns of 2048 columns at one column a packet; 4096 x 16 x 128 records are 256 MiB
constexpr int64_t kMaxStride = 32768;   // the largest packet (LEGACY, H = 128, C = 16) is 24896 bytes
constexpr int kPoseDoubles = 16;        // transform12, n, padding: keeps the packet area 8-byte aligned

thread_local PhaseClock<3> g_ouster_clock;  // of this thread's last nidreg_ouster_decode: upload, kernel, copy back

}  // namespace

extern "C" {

int nidreg_ouster_decode(int device_id, const uint8_t* packets, int64_t num_packets, int64_t packet_stride, int profile, int H, int W, int C, const double* column_table,
                         const double* beam_table, double n_mm, const double* transform12, uint64_t ts0, void* records_out, int32_t* returns_per_packet) {
  const std::string who = "nidreg_ouster_decode";
  // every refusal comes before the device is touched, and nothing is written
  if (profile != kOusterLegacy && profile != kOusterRng19 && profile != kOusterRng15)
    return fail(NIDREG_ERR_INVALID, who + ": profile " + std::to_string(profile) + ": 0 (LEGACY), 1 (RNG19_RFL8_SIG16_NIR16) and 2 (RNG15_RFL8_NIR8) are decoded here");
  if (H != 16 && H != 32 && H != 64 && H != 128) return fail(NIDREG_ERR_INVALID, who + ": H " + std::to_string(H) + ": 16, 32, 64 and 128 pixels per column are decoded here");
  if (W < 16 || W > 4096) return fail(NIDREG_ERR_INVALID, who + ": W " + std::to_string(W) + " outside [16, 4096]");
  if (C < 1 || C > 16) return fail(NIDREG_ERR_INVALID, who + ": C " + std::to_string(C) + " outside [1, 16]");
  const int64_t size = ouster_packet_bytes(profile, H, C);
  if (const int rc = check_packets(who, num_packets, kMaxPackets, packet_stride, size, kMaxStride)) return rc;
  if (num_packets > 0 && (!packets || !column_table || !beam_table || !transform12 || !records_out))
    return fail(NIDREG_ERR_INVALID, who + ": null packets, column_table, beam_table, transform12 or records_out");
  for (int i = 0; column_table && i < 2 * W; i++)
    if (!std::isfinite(column_table[i])) return fail(NIDREG_ERR_INVALID, who + ": column table entry " + std::to_string(i % 2) + " of column " + std::to_string(i / 2) + " is not finite");
  for (int i = 0; beam_table && i < 4 * H; i++)
    if (!std::isfinite(beam_table[i])) return fail(NIDREG_ERR_INVALID, who + ": beam table entry " + std::to_string(i % 4) + " of beam " + std::to_string(i / 4) + " is not finite");
  for (int i = 0; transform12 && i < 12; i++)
    if (!std::isfinite(transform12[i])) return fail(NIDREG_ERR_INVALID, who + ": transform12 entry " + std::to_string(i) + " is not finite");
  if (!std::isfinite(n_mm)) return fail(NIDREG_ERR_INVALID, who + ": n_mm is not finite");
  if (num_packets == 0) return NIDREG_OK;
  if (const int rc = use_device(who.c_str(), device_id)) return rc;

  g_ouster_clock.start();
  // one staging block, one copy: [column table: W x 2][beam table: H x 4][transform12, n, 0, 0, 0][the packet area]
  const size_t N = size_t(num_packets);
  const size_t column_bytes = size_t(W) * 2 * sizeof(double), beam_bytes = size_t(H) * 4 * sizeof(double), packet_bytes = packet_area_bytes(num_packets, packet_stride, size);
  StagingBlock stage;
  const size_t o_columns = stage.part(column_bytes), o_beams = stage.part(beam_bytes), o_pose = stage.part(kPoseDoubles * sizeof(double)), o_packets = stage.packet_part(packet_bytes);
  if (const int rc = stage.take(who)) return rc;
  stage.put(o_columns, column_table, column_bytes);
  stage.put(o_beams, beam_table, beam_bytes);
  stage.put(o_pose, transform12, 12 * sizeof(double));
  stage.put(o_pose + 12 * sizeof(double), &n_mm, sizeof(double));
  stage.put(o_packets, packets, packet_bytes);
  const size_t record_words = N * size_t(C) * size_t(H) * kOusterRecordWords;
  DeviceBuf d_rec, d_col, d_ret;
  HIP_TRY(stage.upload());
  HIP_TRY(d_rec.alloc(record_words * sizeof(uint32_t)));
  if (returns_per_packet) {
    HIP_TRY(d_col.alloc(N * size_t(C) * sizeof(int32_t)));
    HIP_TRY(d_ret.alloc(N * sizeof(int32_t)));
  }
  g_ouster_clock.lap(0);

  hipError_t launched = hipErrorInvalidValue;
  with_int<kOusterLegacy, kOusterRng19, kOusterRng15>(profile, [&](auto P) {
    launched = launch(k_ouster_decode<P>, dim3(unsigned(C), unsigned(num_packets)), kOusterThreads, 0, nullptr, stage.device<uint8_t>(o_packets), packet_stride, H, W,
                      stage.device<double>(o_columns), stage.device<double>(o_beams), stage.device<double>(o_pose), ts0, d_rec.as<uint32_t>(), d_col.as<int32_t>());
  });
  HIP_TRY(launched);
  if (returns_per_packet) HIP_TRY(launch(k_ouster_sum_returns, blocks_for(num_packets, 64), 64, 0, nullptr, d_col.as<int32_t>(), int(num_packets), C, d_ret.as<int32_t>()));
  HIP_TRY(hipStreamSynchronize(nullptr));
  g_ouster_clock.lap(1);

  HIP_TRY(hipMemcpy(records_out, d_rec.as<void>(), record_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (returns_per_packet) HIP_TRY(hipMemcpy(returns_per_packet, d_ret.as<void>(), N * sizeof(int32_t), hipMemcpyDeviceToHost));
  g_ouster_clock.lap(2);
  return NIDREG_OK;
}

int nidreg_ouster_get_timing(double* ms3) { return g_ouster_clock.read("nidreg_ouster_get_timing", ms3); }

}  // extern "C"
