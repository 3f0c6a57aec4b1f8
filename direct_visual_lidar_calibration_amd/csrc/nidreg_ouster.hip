// nidreg_ouster.hip -- C ABI of the Ouster packet decode (include/nidreg.h: nidreg_ouster_decode) and the translation unit of its
// kernels (nid_ouster_kernels.hpp).  Stateless, like nidreg_velodyne_decode next door (nidreg_packet.hip): validation (all of it
// BEFORE the device is touched), ONE upload of column table + beam table + transform + the packets as the batcher laid them out, one
// launch (two with returns_per_packet), the copy back.  Nothing stays on a device between calls: the tables are the caller's, built
// from the sensor's metadata.  No CPU path for the arithmetic.
#include "nid_launch.hpp"
#include "nid_ouster_kernels.hpp"

#include <chrono>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace nidreg;

namespace {

constexpr int64_t kMaxPackets = 4096;   // two turns of 2048 columns at one column a packet; 4096 x 16 x 128 records are 256 MiB
constexpr int64_t kMaxStride = 32768;   // the largest packet (LEGACY, H = 128, C = 16) is 24896 bytes
constexpr int kPoseDoubles = 16;        // transform12, n, padding: keeps the packet area 8-byte aligned

thread_local double g_ouster_ms[3] = {0, 0, 0};  // of this thread's last nidreg_ouster_decode: upload, kernel, copy back

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

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
  if (packet_stride < size) return fail(NIDREG_ERR_INVALID, who + ": packet_stride " + std::to_string(packet_stride) + " is below the " + std::to_string(size) + " bytes of a packet");
  if (packet_stride > kMaxStride) return fail(NIDREG_ERR_INVALID, who + ": packet_stride " + std::to_string(packet_stride) + " is above " + std::to_string(kMaxStride));
  if (num_packets < 0 || num_packets > kMaxPackets) return fail(NIDREG_ERR_INVALID, who + ": num_packets " + std::to_string(num_packets) + " outside [0, " + std::to_string(kMaxPackets) + "]");
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

  const auto t_upload = std::chrono::steady_clock::now();
  // one staging block, one copy: [column table: W x 2][beam table: H x 4][transform12, n, 0, 0, 0][the packet area, then padding to whole dwords]
  const size_t N = size_t(num_packets);
  const size_t column_bytes = size_t(W) * 2 * sizeof(double), beam_bytes = size_t(H) * 4 * sizeof(double), pose_bytes = kPoseDoubles * sizeof(double);
  const size_t packet_bytes = (N - 1) * size_t(packet_stride) + size_t(size);  // the last packet's tail is not the caller's to give
  const size_t total = column_bytes + beam_bytes + pose_bytes + ((packet_bytes + 3) / 4) * 4 + 4;
  std::vector<uint8_t> stage;
  try {
    stage.assign(total, 0);
  } catch (const std::bad_alloc&) {  // (nothing may leave an extern "C" function)
    return fail(NIDREG_ERR_INVALID, who + ": no host memory for a staging block of " + std::to_string(total) + " bytes");
  }
  std::memcpy(stage.data(), column_table, column_bytes);
  std::memcpy(stage.data() + column_bytes, beam_table, beam_bytes);
  std::memcpy(stage.data() + column_bytes + beam_bytes, transform12, 12 * sizeof(double));
  std::memcpy(stage.data() + column_bytes + beam_bytes + 12 * sizeof(double), &n_mm, sizeof(double));
  std::memcpy(stage.data() + column_bytes + beam_bytes + pose_bytes, packets, packet_bytes);
  const size_t record_words = N * size_t(C) * size_t(H) * kOusterRecordWords;
  DeviceBuf d_in, d_rec, d_col, d_ret;
  HIP_TRY(d_in.alloc(total));
  HIP_TRY(d_rec.alloc(record_words * sizeof(uint32_t)));
  if (returns_per_packet) {
    HIP_TRY(d_col.alloc(N * size_t(C) * sizeof(int32_t)));
    HIP_TRY(d_ret.alloc(N * sizeof(int32_t)));
  }
  HIP_TRY(hipMemcpy(d_in.as<void>(), stage.data(), total, hipMemcpyHostToDevice));
  g_ouster_ms[0] = ms_since(t_upload);

  const auto t_kernel = std::chrono::steady_clock::now();
  const uint8_t* const base = d_in.as<uint8_t>();
  const double* const d_columns = reinterpret_cast<const double*>(base);
  const double* const d_beams = reinterpret_cast<const double*>(base + column_bytes);
  const double* const d_pose = reinterpret_cast<const double*>(base + column_bytes + beam_bytes);
  const uint8_t* const d_packets = base + column_bytes + beam_bytes + pose_bytes;  // 8-byte aligned: the kernel's dword loads need 4
  const dim3 grid(static_cast<unsigned>(C), static_cast<unsigned>(num_packets)), block(kOusterThreads);
  if (profile == kOusterLegacy)
    hipLaunchKernelGGL(k_ouster_decode<kOusterLegacy>, grid, block, 0, nullptr, d_packets, (long long)packet_stride, H, W, d_columns, d_beams, d_pose, (unsigned long long)ts0,
                       d_rec.as<uint32_t>(), d_col.as<int32_t>());
  else if (profile == kOusterRng19)
    hipLaunchKernelGGL(k_ouster_decode<kOusterRng19>, grid, block, 0, nullptr, d_packets, (long long)packet_stride, H, W, d_columns, d_beams, d_pose, (unsigned long long)ts0,
                       d_rec.as<uint32_t>(), d_col.as<int32_t>());
  else
    hipLaunchKernelGGL(k_ouster_decode<kOusterRng15>, grid, block, 0, nullptr, d_packets, (long long)packet_stride, H, W, d_columns, d_beams, d_pose, (unsigned long long)ts0,
                       d_rec.as<uint32_t>(), d_col.as<int32_t>());
  HIP_TRY(hipGetLastError());
  if (returns_per_packet) {
    hipLaunchKernelGGL(k_ouster_sum_returns, dim3(static_cast<unsigned>((num_packets + 63) / 64)), dim3(64), 0, nullptr, d_col.as<int32_t>(), int(num_packets), C, d_ret.as<int32_t>());
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(nullptr));
  g_ouster_ms[1] = ms_since(t_kernel);

  const auto t_copy = std::chrono::steady_clock::now();
  HIP_TRY(hipMemcpy(records_out, d_rec.as<void>(), record_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (returns_per_packet) HIP_TRY(hipMemcpy(returns_per_packet, d_ret.as<void>(), N * sizeof(int32_t), hipMemcpyDeviceToHost));
  g_ouster_ms[2] = ms_since(t_copy);
  return NIDREG_OK;
}

int nidreg_ouster_get_timing(double* ms3) {
  if (!ms3) return fail(NIDREG_ERR_INVALID, "nidreg_ouster_get_timing: null argument");
  std::memcpy(ms3, g_ouster_ms, sizeof(g_ouster_ms));
  return NIDREG_OK;
}

}  // extern "C"
