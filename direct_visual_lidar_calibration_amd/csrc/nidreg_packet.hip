// nidreg_packet.hip -- C ABI of the Velodyne packet decode (include/nidreg.h: nidreg_velodyne_decode) and the translation unit of
// its kernel (nid_packet_kernels.hpp).  Stateless for the caller, like nidreg_image_to_mono8: validation (all of it BEFORE the
// device is touched), ONE upload of laser table + packet times + the packets as they lie in the message, one launch, the copy back.
// What stays on a device between calls is the pair of 36000-entry cosine / sine tables, which no argument changes.  No CPU path
// for the arithmetic.
#include "nid_launch.hpp"
#include "nid_packet_kernels.hpp"

#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

using namespace nidreg;

namespace {

constexpr int64_t kMaxPackets = 65536;
constexpr int64_t kMaxStride = 4096;  // the messages' are 1214 and 1216; the bound keeps the staged packet area below 2^28 bytes

thread_local double g_packet_ms[3] = {0, 0, 0};  // of this thread's last nidreg_velodyne_decode: upload, kernel, copy back

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// cos / sin of az * (pi / 18000), az = 0..35999, by libm on the host (tests/velodyne_oracle.py builds the same with math.cos /
// math.sin and the same argument expression); 2 x 36000 doubles per device, uploaded at the first call and kept for the process
std::mutex g_trig_mu;
std::map<int, double*> g_trig;

int trig_tables(int device_id, const double** cos_table, const double** sin_table) {
  std::lock_guard<std::mutex> lk(g_trig_mu);
  auto it = g_trig.find(device_id);
  if (it == g_trig.end()) {
    std::vector<double> host;
    try {
      host.assign(2 * size_t(kAzimuthSteps), 0.0);
    } catch (const std::bad_alloc&) {
      return fail(NIDREG_ERR_INVALID, "nidreg_velodyne_decode: no host memory for the cosine / sine tables");
    }
    for (int az = 0; az < kAzimuthSteps; az++) {
      const double angle = double(az) * (M_PI / 18000.0);
      host[az] = std::cos(angle);
      host[size_t(kAzimuthSteps) + az] = std::sin(angle);
    }
    DeviceBuf d;
    HIP_TRY(d.alloc(host.size() * sizeof(double)));
    HIP_TRY(hipMemcpy(d.as<void>(), host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice));
    it = g_trig.emplace(device_id, static_cast<double*>(d.release())).first;
  }
  *cos_table = it->second;
  *sin_table = it->second + kAzimuthSteps;
  return NIDREG_OK;
}

}  // namespace

extern "C" {

int nidreg_velodyne_decode(int device_id, const uint8_t* packets, int64_t num_packets, int64_t packet_stride, const double* packet_times, const double* lasers, int num_lasers,
                           double distance_resolution, double firing_period, double laser_period, float* records_out, int32_t* returns_per_packet) {
  const std::string who = "nidreg_velodyne_decode";
  // every refusal comes before the device is touched, and nothing is written
  if (num_lasers != 16 && num_lasers != 32)
    return fail(NIDREG_ERR_INVALID, who + ": num_lasers " + std::to_string(num_lasers) + ": 16 (the VLP-16 packet layout) and 32 (the HDL-32E layout) are decoded here");
  if (packet_stride < kPacketBytes) return fail(NIDREG_ERR_INVALID, who + ": packet_stride " + std::to_string(packet_stride) + " is below the " + std::to_string(kPacketBytes) + " bytes of a packet");
  if (packet_stride > kMaxStride) return fail(NIDREG_ERR_INVALID, who + ": packet_stride " + std::to_string(packet_stride) + " is above " + std::to_string(kMaxStride));
  if (num_packets < 0 || num_packets > kMaxPackets) return fail(NIDREG_ERR_INVALID, who + ": num_packets " + std::to_string(num_packets) + " outside [0, " + std::to_string(kMaxPackets) + "]");
  if (num_packets > 0 && (!packets || !packet_times || !lasers || !records_out)) return fail(NIDREG_ERR_INVALID, who + ": null packets, packet_times, lasers or records_out");
  for (int i = 0; lasers && i < num_lasers * kLaserDoubles; i++)
    if (!std::isfinite(lasers[i]))
      return fail(NIDREG_ERR_INVALID, who + ": laser table entry " + std::to_string(i % kLaserDoubles) + " of laser " + std::to_string(i / kLaserDoubles) + " is not finite");
  if (!std::isfinite(distance_resolution) || !std::isfinite(firing_period) || !std::isfinite(laser_period))
    return fail(NIDREG_ERR_INVALID, who + ": distance_resolution, firing_period or laser_period is not finite");
  if (num_packets == 0) return NIDREG_OK;
  if (const int rc = use_device(who.c_str(), device_id)) return rc;

  const auto t_upload = std::chrono::steady_clock::now();
  const double *d_cos = nullptr, *d_sin = nullptr;
  if (const int rc = trig_tables(device_id, &d_cos, &d_sin)) return rc;
  // one staging block, one copy: [laser table: 32 x 8 doubles][packet times][the packet area, then padding to whole dwords]
  const size_t N = size_t(num_packets);
  const size_t laser_bytes = 32 * kLaserDoubles * sizeof(double), time_bytes = N * sizeof(double);
  const size_t packet_bytes = (N - 1) * size_t(packet_stride) + kPacketBytes;  // the last packet's tail is not the caller's to give
  const size_t total = laser_bytes + time_bytes + ((packet_bytes + 3) / 4) * 4 + 4;
  std::vector<uint8_t> stage;
  try {
    stage.assign(total, 0);
  } catch (const std::bad_alloc&) {  // (nothing may leave an extern "C" function)
    return fail(NIDREG_ERR_INVALID, who + ": no host memory for a staging block of " + std::to_string(total) + " bytes");
  }
  std::memcpy(stage.data(), lasers, size_t(num_lasers) * kLaserDoubles * sizeof(double));
  std::memcpy(stage.data() + laser_bytes, packet_times, time_bytes);
  std::memcpy(stage.data() + laser_bytes + time_bytes, packets, packet_bytes);
  const size_t record_floats = N * kPacketThreads * kPacketRecordFloats;
  DeviceBuf d_in, d_rec, d_ret;
  HIP_TRY(d_in.alloc(total));
  HIP_TRY(d_rec.alloc(record_floats * sizeof(float)));
  if (returns_per_packet) HIP_TRY(d_ret.alloc(N * sizeof(int32_t)));
  HIP_TRY(hipMemcpy(d_in.as<void>(), stage.data(), total, hipMemcpyHostToDevice));
  g_packet_ms[0] = ms_since(t_upload);

  const auto t_kernel = std::chrono::steady_clock::now();
  const uint8_t* const base = d_in.as<uint8_t>();
  const double* const d_lasers = reinterpret_cast<const double*>(base);
  const double* const d_times = reinterpret_cast<const double*>(base + laser_bytes);
  const uint8_t* const d_packets = base + laser_bytes + time_bytes;  // 8-byte aligned: the kernel's dword loads need 4
  const dim3 grid(static_cast<unsigned>(num_packets)), block(kPacketThreads);
  if (num_lasers == 16)
    hipLaunchKernelGGL(k_velodyne_decode<16>, grid, block, 0, nullptr, d_packets, (long long)packet_stride, d_times, d_lasers, d_cos, d_sin, distance_resolution, firing_period, laser_period,
                       d_rec.as<float>(), d_ret.as<int32_t>());
  else
    hipLaunchKernelGGL(k_velodyne_decode<32>, grid, block, 0, nullptr, d_packets, (long long)packet_stride, d_times, d_lasers, d_cos, d_sin, distance_resolution, firing_period, laser_period,
                       d_rec.as<float>(), d_ret.as<int32_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(nullptr));
  g_packet_ms[1] = ms_since(t_kernel);

  const auto t_copy = std::chrono::steady_clock::now();
  HIP_TRY(hipMemcpy(records_out, d_rec.as<void>(), record_floats * sizeof(float), hipMemcpyDeviceToHost));
  if (returns_per_packet) HIP_TRY(hipMemcpy(returns_per_packet, d_ret.as<void>(), N * sizeof(int32_t), hipMemcpyDeviceToHost));
  g_packet_ms[2] = ms_since(t_copy);
  return NIDREG_OK;
}

int nidreg_velodyne_get_timing(double* ms3) {
  if (!ms3) return fail(NIDREG_ERR_INVALID, "nidreg_velodyne_get_timing: null argument");
  std::memcpy(ms3, g_packet_ms, sizeof(g_packet_ms));
  return NIDREG_OK;
}

}  // extern "C"
