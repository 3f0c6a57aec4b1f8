// nidreg_packet.hip -- C ABI of the Velodyne packet decode (include/nidreg.h: nidreg_velodyne_decode) and the translation unit of
// its kernel (nid_packet_kernels.hpp).  Stateless for the caller, like nidreg_image_to_mono8: validation (all of it BEFORE the
// device is touched), ONE upload of laser table + packet times + the packets as they lie in the message, one launch, the copy back.
// What stays on a device between calls is the pair of 36000-entry cosine / sine tables, which no argument changes.  No CPU path
// for the arithmetic.
#include "nid_host.hpp"
#include "nid_packet_kernels.hpp"

#include <cmath>
#include <map>
#include <mutex>

using namespace nidreg;

namespace {

constexpr int64_t kMaxPackets = 65536;
constexpr int64_t kMaxStride = 4096;  // the messages' are 1214 and 1216; the bound keeps the staged packet area below 2^28 bytes

thread_local PhaseClock<3> g_packet_clock;  // of this thread's last nidreg_velodyne_decode: upload, kernel, copy back

// cos / sin of az * (pi / 18000), az = 0..35999, by libm on the host (tests/velodyne_oracle.py builds the same with math.cos /
// math.sin and the same argument expression); 2 x 36000 doubles per device, uploaded at the first call and kept for the process
std::mutex g_trig_mu;
std::map<int, double*> g_trig;

int trig_tables(int device_id, const double** cos_table, const double** sin_table) {
  std::lock_guard<std::mutex> lk(g_trig_mu);
  auto it = g_trig.find(device_id);
  if (it == g_trig.end()) {
    std::vector<uint8_t> bytes;
    if (const int rc = host_zeros(bytes, 2 * size_t(kAzimuthSteps) * sizeof(double), "nidreg_velodyne_decode", "the cosine / sine tables")) return rc;
    double* const host = reinterpret_cast<double*>(bytes.data());
    for (int az = 0; az < kAzimuthSteps; az++) {
      const double angle = double(az) * (M_PI / 18000.0);
      host[az] = std::cos(angle);
      host[size_t(kAzimuthSteps) + az] = std::sin(angle);
    }
    DeviceBuf d;
    HIP_TRY(d.alloc(bytes.size()));
    HIP_TRY(hipMemcpy(d.as<void>(), host, bytes.size(), hipMemcpyHostToDevice));
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
  if (const int rc = check_packets(who, num_packets, kMaxPackets, packet_stride, kPacketBytes, kMaxStride)) return rc;
  if (num_packets > 0 && (!packets || !packet_times || !lasers || !records_out)) return fail(NIDREG_ERR_INVALID, who + ": null packets, packet_times, lasers or records_out");
  for (int i = 0; lasers && i < num_lasers * kLaserDoubles; i++)
    if (!std::isfinite(lasers[i]))
      return fail(NIDREG_ERR_INVALID, who + ": laser table entry " + std::to_string(i % kLaserDoubles) + " of laser " + std::to_string(i / kLaserDoubles) + " is not finite");
  if (!std::isfinite(distance_resolution) || !std::isfinite(firing_period) || !std::isfinite(laser_period))
    return fail(NIDREG_ERR_INVALID, who + ": distance_resolution, firing_period or laser_period is not finite");
  if (num_packets == 0) return NIDREG_OK;
  if (const int rc = use_device(who.c_str(), device_id)) return rc;

  g_packet_clock.start();
  const double *d_cos = nullptr, *d_sin = nullptr;
  if (const int rc = trig_tables(device_id, &d_cos, &d_sin)) return rc;
  // one staging block, one copy: [laser table: 32 x 8 doubles][packet times][the packet area]
  const size_t N = size_t(num_packets);
  const size_t time_bytes = N * sizeof(double), packet_bytes = packet_area_bytes(num_packets, packet_stride, kPacketBytes);
  StagingBlock stage;
  const size_t o_lasers = stage.part(32 * kLaserDoubles * sizeof(double)), o_times = stage.part(time_bytes), o_packets = stage.packet_part(packet_bytes);
  if (const int rc = stage.take(who)) return rc;
  stage.put(o_lasers, lasers, size_t(num_lasers) * kLaserDoubles * sizeof(double));
  stage.put(o_times, packet_times, time_bytes);
  stage.put(o_packets, packets, packet_bytes);
  const size_t record_floats = N * kPacketThreads * kPacketRecordFloats;
  DeviceBuf d_rec, d_ret;
  HIP_TRY(stage.upload());
  HIP_TRY(d_rec.alloc(record_floats * sizeof(float)));
  if (returns_per_packet) HIP_TRY(d_ret.alloc(N * sizeof(int32_t)));
  g_packet_clock.lap(0);

  hipError_t launched = hipErrorInvalidValue;
  with_int<16, 32>(num_lasers, [&](auto L) {
    launched = launch(k_velodyne_decode<L>, unsigned(num_packets), kPacketThreads, 0, nullptr, stage.device<uint8_t>(o_packets), packet_stride, stage.device<double>(o_times),
                      stage.device<double>(o_lasers), d_cos, d_sin, distance_resolution, firing_period, laser_period, d_rec.as<float>(), d_ret.as<int32_t>());
  });
  HIP_TRY(launched);
  HIP_TRY(hipStreamSynchronize(nullptr));
  g_packet_clock.lap(1);

  HIP_TRY(hipMemcpy(records_out, d_rec.as<void>(), record_floats * sizeof(float), hipMemcpyDeviceToHost));
  if (returns_per_packet) HIP_TRY(hipMemcpy(returns_per_packet, d_ret.as<void>(), N * sizeof(int32_t), hipMemcpyDeviceToHost));
  g_packet_clock.lap(2);
  return NIDREG_OK;
}

int nidreg_velodyne_get_timing(double* ms3) { return g_packet_clock.read("nidreg_velodyne_get_timing", ms3); }

}  // extern "C"
