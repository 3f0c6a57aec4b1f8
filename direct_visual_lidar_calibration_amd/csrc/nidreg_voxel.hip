// nidreg_voxel.hip -- C ABI of the voxel integrator (include/nidreg.h: nidreg_integrator_*): vlcal::StaticPointCloudIntegrator
// (src/vlcal/preprocess/static_point_cloud_integrator.cpp:25-62) on the device (kernels: nid_voxel_kernels.hpp).  The handle owns
// the hash table, one frame's upload (and, for the PointCloud2 route, its decoded form) and the per-point slot scratch of one chunk: device memory is O(occupied voxels + one frame).
#include "nid_voxel_kernels.hpp"
#include "nid_las_kernels.hpp"
#include "nid_lzf_host.hpp"
#include "nid_launch.hpp"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

struct nidreg_integrator {
  int device = 0;
  double res = 0.0, min_distance = 0.0;
  int64_t cap = 0;       // slots, a power of two <= kMaxCap
  int64_t size = 0;      // occupied voxels after the last completed insert
  int64_t offered = 0;   // points offered by the accepted inserts so far = the next sequence number
  nidreg::DeviceBuf d_slots;     // VoxSlot[cap]
  nidreg::DeviceBuf d_counters;  // vox_u64[4]: [0] occupied slots, [1..3] k_vox_check's counts / k_vox_compact's cursor
  nidreg::DeviceBuf d_frame;     // the frame being inserted (grow-only)
  size_t frame_bytes = 0;
  nidreg::DeviceBuf d_slot_of;   // unsigned[min(frame, kChunk)] (grow-only)
  int64_t slot_of_cap = 0;
  nidreg::DeviceBuf d_raw;       // nidreg_integrator_insert_cloud2: the message's records as uploaded, a multiple of 16 bytes (grow-only)
  size_t raw_bytes = 0;
};

namespace nidreg {

unsigned vox_grid(int64_t n) { return unsigned(std::max<int64_t>(1, std::min<int64_t>((n + kVoxThreads - 1) / kVoxThreads, kVoxMaxBlocks))); }

namespace {

constexpr int64_t kInitialCap = int64_t(1) << 16;  // 2 MB
constexpr int64_t kMaxCap = int64_t(1) << 31;      // slot numbers are 32-bit (64 GB of table)
constexpr int64_t kChunk = int64_t(1) << 20;       // points per claim / payload launch pair: bounds the slot scratch and how far the table is grown ahead

int64_t pow2_at_least(int64_t v) {
  int64_t c = kInitialCap;
  while (c < v) c <<= 1;
  return c;
}

// a table of at least 2 x `need` slots (load factor <= 1/2 once `need` voxels are in): rehash on the device when the current one is smaller
int vox_reserve(nidreg_integrator* h, int64_t need) {
  if (2 * need <= h->cap) return NIDREG_OK;
  if (2 * need > kMaxCap) return fail(NIDREG_ERR_INVALID, "nidreg_integrator_insert: more than 2^30 voxels");
  const int64_t cap = pow2_at_least(2 * need);
  DeviceBuf fresh;
  HIP_TRY(fresh.alloc(size_t(cap) * sizeof(VoxSlot)));
  HIP_TRY(hipMemsetAsync(fresh.as<void>(), 0, size_t(cap) * sizeof(VoxSlot), nullptr));
  if (h->size > 0) {
    HIP_TRY(launch(k_vox_rehash, vox_grid(h->cap), kVoxThreads, 0, nullptr, h->d_slots.as<VoxSlot>(), h->cap, fresh.as<VoxSlot>(), unsigned(cap - 1)));
    HIP_TRY(hipStreamSynchronize(nullptr));  // the old table is freed below
  }
  h->d_slots = std::move(fresh);
  h->cap = cap;
  return NIDREG_OK;
}

int vox_read_size(nidreg_integrator* h, int64_t* size) {
  vox_u64 v = 0;
  HIP_TRY(hipMemcpy(&v, h->d_counters.as<vox_u64>(), sizeof(v), hipMemcpyDeviceToHost));  // (synchronises the null stream)
  *size = int64_t(v);
  return NIDREG_OK;
}

// what the insert routes share once the frame sits in h->d_frame: the check pass, then claim + payload per chunk.  num_skipped
// (nidreg_integrator_insert_cloud2): a point with a non-finite coordinate does not refuse the frame; it takes its sequence number,
// claims nothing (k_vox_claim inserts kVoxOk points only) and is counted there.
template <typename Frame>
int vox_insert(nidreg_integrator* h, const char* who, const Frame& frame, int64_t n, int64_t* num_skipped = nullptr) {
  vox_u64* const d_cnt = h->d_counters.as<vox_u64>();
  HIP_TRY(hipMemsetAsync(d_cnt + 1, 0, 3 * sizeof(vox_u64), nullptr));
  HIP_TRY(launch(k_vox_check<Frame>, vox_grid(n), kVoxThreads, 0, nullptr, frame, n, h->res, h->min_distance, d_cnt));
  vox_u64 cnt[4];
  HIP_TRY(hipMemcpy(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost));
  if (num_skipped) {
    *num_skipped = int64_t(cnt[1]);
    if (cnt[2]) {
      char msg[512];
      std::snprintf(msg, sizeof(msg),
                    "%s: %llu point(s) outside the packed-key limit (the voxel index floor(coordinate / voxel_resolution) must lie in [-1048576, 1048576) on every axis: "
                    "|coordinate| < %g at voxel_resolution %g); nothing was inserted",
                    who, cnt[2], double(kVoxAxisLimit) * h->res, h->res);
      return fail(NIDREG_ERR_INVALID, msg);
    }
  } else if (cnt[1] || cnt[2]) {
    char msg[512];
    std::snprintf(msg, sizeof(msg),
                  "%s: %llu point(s) with a non-finite coordinate, %llu point(s) outside the packed-key limit (the voxel index floor(coordinate / voxel_resolution) must lie in "
                  "[-1048576, 1048576) on every axis: |coordinate| < %g at voxel_resolution %g); nothing was inserted",
                  who, cnt[1], cnt[2], double(kVoxAxisLimit) * h->res, h->res);
    return fail(NIDREG_ERR_INVALID, msg);
  }
  if (h->slot_of_cap < std::min(n, kChunk)) {
    HIP_TRY(h->d_slot_of.alloc(size_t(std::min(n, kChunk)) * sizeof(unsigned)));
    h->slot_of_cap = std::min(n, kChunk);
  }
  int64_t size_bound = h->size;  // occupied slots, or an upper bound of them while the chunks run without a read-back
  for (int64_t i0 = 0; i0 < n; i0 += kChunk) {
    const int64_t m = std::min(kChunk, n - i0);
    if (2 * (size_bound + m) > h->cap) {
      if (const int rc = vox_read_size(h, &h->size)) return rc;
      size_bound = h->size;
      if (const int rc = vox_reserve(h, size_bound + m)) return rc;
    }
    const vox_u64 seq0 = vox_u64(h->offered + i0);
    HIP_TRY(launch(k_vox_claim<Frame>, vox_grid(m), kVoxThreads, 0, nullptr, frame, i0, m, seq0, h->res, h->min_distance, h->d_slots.as<VoxSlot>(), unsigned(h->cap - 1),
                   h->d_slot_of.as<unsigned>(), d_cnt));
    HIP_TRY(launch(k_vox_payload<Frame>, vox_grid(m), kVoxThreads, 0, nullptr, frame, i0, m, seq0, h->d_slots.as<VoxSlot>(), h->d_slot_of.as<unsigned>()));
    size_bound += m;
  }
  if (const int rc = vox_read_size(h, &h->size)) return rc;
  h->offered += n;
  return NIDREG_OK;
}

int vox_frame_room(nidreg_integrator* h, size_t bytes) {
  if (h->frame_bytes >= bytes) return NIDREG_OK;
  HIP_TRY(h->d_frame.alloc(bytes));
  h->frame_bytes = bytes;
  return NIDREG_OK;
}

// sensor_msgs/PointField datatype -> bytes; 0 = not a type the route reads
int cloud2_type_bytes(int32_t t) { return t == kPcUint8 ? 1 : t == kPcUint16 ? 2 : (t == kPcUint32 || t == kPcFloat32) ? 4 : t == kPcFloat64 ? 8 : 0; }

// the decode kernel of the PointCloud2 route for the field types integrator_stage_cloud2 has accepted, staged or not by the step
hipError_t cloud2_launch(const VoxCloud2& c, int32_t xyz_datatype, int32_t intensity_datatype, double4* pts, double* inten) {
  hipError_t e = hipErrorInvalidValue;
  with_int<kPcFloat32, kPcFloat64>(xyz_datatype, [&](auto X) {
    with_field_type(intensity_datatype, [&](auto I) {
      with_bool(c.step <= kVoxStageStep, [&](auto STAGED) { e = launch(k_vox_decode_cloud2<X, I, STAGED>, vox_grid(c.n), kVoxThreads, 0, nullptr, c, pts, inten); });
    });
  });
  return e;
}

}  // namespace

// the two halves of the PointCloud2 route around the decode kernel, shared with nidreg_odom_deskew_insert (nidreg_odom.hip): the
// argument checks and the upload of the records as they lie in the message ...
int integrator_stage_cloud2(nidreg_integrator* h, const char* who, const void* data, int64_t num_points, int32_t point_step, int32_t x_offset, int32_t y_offset, int32_t z_offset,
                            int32_t xyz_datatype, int32_t intensity_offset, int32_t intensity_datatype, VoxCloud2* cloud, double4** d_pts_out, double** d_int_out) {
  if (!h) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null integrator");
  if (num_points < 0 || (num_points > 0 && !data)) return fail(NIDREG_ERR_INVALID, std::string(who) + ": negative num_points or null data");
  if (point_step < 1 || point_step > 65535) return fail(NIDREG_ERR_INVALID, std::string(who) + ": point_step must lie in 1..65535");
  if (xyz_datatype != kPcFloat32 && xyz_datatype != kPcFloat64)
    return fail(NIDREG_ERR_INVALID, std::string(who) + ": x, y and z must all be FLOAT32 (7) or all FLOAT64 (8), got datatype " + std::to_string(xyz_datatype));
  const int xyz_bytes = cloud2_type_bytes(xyz_datatype), int_bytes = cloud2_type_bytes(intensity_datatype);
  if (!int_bytes) return fail(NIDREG_ERR_INVALID, std::string(who) + ": the intensity must be UINT8, UINT16, UINT32, FLOAT32 or FLOAT64, got datatype " + std::to_string(intensity_datatype));
  for (const int32_t off : {x_offset, y_offset, z_offset})
    if (off < 0 || off > point_step - xyz_bytes) return fail(NIDREG_ERR_INVALID, std::string(who) + ": a coordinate field lies outside the point_step bytes of a record");
  if (intensity_offset < 0 || intensity_offset > point_step - int_bytes) return fail(NIDREG_ERR_INVALID, std::string(who) + ": the intensity field lies outside the point_step bytes of a record");
  if (num_points == 0) return NIDREG_OK;
  if (num_points > INT64_MAX / 65535) return fail(NIDREG_ERR_INVALID, std::string(who) + ": num_points x point_step overflows");
  HIP_TRY(hipSetDevice(h->device));
  const size_t bytes = size_t(num_points) * size_t(point_step);
  const size_t room = (bytes + 15) & ~size_t(15);  // the staging loads of k_vox_decode_cloud2 end on a 16-byte boundary
  if (h->raw_bytes < room) {
    HIP_TRY(h->d_raw.alloc(room));
    h->raw_bytes = room;
  }
  if (const int rc = vox_frame_room(h, size_t(num_points) * 40)) return rc;
  HIP_TRY(hipMemcpy(h->d_raw.as<void>(), data, bytes, hipMemcpyHostToDevice));  // the records as they lie in the message
  unsigned char* const d = h->d_frame.as<unsigned char>();
  *d_pts_out = reinterpret_cast<double4*>(d);
  *d_int_out = reinterpret_cast<double*>(d + size_t(num_points) * 32);
  *cloud = VoxCloud2{h->d_raw.as<const unsigned char>(), (long long)num_points, point_step, x_offset, y_offset, z_offset, intensity_offset};
  return NIDREG_OK;
}

// ... and the insert of the double frame a kernel has written where integrator_stage_cloud2 said
int integrator_insert_staged(nidreg_integrator* h, const char* who, int64_t num_points, int64_t* num_skipped) {
  unsigned char* const d = h->d_frame.as<unsigned char>();
  int64_t skipped = 0;
  const int rc = vox_insert(h, who, VoxFrameF64{reinterpret_cast<const double4*>(d), reinterpret_cast<const double*>(d + size_t(num_points) * 32)}, num_points, &skipped);
  if (num_skipped) *num_skipped = skipped;
  return rc;
}

}  // namespace nidreg

using namespace nidreg;

extern "C" {

int nidreg_integrator_create(int device_id, double voxel_resolution, double min_distance, nidreg_integrator** out) {
  if (!out) return fail(NIDREG_ERR_INVALID, "nidreg_integrator_create: null out");
  *out = nullptr;
  if (!(voxel_resolution > 0.0) || !std::isfinite(voxel_resolution)) return fail(NIDREG_ERR_INVALID, "nidreg_integrator_create: voxel_resolution must be positive and finite");
  if (std::isnan(min_distance)) return fail(NIDREG_ERR_INVALID, "nidreg_integrator_create: min_distance is NaN");
  if (device_id < 0) return fail(NIDREG_ERR_INVALID, "nidreg_integrator_create: device_id out of range");
  if (const int rc = use_device("nidreg_integrator_create", device_id)) return rc;
  std::unique_ptr<nidreg_integrator> h(new nidreg_integrator());
  h->device = device_id;
  h->res = voxel_resolution;
  h->min_distance = min_distance;
  h->cap = kInitialCap;
  HIP_TRY(h->d_slots.alloc(size_t(h->cap) * sizeof(VoxSlot)));
  HIP_TRY(h->d_counters.alloc(4 * sizeof(vox_u64)));
  HIP_TRY(hipMemsetAsync(h->d_slots.as<void>(), 0, size_t(h->cap) * sizeof(VoxSlot), nullptr));
  HIP_TRY(hipMemsetAsync(h->d_counters.as<void>(), 0, 4 * sizeof(vox_u64), nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  *out = h.release();
  return NIDREG_OK;
}

int nidreg_integrator_insert(nidreg_integrator* h, const double* points, int64_t point_stride, const double* intensities, int64_t n) {
  if (!h) return fail(NIDREG_ERR_INVALID, "nidreg_integrator_insert: null integrator");
  if (n < 0 || (n > 0 && (!points || !intensities))) return fail(NIDREG_ERR_INVALID, "nidreg_integrator_insert: negative n or null points / intensities");
  if (n == 0) return NIDREG_OK;
  const int64_t stride = point_stride > 0 ? point_stride : 32;
  if (stride < 24 || stride % 8 || reinterpret_cast<uintptr_t>(points) % 8 || reinterpret_cast<uintptr_t>(intensities) % 8)
    return fail(NIDREG_ERR_INVALID, "nidreg_integrator_insert: point_stride must be >= 24 bytes, strides and pointers 8-byte aligned");
  if (stride > INT64_MAX / n) return fail(NIDREG_ERR_INVALID, "nidreg_integrator_insert: stride x n overflows");
  HIP_TRY(hipSetDevice(h->device));
  // device frame: n points of 32 bytes (x y z and an unused fourth double), then n intensities
  if (const int rc = vox_frame_room(h, size_t(n) * 40)) return rc;
  unsigned char* const d = h->d_frame.as<unsigned char>();
  if (stride == 32) {
    HIP_TRY(hipMemcpy(d, points, size_t(n) * 32, hipMemcpyHostToDevice));
  } else {
    HIP_TRY(hipMemcpy2D(d, 32, points, size_t(stride), size_t(std::min<int64_t>(stride, 32)), size_t(n), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(d + size_t(n) * 32, intensities, size_t(n) * 8, hipMemcpyHostToDevice));
  const VoxFrameF64 frame{reinterpret_cast<const double4*>(d), reinterpret_cast<const double*>(d + size_t(n) * 32)};
  return vox_insert(h, "nidreg_integrator_insert", frame, n);
}

int nidreg_integrator_insert_f32(nidreg_integrator* h, const float* points, int64_t point_stride, const float* intensities, int64_t intensity_stride, int64_t n) {
  if (!h) return fail(NIDREG_ERR_INVALID, "nidreg_integrator_insert_f32: null integrator");
  if (n < 0 || (n > 0 && (!points || !intensities))) return fail(NIDREG_ERR_INVALID, "nidreg_integrator_insert_f32: negative n or null points / intensities");
  if (n == 0) return NIDREG_OK;
  if (point_stride < 12 || intensity_stride < 4) return fail(NIDREG_ERR_INVALID, "nidreg_integrator_insert_f32: point_stride must be >= 12 and intensity_stride >= 4 bytes");
  if (point_stride % 4 || intensity_stride % 4 || reinterpret_cast<uintptr_t>(points) % 4 || reinterpret_cast<uintptr_t>(intensities) % 4)
    return fail(NIDREG_ERR_INVALID, "nidreg_integrator_insert_f32: strides and pointers must be 4-byte aligned");
  if (point_stride > INT64_MAX / n || intensity_stride > INT64_MAX / n) return fail(NIDREG_ERR_INVALID, "nidreg_integrator_insert_f32: stride x n overflows");
  HIP_TRY(hipSetDevice(h->device));
  if (const int rc = vox_frame_room(h, size_t(n) * 16)) return rc;
  // the stored PLY record (x y z intensity, 16 bytes) is uploaded as it lies; any other layout is packed into it on the host first
  if (point_stride == 16 && intensity_stride == 16 && intensities == points + 3) {
    HIP_TRY(hipMemcpy(h->d_frame.as<void>(), points, size_t(n) * 16, hipMemcpyHostToDevice));
  } else {
    std::vector<float> packed(size_t(n) * 4);
    const unsigned char* p = reinterpret_cast<const unsigned char*>(points);
    const unsigned char* q = reinterpret_cast<const unsigned char*>(intensities);
    for (int64_t i = 0; i < n; i++) {
      std::memcpy(&packed[size_t(i) * 4], p + i * point_stride, 12);
      std::memcpy(&packed[size_t(i) * 4 + 3], q + i * intensity_stride, 4);
    }
    HIP_TRY(hipMemcpy(h->d_frame.as<void>(), packed.data(), size_t(n) * 16, hipMemcpyHostToDevice));
  }
  const VoxFrameF32 frame{h->d_frame.as<const float4>()};
  return vox_insert(h, "nidreg_integrator_insert_f32", frame, n);
}

int nidreg_integrator_insert_cloud2(nidreg_integrator* h, const void* data, int64_t num_points, int32_t point_step, int32_t x_offset, int32_t y_offset, int32_t z_offset, int32_t xyz_datatype,
                                    int32_t intensity_offset, int32_t intensity_datatype, int64_t* num_skipped) {
  const char* const who = "nidreg_integrator_insert_cloud2";
  if (num_skipped) *num_skipped = 0;
  VoxCloud2 c;
  double4* d_pts = nullptr;
  double* d_int = nullptr;
  if (const int rc = integrator_stage_cloud2(h, who, data, num_points, point_step, x_offset, y_offset, z_offset, xyz_datatype, intensity_offset, intensity_datatype, &c, &d_pts, &d_int)) return rc;
  if (num_points == 0) return NIDREG_OK;
  HIP_TRY(cloud2_launch(c, xyz_datatype, intensity_datatype, d_pts, d_int));
  return integrator_insert_staged(h, who, num_points, num_skipped);
}

// host wall-clock milliseconds of the calling thread's last nidreg_integrator_insert_las: checks + allocation + upload, decode kernel
// (launch to idle), the integrator's passes
static thread_local PhaseClock<3> g_las_clock;

// LAS point formats 0..10: the base record length, and where the red channel lies (0 = the format has no RGB)
static const int kLasBaseLength[11] = {20, 28, 26, 34, 57, 63, 30, 36, 38, 59, 67};
static const int kLasRgbOffset[11] = {0, 0, 20, 28, 0, 28, 0, 30, 30, 0, 30};

int nidreg_integrator_insert_las(nidreg_integrator* h, const void* records, int64_t num_points, int32_t record_length, int32_t point_format, const double* scale3, const double* offset3,
                                 const double* origin3, int32_t intensity_source, const uint64_t* exclude_classes4, int32_t keep_withheld, int64_t* num_skipped) {
  const std::string who = "nidreg_integrator_insert_las";
  if (num_skipped) *num_skipped = 0;
  g_las_clock.clear();
  g_las_clock.start();
  // every check of the arguments themselves comes before the handle is looked at, and all of it before the device is touched
  if (point_format < 0 || point_format > 10) return fail(NIDREG_ERR_INVALID, who + ": point formats 0..10 are read, got " + std::to_string(point_format));
  if (record_length < kLasBaseLength[point_format] || record_length > 65535)
    return fail(NIDREG_ERR_INVALID, who + ": record_length " + std::to_string(record_length) + " is outside " + std::to_string(kLasBaseLength[point_format]) + "..65535, the range of point format " +
                                        std::to_string(point_format));
  if (!scale3 || !offset3 || !origin3) return fail(NIDREG_ERR_INVALID, who + ": null scale3, offset3 or origin3");
  for (int a = 0; a < 3; a++) {
    if (!std::isfinite(scale3[a]) || scale3[a] == 0.0) return fail(NIDREG_ERR_INVALID, who + ": a scale must be finite and not zero, got " + std::to_string(scale3[a]));
    if (!std::isfinite(offset3[a]) || !std::isfinite(origin3[a])) return fail(NIDREG_ERR_INVALID, who + ": a non-finite offset or origin");
  }
  if (intensity_source != 0 && intensity_source != 1) return fail(NIDREG_ERR_INVALID, who + ": intensity_source must be 0 (intensity) or 1 (rgb), got " + std::to_string(intensity_source));
  if (intensity_source == 1 && !kLasRgbOffset[point_format]) return fail(NIDREG_ERR_INVALID, who + ": rgb intensity asked of point format " + std::to_string(point_format) + ", which has no RGB channels");
  if (num_points < 0 || (num_points > 0 && !records)) return fail(NIDREG_ERR_INVALID, who + ": negative num_points or null records");
  // the handle, the upload of the records as they lie in the file and the frame's room: the PointCloud2 route's first half, told
  // the truth about the record -- three 4-byte coordinates at 0, 4, 8 and a 16-bit intensity at 12
  VoxCloud2 c;
  double4* d_pts = nullptr;
  double* d_int = nullptr;
  if (const int rc = integrator_stage_cloud2(h, who.c_str(), records, num_points, record_length, 0, 4, 8, kPcFloat32, 12, kPcUint16, &c, &d_pts, &d_int)) return rc;
  if (num_points == 0) return NIDREG_OK;
  g_las_clock.lap(0);
  const bool modern = point_format >= 6;
  VoxLas las;
  las.raw = c.raw, las.n = c.n, las.step = c.step;
  las.o_rgb = intensity_source == 1 ? kLasRgbOffset[point_format] : -1;
  las.o_class = modern ? 16 : 15;
  las.class_bits = modern ? 0xffu : 0x1fu;
  las.withheld_drop = keep_withheld ? 0u : (modern ? 0x04u : 0x80u);
  las.sx = scale3[0], las.sy = scale3[1], las.sz = scale3[2];
  las.ox = offset3[0], las.oy = offset3[1], las.oz = offset3[2];
  las.gx = origin3[0], las.gy = origin3[1], las.gz = origin3[2];
  vox_u64 m[4] = {0, 0, 0, 0};
  if (exclude_classes4)
    for (int k = 0; k < 4; k++) m[k] = vox_u64(exclude_classes4[k]);
  HIP_TRY(with_bool(record_length <= kVoxStageStep, [&](auto STAGED) {
    return launch(k_vox_decode_las<STAGED>, vox_grid(num_points), kVoxThreads, 0, nullptr, las, m[0], m[1], m[2], m[3], d_pts, d_int);
  }));
  HIP_TRY(hipStreamSynchronize(nullptr));  // (the check pass that follows reads its counters back, so the insert waits here anyway: this only splits the clock)
  g_las_clock.lap(1);
  const int rc = integrator_insert_staged(h, who.c_str(), num_points, num_skipped);
  g_las_clock.lap(2);
  return rc;
}

int nidreg_integrator_las_timing(double* ms3) { return g_las_clock.read("nidreg_integrator_las_timing", ms3, "ms3"); }

int nidreg_lzf_decompress(const uint8_t* in, int64_t in_size, uint8_t* out, int64_t out_size, int64_t* written) {
  if (written) *written = 0;
  if (in_size < 0 || out_size < 0 || (in_size > 0 && !in) || (out_size > 0 && !out)) return fail(NIDREG_ERR_INVALID, "nidreg_lzf_decompress: negative size or null buffer");
  size_t got = 0;
  std::string reason;
  const bool ok = nidlzf::decompress(in, size_t(in_size), out, size_t(out_size), got, reason);
  if (written) *written = int64_t(got);
  return ok ? NIDREG_OK : fail(NIDREG_ERR_INVALID, "nidreg_lzf_decompress: " + reason);
}

int nidreg_integrator_size(nidreg_integrator* h, int64_t* num_voxels) {
  if (!h || !num_voxels) return fail(NIDREG_ERR_INVALID, "nidreg_integrator_size: null argument");
  *num_voxels = h->size;
  return NIDREG_OK;
}

int nidreg_integrator_info(nidreg_integrator* h, int64_t* info4) {
  if (!h || !info4) return fail(NIDREG_ERR_INVALID, "nidreg_integrator_info: null argument");
  info4[0] = h->size, info4[1] = h->cap, info4[2] = h->offered, info4[3] = int64_t(sizeof(VoxSlot));
  return NIDREG_OK;
}

int nidreg_integrator_get(nidreg_integrator* h, float* records16, int64_t* seq) {
  if (!h) return fail(NIDREG_ERR_INVALID, "nidreg_integrator_get: null integrator");
  const int64_t m = h->size;
  if (m == 0) return NIDREG_OK;
  if (!records16) return fail(NIDREG_ERR_INVALID, "nidreg_integrator_get: null records16");
  HIP_TRY(hipSetDevice(h->device));
  const size_t sm = size_t(m);
  int end_bit = 1;
  while (end_bit < 64 && (vox_u64(h->offered) >> end_bit) != 0) end_bit++;  // keys are sequence numbers + 1 <= offered
  DeviceBuf d_keys, d_keys2, d_vals, d_vals2, d_tmp, d_out;
  HIP_TRY(d_keys.alloc(sm * 8));
  HIP_TRY(d_keys2.alloc(sm * 8));
  HIP_TRY(d_vals.alloc(sm * 4));
  HIP_TRY(d_vals2.alloc(sm * 4));
  HIP_TRY(d_out.alloc(sm * 24));  // m records, then m sequence numbers
  vox_u64* const cursor = h->d_counters.as<vox_u64>() + 3;
  HIP_TRY(hipMemsetAsync(cursor, 0, sizeof(vox_u64), nullptr));
  HIP_TRY(launch(k_vox_compact, vox_grid(h->cap), kVoxThreads, 0, nullptr, h->d_slots.as<const VoxSlot>(), h->cap, cursor, d_keys.as<vox_u64>(), d_vals.as<unsigned>()));
  size_t tmp_bytes = 0;
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp_bytes, d_keys.as<vox_u64>(), d_keys2.as<vox_u64>(), d_vals.as<unsigned>(), d_vals2.as<unsigned>(), sm, 0, unsigned(end_bit), hipStream_t(nullptr)));
  HIP_TRY(d_tmp.alloc(std::max<size_t>(tmp_bytes, 1)));
  HIP_TRY(rocprim::radix_sort_pairs(d_tmp.as<void>(), tmp_bytes, d_keys.as<vox_u64>(), d_keys2.as<vox_u64>(), d_vals.as<unsigned>(), d_vals2.as<unsigned>(), sm, 0, unsigned(end_bit), hipStream_t(nullptr)));
  float4* const d_rec = d_out.as<float4>();
  long long* const d_seq = reinterpret_cast<long long*>(d_out.as<unsigned char>() + sm * 16);
  HIP_TRY(launch(k_vox_gather, vox_grid(m), kVoxThreads, 0, nullptr, h->d_slots.as<const VoxSlot>(), d_keys2.as<const vox_u64>(), d_vals2.as<const unsigned>(), m, d_rec, d_seq));
  HIP_TRY(hipMemcpy(records16, d_rec, sm * 16, hipMemcpyDeviceToHost));
  if (seq) HIP_TRY(hipMemcpy(seq, d_seq, sm * 8, hipMemcpyDeviceToHost));
  return NIDREG_OK;
}

void nidreg_integrator_destroy(nidreg_integrator* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(nullptr);
  delete h;
}

}  // extern "C"
