// nid_launch.hpp -- host-visible launch wrappers around the templated kernels.  One precision (double), and every translation
// unit is built with -ffp-contract=off (csrc/Makefile): the fusions wanted are explicit fma calls, and the NEAREST path's
// +,-,*,/,sqrt match the CPU bit for bit.
#pragma once
#include <mutex>

#include "nid_host.hpp"
#include "nid_multi.hpp"

namespace nidreg {

struct Chunk;
struct EntropyScalars;
struct ShardTable;
struct PassArgs {
  int model;
  int rec64;  // 1: Rec64 records (double xyz), 0: Rec32
  const void* pts;
  const Chunk* chunks;
  int nchunks;
  int nslots;  // segments of the gradient pass's table: one 12-double partial each
  int seg;     // the table of THIS launch has chunks that run across column groups: the looped (SEG) kernel instantiations
  const uint32_t* gend;  // end offsets of the column groups among the records (a chunk may run across group boundaries)
  const uint8_t* img;  // padded, edge-replicated bin image
  int pitch, W, H, B, GW, cshift;
  int wide;  // SPLINE histogram pass: the 512-thread / 32-copy single-column specialisation (B = 256, GW = 1)
  double R[9], t[3];  // SPLINE pose
  double iso[12];     // NEAREST pose (rows 0..2 of the 4x4)
  double intr[5], dist[8];
  double magic;     // 2^(frac_bits - 1074): subnormal pre-scale of the x-weights
  double inv_unit;  // 2^(-frac_bits)
  double cos_fov;
  NearestFast nfast;  // NEAREST: the fast decision tier's band coefficients (on = 0: exact tier only); nid_multi.hpp
  unsigned long long* hist;
  const double* phi_q;
  const EntropyScalars* scal;
  double* partials;
  double q[4];          // quaternion of the pose (gradient chain rule)
  double* out;          // device result block
  double* out_host;     // host-mapped mirror (nullable)
  double tag;           // completion tag written behind the results (host polls it)
  unsigned int* counter;  // last-workgroup ticket
  hipStream_t stream;
  size_t lds_hist, lds_grad;
  const MultiEntry* multi;  // non-NULL: one grid over several pairs (chunks / nchunks are then the combined table)
  MultiDyn dyn;
  // the gradient kernel runs the entropy tail itself (k_entropy launched with tail = 0): nid_multi.hpp GradTail.  gt.zero_buf
  // (gt.from_partials == 2): the next evaluation's histogram buffer, cleared by the gradient kernel
  GradTail gt;
  int prio;  // progress priority (s_setprio) in the spline passes: set when the evaluation has its device to itself
};

hipError_t launch_spline_hist(const PassArgs& a);
hipError_t launch_spline_grad(const PassArgs& a);
hipError_t launch_nearest_hist(const PassArgs& a);
// workgroups of the selected kernel instantiation (model, record type, tiling) that fit on one CU at once
// (hipOccupancyMaxActiveBlocksPerMultiprocessor; 0 on error): a pass gets exactly one round of co-resident workgroups
int occupancy_spline_hist(const PassArgs& a);
int occupancy_spline_grad(const PassArgs& a);
int occupancy_nearest_hist(const PassArgs& a);
// ONE launch per cost+Jacobian evaluation (nid_fused.hpp; small tables, grids of co-resident workgroups): a.chunks / a.nchunks =
// the fused table, a.hist = this evaluation's histogram buffer, a.gt.zero_buf the next one's
struct FusedArgs {
  unsigned long long* barrier;         // arrival counter of the grid barrier (device memory, counts over the handle's lifetime)
  unsigned long long barrier_target;   // arrivals once every workgroup of THIS launch has arrived
  unsigned long long* flags;           // one release word per workgroup, kFusedFlagStride (16) words apart
  unsigned long long epoch;            // this launch's number: what the releasing workgroup stores into the flags
  unsigned long long timeout_ticks;    // 100 MHz wall-clock ticks a workgroup waits at the barrier before it gives up
  int cap;                             // points of LDS stash per workgroup (>= the longest chunk)
  int full;                            // 1: (u, v) + projection context + patch + record per point, 0: (u, v) only
};
size_t fused_lds_bytes_for(const PassArgs& a, int full, int cap);
hipError_t launch_spline_fused(const PassArgs& a, const FusedArgs& f);
int occupancy_spline_fused(const PassArgs& a, const FusedArgs& f);  // workgroups of that instantiation per CU (0 on error)
hipError_t launch_project(int model, const double* intr, const double* dist, const double* p3, long long n, double* uv, double* jac, hipStream_t stream);

// the same scalar projection code run on the host (nid_kernels_f64.hip): host arrays, fp64, 0 = ok
int project_host(int model, const double* intr, const double* dist, const double* p3, long long n, double* uv, double* jac);
// vlcal::estimate_direction (estimate_fov.cpp:17-34) over project_host: the bearing of pixel (pu, pv) by NelderMead<2> (nidreg_pose.hip)
void estimate_direction_host(int model, const double* intr5, const double* dist8, double pu, double pv, double* dir3);

// ViewCulling::cull (nid_cull_kernels.hpp); all pointers are device memory
hipError_t launch_cull(int model, const double* intr, const double* dist, const double* d_pts, long long stride_d, long long n, const double* T, int W, int H, double min_z,
                       int depth, int* d_pix, unsigned int* d_zbuf, unsigned char* d_keep, hipStream_t stream);

// the compaction of nidreg_cloud_select behind another flag pass (nidreg_select.hip: k_select_scan, k_select_scatter as they are; null
// stream; all pointers are device memory).  d_count: 3 x ntiles words, the first ntiles the tiles' flagged points; d_offset: ntiles + 3
// words, [ntiles] the total; d_idx_out nullable
hipError_t launch_select_scan(const int* d_count, int ntiles, int* d_offset);
hipError_t launch_select_scatter(const unsigned char* d_flag, const int* d_offset, int ntiles, const double* d_pts, const double* d_int, long long n, int32_t* d_idx_out, double* d_pts_out,
                                 double* d_int_out);

// PointsColorUpdater::update / generate_lidar_image (nid_render_kernels.hpp); all pointers are device memory,
// T = rows of the 4x4 T_camera_lidar
hipError_t launch_colorize(int model, const double* intr, const double* dist, const double* d_pts, long long stride_d, long long n, const double* T, const uint8_t* d_img, int W, int H,
                           double min_nz, const float* d_icolor, double blend_weight, float* d_out, hipStream_t stream);
hipError_t launch_lidar_image(int model, const double* intr, const double* dist, const double* d_pts, long long stride_d, const double* d_intensities, long long n, const double* T, int W,
                              int H, double min_nz, int* d_pix, u64* d_zmin, int* d_index_image, double* d_intensity_image, hipStream_t stream);

// preprocess.cpp:464-473 rank equalisation in place on a device array (nid_build.hip; synchronises the stream)
hipError_t equalize_intensities_device(double* d_intensities, long long n, hipStream_t stream);

// the PointCloud2 route of the voxel integrator in two halves (nidreg_voxel.hip), for a caller that puts its own kernel between them
// (nidreg_odom_deskew_insert): argument checks + upload of the raw records and room for the decoded frame (num_points == 0: nothing
// is staged), then the insert of the num_points x double4 points / num_points x double intensities written there
struct VoxCloud2;
int integrator_stage_cloud2(nidreg_integrator* h, const char* who, const void* data, int64_t num_points, int32_t point_step, int32_t x_offset, int32_t y_offset, int32_t z_offset,
                            int32_t xyz_datatype, int32_t intensity_offset, int32_t intensity_datatype, VoxCloud2* cloud, double4** d_pts, double** d_int);
int integrator_insert_staged(nidreg_integrator* h, const char* who, int64_t num_points, int64_t* num_skipped);
// the grid of the integrator's grid-strided kernels over n items, and a validated sensor_msgs/PointField datatype as a template
// argument (kPcUint8 = 2, kPcUint16 = 4, kPcUint32 = 6, kPcFloat32 = 7, kPcFloat64 = 8: nid_voxel_kernels.hpp)
NIDREG_HIDDEN unsigned vox_grid(int64_t n);
template <typename F>
NIDREG_HIDDEN inline bool with_field_type(int32_t t, F&& f) {
  return with_int<2, 4, 6, 7, 8>(t, f);
}

// view-culling parameters for the device-side record build (all host values; T = rows of the 4x4)
struct CullArgs {
  int model;
  double intr[5], dist[8];
  double T[16];
  int W, H;
  double min_z;
  int depth;
};

// Per-device scratch arena for handle construction: the reference builds a new NIDCost per pair per outer
// iteration (visual_camera_calibration.cpp:199-208), and hipMalloc / hipFree of the temporaries (upload
// staging, sort keys, rocPRIM scratch) used to cost more than the kernels.  One grow-only allocation per
// device, carved linearly; the lock is held for the whole construction (the reference constructs its cost
// objects sequentially).  nidreg_trim() releases it.
class ScratchArena {
 public:
  static ScratchArena& of(int device);
  void lock() { mu_.lock(); }
  void unlock() { mu_.unlock(); }
  hipError_t reserve(size_t bytes);  // grow to >= bytes (invalidates earlier carves), rewinds the cursor
  void* carve(size_t bytes);         // 256-byte aligned; nullptr when the reservation is exhausted
  void release();                    // hipFree (called with the lock held)
 private:
  std::mutex mu_;
  void* base_ = nullptr;
  size_t cap_ = 0, cur_ = 0;
};

// scratch bytes build_records_device carves for n input points (+ a W x H depth buffer when culling)
size_t build_scratch_bytes(long long n, bool cull, int W, int H);

// [cull ->] bucket -> Morton sort -> gather on the device (nid_build.hip).  d_pts: n x 4 doubles (x y z 1),
// cull nullable.  input_order: keep the caller's order inside each column group (stable sort on the group bits
// only) instead of the Morton order.  Temporaries come from `arena` (reserved by the caller for at least
// build_scratch_bytes).  Returns the record buffer (hipMalloc, caller owns: DeviceBuf::adopt), its type, and the column-group offsets.
// Bsrc = the caller's bin count (bin_points = clamp(int(intensity * Bsrc))); d_lut (nullable; bins > 256): occupied bin -> compact bin.
hipError_t build_records_device(
  const double* d_pts, const double* d_intensities, long long n, const CullArgs* cull, int Bsrc, const uint16_t* d_lut, int GW, int NG, bool force_rec32, bool input_order, ScratchArena& arena,
  void** d_recs_out, int* rec64_out, std::vector<int64_t>& gcount, hipStream_t stream);
// float32 cloud ingest (nidreg_cloud_create_f32, nid_build.hip k_cloud_widen): the n records staged at d_src -- x y z at byte
// pt_off + i * pt_stride, the intensity at in_off + i * in_stride (all multiples of 4) -- widened exactly into a cloud's
// d_pts (n x 4 doubles: x y z 1) and d_int (n doubles).  Asynchronous on `stream`.
hipError_t widen_cloud_device(const void* d_src, long long pt_off, long long pt_stride, long long in_off, long long in_stride, long long n, double* d_pts, double* d_int,
                              hipStream_t stream);
// which of the B bins the n device-resident values occupy (used_host: B bytes)
hipError_t mark_bins_device(const double* d_v, long long n, int B, unsigned char* used_host);

// bin image (nid_device.hpp load_patch layout: strips of four rows, padded by 1 left/top and >= 2 right/bottom,
// edge replicated) from the caller's CV_64FC1 / CV_8UC1 image already uploaded to d_src (row stride in bytes)
hipError_t build_bin_image_device(const void* d_src, int is_f64, long long row_stride, int W, int H, int B, const uint16_t* d_lut, int pitch, int nstrips, uint8_t* d_img, hipStream_t stream);

}  // namespace nidreg
