/*
 * nidreg.h -- C ABI of the MI355X-native NID direct LiDAR-camera registration core.
 *
 * This is the drop-in boundary for the hot path of koide3/direct_visual_lidar_calibration's
 * `calibrate`: everything behind these entry points runs as hand-written HIP kernels on gfx950
 * (direct_visual_lidar_calibration_amd/csrc/).  Plain pointers and sizes only; no C++/torch types.
 *
 * Reference interfaces each entry point replaces (paths relative to the reference tree):
 *   nidreg_model_from_name   camera::create_camera model strings + parameter counts
 *                            (src/camera/create_camera.cpp:17-51)
 *   nidreg_create            vlcal::NIDCost::NIDCost           (include/vlcal/costs/nid_cost.hpp:23-34)
 *                            vlcal::CostCalculatorNID ctor     (src/vlcal/calib/cost_calculator_nid.cpp:13-17)
 *   nidreg_eval              NIDCost::operator()<double | ceres::Jet<double,7>>
 *                                                              (include/vlcal/costs/nid_cost.hpp:36-107)
 *   nidreg_eval_iso          CostCalculatorNID::calculate      (src/vlcal/calib/cost_calculator_nid.cpp:21-67)
 *   nidreg_eval_multi        MultiNIDCost::operator()          (src/vlcal/calib/visual_camera_calibration.cpp:147-173)
 *   nidreg_eval_iso_multi    the Nelder-Mead objective's sum over pairs
 *                                                              (src/vlcal/calib/visual_camera_calibration.cpp:103-119)
 *   nidreg_project           GenericCameraBase::project        (include/camera/generic_camera_base.hpp:29)
 *   nidreg_view_culling      ViewCulling::cull                 (src/vlcal/calib/view_culling.cpp:21-92)
 *   nidreg_colorizer_*       vlcal::PointsColorUpdater         (src/vlcal/common/points_color_updater.cpp:26-61)
 *   nidreg_generate_lidar_image  vlcal::generate_lidar_image   (src/vlcal/preprocess/generate_lidar_image.cpp:7-41)
 *   nidreg_equalize_intensities  the rank equalisation loop    (src/vlcal/preprocess/preprocess.cpp:464-473)
 *   nidreg_shard_*           (no reference counterpart) split-phase evaluation of one pair whose
 *                            points are sharded over several GPUs, ONE PROCESS PER GPU; the caller
 *                            all-reduces the fixed-point histogram (RCCL) between the phases.
 *   desc.num_devices /       (no reference counterpart) one pair over several GPUs inside ONE process: nidreg_create /
 *   NIDREG_DEVICES           nidreg_create_from_cloud cut the cloud along the histogram column (every GPU owns a range of
 *                            column groups and the points that fall into them) and every GPU stores its columns of the
 *                            integer histogram into every other GPU's replica, once per evaluation (the reference's calibrate is a
 *                            single process, src/calibrate.cpp:117-120)
 *   nidreg_cloud_create_f32  the float32 cloud as stored: preprocess.cpp writes x y z intensity as four floats per
 *                            vertex (src/vlcal/preprocess/preprocess.cpp:161-169); VisualLiDARData widens them to
 *                            doubles on the host after loading (src/vlcal/common/visual_lidar_data.cpp:19-26) --
 *                            here the floats are uploaded and widened on the GPU
 *   nidreg_mask_*,           (no reference counterpart: its users edit the PNG or the PLY by hand) image regions and LiDAR
 *   nidreg_cloud_select      ranges left out of the cost: the cull, an eroded 8-bit mask at the point's pixel and a range gate,
 *                            compacted on the device into a new cloud
 *   nidreg_cloud_fold*       (no reference counterpart) a hashed fold of a cloud, per point or per spatial block, or its complement,
 *                            compacted on the device into a new cloud: the subsets `evaluate` recalibrates on
 *   nidreg_estimate_directions   vlcal::estimate_direction per keypoint (src/vlcal/common/estimate_fov.cpp:17-34; the loop of
 *                            src/vlcal/common/estimate_pose.cpp:46-51)
 *   nidreg_estimate_rotation_ransac  PoseEstimation::estimate_rotation_ransac, the hypothesis loop and the inlier flags
 *                            (src/vlcal/common/estimate_pose.cpp:53-145)
 *   nidreg_ransac_sample_pairs   (no reference counterpart) the hypotheses' sampler on the host; replaces the per-thread
 *                            mt19937 streams of src/vlcal/common/estimate_pose.cpp:90-108
 *   nidreg_integrator_*      vlcal::StaticPointCloudIntegrator, insert_points / get_points
 *                            (src/vlcal/preprocess/static_point_cloud_integrator.cpp:25-62)
 *   nidreg_odom_*            vlcal::DynamicPointCloudIntegrator: kNN covariances, the iVox model, CT-GICP linearise / error, deskewed insert
 *                            (src/vlcal/preprocess/dynamic_point_cloud_integrator.cpp:50-155)
 *   nidreg_destroy           ~NIDCost / ~CostCalculatorNID
 *
 * Conventions
 *   - return value: 0 = ok; NIDREG_FALSE (1) = the functor's `return false` (non-finite NID,
 *     nid_cost.hpp:98-102, or the 0.2 m / 2 deg trust gate, visual_camera_calibration.cpp:154);
 *     < 0 = error (nidreg_last_error() gives the text for the calling thread).
 *   - pose for nidreg_eval*: Sophus SE3d::data() order [qx qy qz qw tx ty tz] = T_camera_lidar,
 *     quaternion NOT re-normalised (the reference differentiates the un-normalised formula).
 *     The 7-gradient returned is the ambient Jet gradient d NID / d [qx qy qz qw tx ty tz].
 *   - pose for nidreg_eval_iso*: row-major 4x4 T_camera_lidar (Eigen::Isometry3d::matrix()).
 *   - histograms handed back are row-major [bin_image][bin_points] like `hist(bin_image, bin_points)`.
 *   - threading: concurrent calls on DIFFERENT handles from different host threads are safe (the
 *     reference evaluates one NIDCost per OpenMP thread, visual_camera_calibration.cpp:161);
 *     concurrent calls on the same handle are not supported (never happens in the reference).
 *     Handles sharded over several GPUs are evaluated one after the other on every device they share
 *     (a per-device lock inside nidreg_eval*: each of them uses all of its GPUs anyway).
 *   - an evaluation that has its device to itself runs with issue priority by progress in the two streaming kernels;
 *     evaluations that share a device (concurrent callers) run without it.  The cost and the histograms do not depend
 *     on it, nor on the chunk tables or the GPU count (fixed-point histogram, fixed-point entropy sums: bit-identical);
 *     the gradient is equal up to the order of the workgroup partials, which is a fixed function of the handle.
 *   - NEAREST handles (nidreg_eval_iso*): the integer histogram is the reference's, count for count, for every point whose
 *     decisions (inside the FoV cone, inside the image, which pixel) the arithmetic fixes -- +, -, *, /, sqrt follow the
 *     reference's expression order without contraction.  Three camera models put a libm function between the point and its
 *     pixel (fisheye, atan: atan2 / atan; equirectangular: asin, atan2): there the pixel is exact up to the last place in which
 *     the device's libm and the host's agree, i.e. a point within ~3e-14 px of a pixel boundary may fall on either side
 *     (two CPU builds with different libms disagree in the same way); none of the 10^7 points of the full-size test clouds does.
 *   - the caller keeps ownership of every host buffer; nidreg_create copies what it needs.
 */
#ifndef NIDREG_H
#define NIDREG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NIDREG_OK 0
#define NIDREG_FALSE 1
#define NIDREG_ERR_INVALID (-1)     /* bad argument / unsupported configuration */
#define NIDREG_ERR_HIP (-2)         /* HIP runtime error */
#define NIDREG_ERR_NO_DEVICE (-3)   /* no usable gfx950 device */
#define NIDREG_ERR_FULL (-4)        /* a fixed-size device pool is exhausted (nidreg_odom_model_insert) */

/* camera models (create_camera.cpp:34-51) */
#define NIDREG_MODEL_PLUMB_BOB 0            /* "plumb_bob": 4 intrinsics, 5 distortion (k1 k2 p1 p2 k3) */
#define NIDREG_MODEL_FISHEYE 1              /* "fisheye" | "equidistant": 4 + 4 */
#define NIDREG_MODEL_OMNIDIR 2              /* "omnidir": 5 (fx fy cx cy xi) + 4 */
#define NIDREG_MODEL_EQUIRECTANGULAR 3      /* "equirectangular": 2 (W H) + 0 */
#define NIDREG_MODEL_ATAN 4                 /* "atan": 4 + 1 */
#define NIDREG_MODEL_RATIONAL_POLYNOMIAL 5  /* "rational_polynomial": 4 + 8 (k1 k2 p1 p2 k3 k4 k5 k6) */

/* which reference functor the handle implements */
#define NIDREG_MODE_SPLINE 0   /* NIDCost: B-spline soft assignment, value + Jacobian */
#define NIDREG_MODE_NEAREST 1  /* CostCalculatorNID: FoV gate + nearest pixel, integer histogram */

/* per-point arithmetic */
#define NIDREG_PREC_FP64 0  /* transform / projection / weights in double (parity mode) */
#define NIDREG_PREC_FP32 1  /* REMOVED (round 5): float transform / projection bought 8 % for |dNID| <= 2e-5; refused with NIDREG_ERR_INVALID */

#define NIDREG_IMAGE_F64 0  /* CV_64FC1 normalised to [0,1] (what NIDCost receives) */
#define NIDREG_IMAGE_U8 1   /* CV_8UC1 (what CostCalculatorNID receives) */

/* nidreg_desc.bins: 2 .. NIDREG_MAX_BINS_WIDE, like the reference's `const int bins` (nid_cost.hpp:23, --nid_bins of
 * src/calibrate.cpp:175).  The kernels hold NIDREG_MAX_BINS bins per axis; more are accepted while at most NIDREG_MAX_BINS of
 * them are OCCUPIED on each axis -- always the case for the reference's own data path (8-bit camera images,
 * visual_camera_calibration.cpp:204; intensities rank-equalised to 256 levels, preprocess.cpp:464-473).  The NID and its
 * gradient depend on the multiset of histogram cells and on the marginals only, so the handle runs on the occupied bins,
 * relabelled 0, 1, 2, ... (same cost, same gradient), and nidreg_get_hist* expand them back to the caller's layout.  An input
 * that occupies more than 256 bins on an axis is refused with NIDREG_ERR_INVALID (never truncated). */
#define NIDREG_MAX_BINS 256
#define NIDREG_MAX_BINS_WIDE 4096
#define NIDREG_MAX_DEVICES 16

/* nidreg_desc.flags */
#define NIDREG_FLAG_EXT_STREAM 2  /* launch on desc.ext_stream even when it is NULL (= the legacy default
                                     stream, e.g. torch's current stream); otherwise NULL means "own stream" */
#define NIDREG_FLAG_NEAREST_EXACT 4 /* NEAREST handles: every point through the exact decision tier (the reference's expression
                                     order), none through the fast one -- for A/B runs and bisecting; the environment variable
                                     NIDREG_NEAREST_EXACT=1 does the same for every handle of the process */
#define NIDREG_FLAG_INPUT_ORDER 1 /* keep the caller's point order inside each column group instead of the
                                     default Morton order of the LiDAR-frame bearing (results are
                                     bit-identical either way; the default gathers ~2x faster) */

typedef struct nidreg_handle nidreg_handle;

typedef struct nidreg_desc {
  int32_t struct_size;      /* sizeof(nidreg_desc), for forward compatibility */
  int32_t device_id;        /* HIP device ordinal */
  int32_t model_id;         /* NIDREG_MODEL_* */
  int32_t mode;             /* NIDREG_MODE_* */
  int32_t precision;        /* NIDREG_PREC_* */
  int32_t bins;             /* nid_bins, 2..NIDREG_MAX_BINS_WIDE (4096), see above: beyond NIDREG_MAX_BINS (256) the handle runs on the
                               OCCUPIED bins (the reference's data path quantises both inputs to 256 levels: 8-bit images,
                               visual_camera_calibration.cpp:204; intensities equalised to floor(256 i / n) / 256, preprocess.cpp:464-473);
                               an input that occupies more than 256 bins on an axis, or bins outside the range, is REFUSED with
                               NIDREG_ERR_INVALID (tests/test_abi.py), never truncated. */
  double intrinsics[5];     /* exactly the model's count is read */
  double distortion[8];     /* already zero-padded / truncated like create_camera.cpp:24-27 */
  int32_t width, height;    /* image cols, rows */
  int32_t image_dtype;      /* NIDREG_IMAGE_* */
  int32_t flags;            /* NIDREG_FLAG_* */
  const void* image;        /* host pointer, rows x cols */
  int64_t image_row_stride; /* bytes between rows (cv::Mat::step) */
  int64_t num_points;       /* Frame::size() */
  const double* points;     /* host; Eigen::Vector4d (x y z 1) per point */
  int64_t point_stride;     /* bytes between points (32 for Frame::points) */
  const double* intensities;/* host; Frame::intensities */
  double max_fov;           /* NEAREST only: estimate_camera_fov() result [rad] */
  /* tuning (0 = default) */
  int32_t columns_per_group;/* histogram columns (bin_points values) a workgroup owns in LDS */
  int32_t target_blocks;    /* approximate number of point chunks = workgroups per pass */
  int32_t lds_copies;       /* lane-private copies of each histogram cell in LDS (1,2,4,8,16) */
  int32_t reserved1;
  int64_t scale_points;     /* points the fixed-point scale must hold (0 = num_points); shards of one
                               pair pass the TOTAL so that every rank uses the same 2^-frac unit */
  /* optional externally owned device resources (sharded multi-GPU use); NULL = internal */
  void* ext_stream;         /* hipStream_t the handle launches on */
  void* ext_hist;           /* device buffer of nidreg_hist_words(bins) 64-bit words */
  void* ext_out;            /* device buffer of NIDREG_OUT_DOUBLES doubles */
  /* one pair spread over several GPUs inside the library (single process): num_devices > 1 cuts the cloud along the
     pose-independent histogram column -- device_ids[k] owns a contiguous range of column groups, balanced by their point
     counts, and holds the points that fall into them -- so the GPUs' joint histograms have disjoint support: every GPU keeps
     a replica of the whole integer histogram and stores its own columns into every other GPU's replica, directly between the
     GPUs, once per evaluation (plain stores: no two GPUs write the same word).  Cost and histograms are bit-identical to the unsharded handle's, the gradient differs by
     summation order only.  The same device may be listed several times (a 1-GPU box exercising the protocol).
     0 = device_id alone, unless the environment variable NIDREG_DEVICES="0,1,..." is set -- which shards every handle
     (nidreg_create and nidreg_create_from_cloud), so a caller that knows nothing about GPUs (the reference's
     `new NIDCost(proj, image, points, bins)`) uses the whole node. */
  int32_t num_devices;
  int32_t device_ids[NIDREG_MAX_DEVICES];
} nidreg_desc;

#define NIDREG_OUT_DOUBLES 16  /* [0]=cost [1..7]=grad7 [8]=status [9]=inliers [10..15] reserved */

/* model string -> NIDREG_MODEL_* (or -1); optionally returns the parameter counts */
int nidreg_model_from_name(const char* name, int* num_intrinsics, int* num_distortion);

int nidreg_device_count(void);

int nidreg_create(const nidreg_desc* desc, nidreg_handle** out);
void nidreg_destroy(nidreg_handle* h);

/* Device-resident cloud (one upload per LiDAR-camera pair).  nidreg_create_from_cloud builds a handle from
 * it entirely on the GPU: optional ViewCulling::cull at T_camera_lidar (row-major 4x4; NULL = no culling;
 * min_z / enable_depth_buffer_culling as in nidreg_view_culling), then bucketing, Morton sort and record
 * gather -- the reference's per-outer-iteration `cull -> new NIDCost` (visual_camera_calibration.cpp:
 * 201-206) without a host round trip.  desc->points / intensities / num_points are ignored.  desc->num_devices /
 * NIDREG_DEVICES are honoured: the cull and the sort run on the cloud's GPU, every shard then takes the records of its
 * column groups device to device. */
typedef struct nidreg_cloud nidreg_cloud;
int nidreg_cloud_create(int device_id, const double* points, int64_t point_stride, const double* intensities, int64_t num_points, nidreg_cloud** out);
/* The same cloud from float32 records: x y z (three consecutive floats) every point_stride bytes, one float intensity every
 * intensity_stride bytes -- the stored PLY record (both pointers inside one 16 B or wider record, both strides = the record
 * size) or separate arrays (glk PLYData: vertices stride 12, intensities stride 4).  Only the float bytes are uploaded (the
 * one span covering both arrays when they interleave, else the two spans); the GPU widens them exactly into the layout
 * nidreg_cloud_create makes (x y z 1 doubles + double intensities), so every handle built from it has the same bits.
 * NIDREG_ERR_INVALID, before any device call: num_points outside [0, INT_MAX], a NULL pointer with num_points > 0, strides
 * below 12 / 4 bytes, strides or pointers not 4-byte aligned, a negative device_id (out of range: after the device count). */
int nidreg_cloud_create_f32(int device_id, const float* points, int64_t point_stride, const float* intensities, int64_t intensity_stride, int64_t num_points,
                            nidreg_cloud** out);
void nidreg_cloud_destroy(nidreg_cloud* cloud);
int nidreg_create_from_cloud(const nidreg_desc* desc, const nidreg_cloud* cloud, const double* T_camera_lidar, double min_z, int enable_depth_buffer_culling, nidreg_handle** out);
/* An EMPTY cloud (num_points = 0, or a selection that kept nothing) is a valid argument: the handle has no records, every
 * evaluation runs on zero histograms, the NID is not finite and nidreg_eval returns NIDREG_FALSE like the functor's `return false`
 * (nidreg_eval_iso hands the NaN back: CostCalculatorNID has no finite check). */
int nidreg_cloud_size(const nidreg_cloud* cloud, int64_t* n);
/* the cloud's points (n x 4 doubles: x y z 1) and intensities (n doubles) copied back to the host; either output may be NULL */
int nidreg_cloud_get(const nidreg_cloud* cloud, double* points_out, double* intensities_out);

/* Masks and range gates (no counterpart in the reference, whose users edit the PNG or the PLY by hand): leave image regions -- the
 * vehicle's bonnet, a burnt-in timestamp, a strip of sky -- and LiDAR ranges -- returns too close to carry a usable intensity --
 * out of the cost, on the device.
 *
 * nidreg_mask_create: mask = host, 8-bit, the camera image's size, row_stride bytes between rows; non-zero = use, zero = ignore
 * (nidreg_features_detect's convention).  What is kept is its EROSION by margin pixels: eroded(x, y) = the minimum of the mask
 * over [x - margin, x + margin] x [y - margin, y + margin] clipped to the image (pixels outside the image count as valid), so a
 * pixel is valid iff no ignored pixel lies within margin of it.  The B-spline of NIDCost reads columns x-1..x+2 and rows y-1..y+2
 * around a point's pixel: with margin >= 2 no ignored pixel is read at the pose the selection was made at.  nidreg_mask_get copies
 * the eroded mask out (host, width x height bytes, row_stride between rows).
 *
 * nidreg_cloud_select: the points of `cloud` that
 *   - survive ViewCulling::cull at T_camera_lidar (row-major 4x4), exactly as nidreg_view_culling / nidreg_create_from_cloud run it,
 *   - lie on a valid pixel of the eroded mask (mask NULL: every pixel is valid) -- the pixel is the one the cull truncated the
 *     projection to --, and
 *   - satisfy min_range^2 <= (x x + y y) + z z <= max_range^2 in the cloud's own (LiDAR) frame, in double without contraction
 *     (0 and +inf switch the gate off).  The gate runs AFTER the cull: a near point that is dropped still hides what is behind it.
 * They become a new cloud *out (nidreg_cloud_destroy) in input order, points and intensities copied byte for byte; their ascending
 * indices go to indices_out (nullable; capacity = the cloud's size) and their number to *count_out.  Zero selected points is not an
 * error: *out is an empty cloud.  With mask = NULL and the default range the indices are nidreg_view_culling's, and a handle
 * built from *out with T_camera_lidar = NULL has the records of the one nidreg_create_from_cloud builds from `cloud` with the cull
 * (set desc.scale_points to the size of `cloud` for the same fixed-point unit beyond 2^22 points).  Deterministic: a flag pass, an
 * exclusive scan of per-tile counts and a gather, NIDREG_SELECT_TILE points per workgroup, no atomics.
 * NIDREG_ERR_INVALID before any device call: a NULL mask / out / count_out / cloud / parameter array, width or height outside
 * [1, 16384], row_stride < width, margin outside [0, 64], a negative device_id, a mask whose size differs from width x height or
 * that lives on another device than the cloud, min_range < 0, max_range < min_range, a NaN in either, an unknown model. */
#define NIDREG_SELECT_TILE 1024
typedef struct nidreg_mask nidreg_mask;
int nidreg_mask_create(int device_id, const uint8_t* mask, int width, int height, int64_t row_stride, int margin, nidreg_mask** out);
int nidreg_mask_get(const nidreg_mask* mask, uint8_t* eroded_out, int64_t row_stride);
void nidreg_mask_destroy(nidreg_mask* mask);
int nidreg_cloud_select(const nidreg_cloud* cloud, int model_id, const double* intrinsics, const double* distortion, int width, int height, const double* T_camera_lidar, double min_z,
                        int enable_depth_buffer_culling, const nidreg_mask* mask, double min_range, double max_range, nidreg_cloud** out, int32_t* indices_out, int64_t* count_out);
/* what became of the source's points, for a cloud nidreg_cloud_select made: counts3 = {kept by the cull, of those removed by the mask,
 * of the rest removed by the range gate}; the cloud's size is [0] - [1] - [2].  NIDREG_ERR_INVALID for any other cloud. */
int nidreg_cloud_select_counts(const nidreg_cloud* selected, int64_t* counts3);

/* Folds of a cloud (no counterpart in the reference): a fold of a device-resident cloud, or its complement, as a new cloud on the
 * same device, without a host round trip -- what recalibrating on subsets of the data (jackknife, held-out subsets) needs.
 *
 * The fold of point i is a function of (seed, cell, num_folds) and of the point alone, in integer arithmetic modulo 2^64 apart from
 * the one division below:
 *   mix64(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *   key        cell == 0 (per-point folds): i.
 *              cell > 0 (spatial blocks: the points of one cell-metre cube share a fold): c_a = floor(p_a / cell) per axis in double
 *              (a true division, then floor); if x, y, z are finite and every c_a lies in [-2^20, 2^20):
 *              (c_x + 2^20) | (c_y + 2^20) << 21 | (c_z + 2^20) << 42 (the integrator's packing); otherwise 2^63 | i (the point is
 *              folded on its own)
 *   fold       h = mix64(seed + 0x9E3779B97F4A7C15 * (key + 1));  fold = ((h >> 32) * num_folds) >> 32
 * (seed = 0, key = 0, 1, 2: h = 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F.)
 *
 * nidreg_cloud_fold_ids: the fold of every point to folds_out (n words; may be NULL only for an empty cloud) and the folds' sizes to
 * sizes_out (num_folds words, nullable).
 * nidreg_cloud_fold: the points whose fold equals `fold` (complement == 0) or differs from it (complement != 0) become a new cloud
 * *out (nidreg_cloud_destroy) in input order, points and intensities copied byte for byte; their ascending indices go to indices_out
 * (nullable; capacity = the cloud's size) and their number to *count_out.  An empty result is a valid empty cloud.  The source is
 * not modified.  nidreg_cloud_select_counts refuses *out: it is not a selection.
 * Deterministic, no atomics: a flag pass with wave64 ballots, then nidreg_cloud_select's exclusive scan and gather; the sizes come
 * from per-workgroup ballots and sums, reduced in a fixed order.
 * NIDREG_ERR_INVALID before any device call: a NULL cloud / out / count_out / folds_out (with points), num_folds outside
 * [1, NIDREG_FOLD_MAX], fold outside [0, num_folds), a negative, NaN or infinite cell. */
#define NIDREG_FOLD_MAX 1024
int nidreg_cloud_fold_ids(const nidreg_cloud* cloud, uint64_t seed, double cell, int num_folds, int32_t* folds_out, int64_t* sizes_out);
int nidreg_cloud_fold(const nidreg_cloud* cloud, uint64_t seed, double cell, int num_folds, int fold, int complement, nidreg_cloud** out, int32_t* indices_out, int64_t* count_out);

/* NIDCost::operator(): cost (+ gradient when grad7 != NULL) at se3 = [qx qy qz qw tx ty tz] */
int nidreg_eval(nidreg_handle* h, const double* se3, double* cost, double* grad7);

/* n synchronous nidreg_eval calls back to back, as an optimiser's inner loop issues them (each evaluation completes --
 * host sync included -- before the next starts): se3s n x 7, costs n (nullable), grads7 n x 7 (NULL = cost only).
 * Returns < 0 on the first error, else NIDREG_FALSE if any evaluation was rejected, else NIDREG_OK. */
int nidreg_eval_batch(nidreg_handle* h, const double* se3s, int n, double* costs, double* grads7);

/* CostCalculatorNID::calculate at a row-major 4x4 T_camera_lidar */
int nidreg_eval_iso(nidreg_handle* h, const double* T_camera_lidar, double* cost);

/* Asynchronous evaluation, for callers that hold several INDEPENDENT poses -- Nelder-Mead's initial simplex
 * (include/dfo/nelder_mead.hpp:32-57 evaluates its n + 1 vertices before the first step), multi-start, finite-difference
 * checks; a line search (BFGS, visual_camera_calibration.cpp:210-229) has nothing to overlap and keeps nidreg_eval.
 * nidreg_submit queues the kernels of NIDCost::operator() (want_grad != 0: with the Jacobian) and returns at once with a
 * ticket; nidreg_submit_iso does the same for CostCalculatorNID::calculate.  nidreg_wait blocks until that evaluation is
 * complete and returns what nidreg_eval / nidreg_eval_iso would have (cost, grad7 when it was asked for; NIDREG_FALSE for a
 * non-finite NID).  The evaluations of one handle run back to back in submission order -- no host round trip between
 * them --, each into its own host-mapped result block; tickets may be collected in any order.  At most 8 evaluations of a
 * handle may be in flight (NIDREG_ERR_INVALID beyond that: collect first); a handle must not be destroyed, and its
 * histograms not read, while tickets are outstanding.  Handles spread over several GPUs, handles with caller-provided
 * result buffers and handles with timing enabled evaluate inside nidreg_submit (the ticket then only carries the results).
 * Results are bit-identical to the synchronous calls. */
int nidreg_submit(nidreg_handle* h, const double* se3, int want_grad, int64_t* ticket);
int nidreg_submit_iso(nidreg_handle* h, const double* T_camera_lidar, int64_t* ticket);
int nidreg_wait(nidreg_handle* h, int64_t ticket, double* cost, double* grad7);

/* nidreg_eval_batch's arguments and results for n INDEPENDENT poses, through the submit / wait pair: up to 7 evaluations
 * queued ahead of the one being collected (the handle must have no outstanding tickets). */
int nidreg_eval_pipelined(nidreg_handle* h, const double* se3s, int n, double* costs, double* grads7);

/* MultiNIDCost::operator(): trust gate against init_se3 (NULL = no gate), all pairs in flight at once, plain sum
 * of costs / gradients, NIDREG_FALSE if the gate rejects or any pair is non-finite.  Handles on different GPUs run
 * concurrently (every GPU's histogram pass is queued before the rest).  2..16 compatible SPLINE handles on ONE GPU
 * (same camera, image size, bins, precision) are evaluated by ONE grid per pass over the chunks of all pairs -- three
 * launches in all instead of three per pair; each pair keeps its own histogram, fixed-point unit and result block, so
 * every pair's cost and histogram are bit-identical to evaluating the handles one by one; the gradient's workgroup
 * partials follow the group's chunk table, i.e. it is equal up to summation order (NIDREG_NO_MULTI_GRID=1 in the
 * environment forces the per-pair launches). */
int nidreg_eval_multi(nidreg_handle* const* handles, int n, const double* init_se3, const double* se3, double* cost, double* grad7);

/* sum_i CostCalculatorNID_i::calculate(T); compatible NEAREST handles on one GPU share one grid per pass like nidreg_eval_multi */
int nidreg_eval_iso_multi(nidreg_handle* const* handles, int n, const double* T_camera_lidar, double* cost);

/* raw histograms of the most recent evaluation (any pointer may be NULL).
 * joint: bins*bins doubles [bin_image][bin_points]; hist_image, hist_points: bins doubles. */
int nidreg_get_hist(nidreg_handle* h, double* joint, double* hist_image, double* hist_points);
/* the same joint histogram as exact integers: fixed-point words (value * 2^frac_bits) in SPLINE
 * mode, counts (frac_bits = 0) in NEAREST mode. */
int nidreg_get_hist_fixed(nidreg_handle* h, int64_t* joint, int64_t* inliers, int* frac_bits);

/* GenericCameraBase::project for n points (host in, host out), evaluated on the device with the
 * same projection code the cost kernels use.  p3: n x 3 doubles, uv: n x 2 doubles,
 * jac (nullable): n x 6 doubles = d(u,v)/d(x,y,z) row-major 2x3. */
int nidreg_project(nidreg_handle* h, const double* p3, int64_t n, double* uv, double* jac);
/* the same without a handle (used for one-time host set-up such as estimate_camera_fov,
 * src/vlcal/common/estimate_fov.cpp:17-51); intrinsics[5] / distortion[8] as in nidreg_desc.
 * device_id = NIDREG_DEVICE_HOST: the device's scalar projection code compiled for the host (fp64; equal to the device's
 * result up to the reciprocal seeds, ~1e-14 relative) -- for callers that probe ONE point at a time, like the ~240 probes of
 * estimate_camera_fov's NelderMead<2>, which is host work in the reference too. */
#define NIDREG_DEVICE_HOST (-1)
/* vlcal::estimate_camera_fov (src/vlcal/common/estimate_fov.cpp:36-51; estimate_direction :17-34 with NelderMead<2>,
 * include/dfo/nelder_mead.hpp): the largest view angle over the pixels (0,0), (W/2,0), (0,H/2) [rad] -- what
 * CostCalculatorNID's max_fov, ViewCulling's min_z and generate_lidar_image take.  Host only (no GPU involved). */
int nidreg_estimate_camera_fov(int model_id, const double* intrinsics, const double* distortion, int width, int height, double* max_fov);
int nidreg_project_model(int model_id, const double* intrinsics, const double* distortion, int device_id, int precision, const double* p3, int64_t n, double* uv, double* jac);

/* ---- initial guess: PoseEstimation::estimate_rotation_ransac (src/vlcal/common/estimate_pose.cpp:40-145) ----------------------
 * nidreg_estimate_directions: vlcal::estimate_direction (estimate_fov.cpp:17-34, NelderMead<2> over the projection) for n pixels,
 * uv n x 2 -> dirs3 n x 3 (the loop of estimate_pose.cpp:48-51).  Host only, the same code nidreg_estimate_camera_fov runs for its
 * three pixels; the pixels are spread over at most 16 host threads. */
int nidreg_estimate_directions(int model_id, const double* intrinsics, const double* distortion, const double* uv, int64_t n, double* dirs3);
/* The hypotheses nidreg_estimate_rotation_ransac draws when it is given none: pairs[2k], pairs[2k+1] = two DISTINCT indices in
 * [0, n), a pure function of (seed, k, n) (splitmix64 rounds of a counter; no state, so independent of grid shape and thread
 * count).  DEVIATION: the reference samples with replacement from mt19937 streams seeded per OpenMP thread
 * (estimate_pose.cpp:90-108) -- not reproducible across machines, and a pair that names one correspondence twice is a rank-1
 * problem whose rotation is arbitrary.  Host only.  n >= 2. */
int nidreg_ransac_sample_pairs(uint64_t seed, int64_t n, int iterations, int32_t* pairs);
/* estimate_pose.cpp:53-145 on the device: `iterations` hypotheses, each the least-squares rotation between two pairs of UNIT
 * bearings (find_rotation, :55-83: U diag(1, 1, det U det V) V^T of the SVD of A B^T, here in closed form, fp64), scored by the
 * number of correspondences with |kp - project(R d_lidar)|^2 < error_thresh^2 (:114-123; strict <, a non-finite projection is an
 * outlier).  kpts2: n x 2 pixels, dirs_camera3 / dirs_lidar3: n x 3 unit bearings (nidreg_estimate_directions; the normalised
 * LiDAR points).  sample_pairs: iterations x 2 indices dictating the hypotheses, or NULL = nidreg_ransac_sample_pairs(seed, ...).
 * A hypothesis whose two bearings coincide (or the same index twice) has no rotation and counts 0 inliers.
 * The winner is the largest count, ties to the LOWEST iteration (the reference keeps whichever thread entered its critical
 * section first, :125-130).  R9: its R_camera_lidar, row-major; inlier_flags (n, nullable): :135-142; counts (iterations,
 * nullable): every hypothesis' count.  best_inliers = counts[best_iteration] = the number of set flags.
 * NIDREG_ERR_INVALID before any device call: iterations <= 0, n < 2, a NULL input, an unknown model, an index out of range. */
int nidreg_estimate_rotation_ransac(int model_id, const double* intrinsics, const double* distortion, int device_id, const double* kpts2, const double* dirs_camera3,
                                    const double* dirs_lidar3, int64_t n, int iterations, double error_thresh, uint64_t seed, const int32_t* sample_pairs, double* R9,
                                    int32_t* best_iteration, int32_t* best_inliers, uint8_t* inlier_flags, int32_t* counts);

/* ViewCulling::cull (src/vlcal/calib/view_culling.cpp:21-92) on the device: FoV gate against
 * min_z = cos(estimate_camera_fov), in-image test, per-pixel depth buffer (float distance) and the
 * +0.1 m keep threshold.  points: host, (x y z 1) doubles with the given byte stride; T: row-major 4x4
 * T_camera_lidar.  Writes the surviving indices (ascending; identical to the in-repo oracle's and to the reference's
 * source compiled against the stand-in Eigen of oracle/shim -- a build against real Eigen, whose fixed-size reductions
 * and 4x4 products may associate differently, can differ by 1 ulp in a borderline FoV / pixel / depth decision) into
 * indices_out (capacity num_points) and returns their number, or a negative error code. */
int64_t nidreg_view_culling(int model_id, const double* intrinsics, const double* distortion, int device_id, int width, int height, double min_z, int enable_depth_buffer_culling,
                            const double* points, int64_t point_stride, int64_t num_points, const double* T_camera_lidar, int32_t* indices_out);

/* PointsColorUpdater (src/vlcal/common/points_color_updater.cpp): the per-frame recolouring of the
 * whole cloud the viewer runs every 50 ms while the optimiser works (visual_lidar_visualizer.cpp:89-100).
 * create = the constructor (:26-35): uploads the 8-bit image, the points ((x y z 1) doubles, byte
 * stride >= 32) and the per-point intensity colours (n x RGBA float; the reference fills them with
 * glk::colormapf(TURBO, intensity), a table that lives in Iridescence, so the caller passes them;
 * NULL = (1,1,1,1) like the icosahedron constructor, :24).  min_nz = cos(estimate_camera_fov + 0.5 deg) (:12).
 * update = PointsColorUpdater::update (:37-61): colours[i] = (pix/255, pix/255, pix/255, 1) * float(w)
 * + intensity_colors[i] * float(1 - w) in float arithmetic, or (0,0,0,0) when the point is outside the
 * FoV / image.  colors_out: host n x 4 floats, or NULL to leave the result on the device
 * (nidreg_colorizer_device_colors; valid until the next update / destroy). */
typedef struct nidreg_colorizer nidreg_colorizer;
int nidreg_colorizer_create(int device_id, int model_id, const double* intrinsics, const double* distortion, int width, int height, const uint8_t* image, int64_t image_row_stride,
                            int64_t num_points, const double* points, int64_t point_stride, const float* intensity_colors, double min_nz, nidreg_colorizer** out);
int nidreg_colorizer_update(nidreg_colorizer* c, const double* T_camera_lidar, double blend_weight, float* colors_out);
const float* nidreg_colorizer_device_colors(nidreg_colorizer* c);
void nidreg_colorizer_destroy(nidreg_colorizer* c);

/* generate_lidar_image (src/vlcal/preprocess/generate_lidar_image.cpp:7-41): z-buffered rendering of
 * the cloud through the camera model.  min_nz = cos(estimate_camera_fov) (:10-11).  Per pixel the point
 * with the smallest squared camera-frame distance wins; on exact ties the largest index (the sequential
 * reference overwrites on `!(stored < sq_dist)`, :31).  intensity_image: height x width doubles (0 where
 * nothing landed), index_image: height x width int32 (-1 where nothing landed); either may be NULL.
 * Output is independent of the thread order and identical to the in-repo oracle's sequential loop (same 1-ulp caveat
 * about real Eigen's association order as nidreg_view_culling). */
int nidreg_generate_lidar_image(int model_id, const double* intrinsics, const double* distortion, int device_id, int width, int height, double min_nz, const double* points,
                                int64_t point_stride, const double* intensities, int64_t num_points, const double* T_camera_lidar, double* intensity_image, int32_t* index_image);

/* Intensity rank equalisation of an integrated cloud (src/vlcal/preprocess/preprocess.cpp:464-473,
 * src/preprocess_map.cpp): in place, intensities[rank order i] = floor(256 * i / n) / 256, the values the
 * NID path then bins.  Device radix sort; stable, i.e. equal intensities keep their index order (the
 * reference's std::sort leaves that order unspecified). */
int nidreg_equalize_intensities(int device_id, double* intensities, int64_t num_points);

/* ---- headless viewer: a z-buffered point-splat renderer (csrc/nid_splat_kernels.hpp) ------------------------------------------
 * The reference shows a result in an OpenGL window (src/viewer.cpp; VisualLiDARVisualizer; the colours come from
 * PointsColorUpdater::update, src/vlcal/common/points_color_updater.cpp:37-61).  This is the part of it that makes a picture, without
 * a window: every point is a (2 radius + 1)^2 square of pixels around the pixel it projects to, depth-tested.
 *   nidreg_splat_create      uploads the cloud once ((x y z w) doubles, byte stride >= 32): one upload serves every view of a bag.
 *                            num_points = 0 is valid.
 *   nidreg_splat_set_colors  num_points x RGBA8 (host); may be called again between draws.
 *   nidreg_splat_draw        point i goes through the front end of PointsColorUpdater::update / generate_lidar_image under
 *                            T_view_lidar (row-major 4x4) and the given camera: FoV gate (normalised z >= min_nz), projection,
 *                            truncating cast, in-image test.  A point that fails it draws NOTHING, even where its square would reach
 *                            into the image.  Its depth is d = float(squared camera-frame distance), rounded to nearest (non-finite:
 *                            nothing drawn); per covered pixel inside the image the smallest
 *                                (bits(d) << 32) | (0xFFFFFFFF - i)
 *                            wins: the nearest point in float32 and, among equal float32 depths, the LARGEST index (the tie direction
 *                            of nidreg_generate_lidar_image; depths that differ only in fp64 are equal here).  Then per pixel, in
 *                            integers: a = (alpha * A_i + 127) / 255, channel = (background * (255 - a) + C_i * a + 127) / 255;
 *                            a pixel nothing covers keeps the background.  background_rgb: height rows of 3 * width bytes,
 *                            background_row_stride bytes apart (0: packed), or NULL = black.  out_rgb: height x width x 3 bytes;
 *                            out_index (nullable): height x width int32, the winning point or -1.  Every draw starts from an empty
 *                            depth buffer.  The picture is the same bytes from run to run and equals tests/viewer_oracle.py.
 * NIDREG_ERR_INVALID with a message, before the device is touched and with nothing written: num_points above 2^31 - 1 or negative,
 * a point stride that is no multiple of 8 or below 32, radius outside [0, 8], alpha outside [0, 255], a non-positive width or height
 * or width * height beyond int, a background row stride below 3 * width, an unknown model, a NULL array, a draw of a non-empty cloud
 * before any colours were set. */
typedef struct nidreg_splat nidreg_splat;
int nidreg_splat_create(int device_id, int64_t num_points, const double* points, int64_t point_stride, nidreg_splat** out);
int nidreg_splat_set_colors(nidreg_splat* s, const uint8_t* rgba);
int nidreg_splat_draw(nidreg_splat* s, int model_id, const double* intrinsics, const double* distortion, int width, int height, double min_nz, const double* T_view_lidar, int radius,
                      const uint8_t* background_rgb /* nullable */, int64_t background_row_stride, int alpha, uint8_t* out_rgb, int32_t* out_index /* nullable */);
void nidreg_splat_destroy(nidreg_splat* s);

/* ---- voxel integrator: vlcal::StaticPointCloudIntegrator (src/vlcal/preprocess/static_point_cloud_integrator.cpp) -------------
 * A hash table of voxels on the device (csrc/nid_voxel_kernels.hpp).  The reference's loop (:25-37), per point in order: skip it when
 * sqrt(x^2 + y^2 + z^2) < min_distance; voxel = floor(x / res), floor(y / res), floor(z / res) in double (a true division and a
 * floor: -0.1 at res 0.25 is voxel -1); voxelgrid[voxel] = (x, y, z, intensity), OVERWRITING.  So the integrator ends with one
 * entry per occupied voxel, the LAST point inserted into it over all insert calls.  Here: every point has a sequence number = the
 * number of points offered by the accepted insert calls before it (int64; skipped points count), and a voxel's entry is the point
 * with the largest sequence number -- the same entry, whatever order the GPU visits the points in.  Results are bit-reproducible.
 *   nidreg_integrator_create   the constructor (:16): voxel_resolution > 0 and finite, min_distance not NaN, else
 *                              NIDREG_ERR_INVALID.  (The reference's defaults, :8-12: 0.05 and 1.0.)  The table's capacity is not
 *                              an argument: it grows by rehashing on the device.
 *   nidreg_integrator_insert   insert_points (:25-37).  points: x y z as three consecutive doubles every point_stride bytes (0 = 32,
 *                              Frame::points; >= 24, a multiple of 8), intensities: n doubles.  n == 0 is a valid insert.
 *   nidreg_integrator_insert_f32  the same from float32: x y z every point_stride bytes, one float intensity every
 *                              intensity_stride bytes (the stored 16-byte PLY record is uploaded as it lies, like
 *                              nidreg_cloud_create_f32); widened exactly on the GPU, so the result has the same bits as
 *                              nidreg_integrator_insert fed the widened values.
 *   nidreg_integrator_insert_cloud2  the data bytes of a sensor_msgs/PointCloud2 message as they lie in the message: num_points
 *                              records of point_step bytes (1..65535), uploaded once and decoded on the GPU.  Replaces, per frame,
 *                              extract_raw_points (include/vlcal/common/ros_cloud_converter.hpp:62-175), the finite filter of
 *                              src/vlcal/preprocess/preprocess.cpp:457 and insert_points (:25-36).  x, y, z at x/y/z_offset, all of
 *                              xyz_datatype FLOAT32 (7) or FLOAT64 (8); the intensity channel at intensity_offset, of
 *                              intensity_datatype UINT8 (2), UINT16 (4), UINT32 (6), FLOAT32 (7) or FLOAT64 (8); all converted to
 *                              double exactly.  Offsets are arbitrary byte offsets (no alignment is assumed), little-endian.  A point
 *                              with a non-finite x, y or z is SKIPPED, not refused (the intensity is not tested): it is counted in
 *                              *num_skipped (nullable) and still takes a sequence number -- point i of the frame has number
 *                              offered + i and `offered` advances by num_points --, so entries and order equal those of
 *                              nidreg_integrator_insert fed the decoded, filtered points; only the sequence numbers differ.  A finite
 *                              point outside the packed-key limit still refuses the whole frame.  NIDREG_ERR_INVALID before any
 *                              device call: a field outside the record, point_step out of range, another datatype, NULL data with
 *                              num_points > 0, num_points < 0.  num_points == 0 is a valid insert.  Device memory: the raw frame and
 *                              40 bytes per point of it.
 *   nidreg_integrator_insert_las  the point records of an ASPRS LAS 1.0 - 1.4 file as they lie in the file (dataset.read_las_header says
 *                              where): num_points records of record_length bytes of point_format 0..10 (base lengths 20, 28, 26, 34,
 *                              57, 63, 30, 36, 38, 59, 67; a longer record carries extra bytes), uploaded once and decoded on the GPU
 *                              (csrc/nid_las_kernels.hpp).  Coordinate = (double(int32) * scale + offset) - origin, three separately
 *                              rounded fp64 operations: the file's own definition, then the recentring of a georeferenced map before
 *                              anything is narrowed to float32.  intensity_source 0: the 16-bit intensity; 1: 77 R + 150 G + 29 B of
 *                              the 16-bit colour channels (formats 2, 3, 5, 7, 8, 10 only).  exclude_classes4 (nullable): 256 bits,
 *                              bit c set = points of class c are dropped (the class is 5 bits in formats 0 - 5, 8 bits in 6 - 10);
 *                              withheld points are dropped unless keep_withheld.  A dropped point is SKIPPED the way a non-finite
 *                              PointCloud2 point is: counted in *num_skipped (nullable), and it still takes its sequence number.
 *                              A kept point outside the packed-key limit refuses the whole chunk.  NIDREG_ERR_INVALID before any
 *                              device call, the arguments before the handle: a format outside 0..10, a record_length below the
 *                              format's base or above 65535, a NULL scale3 / offset3 / origin3, a scale that is zero or non-finite, a
 *                              non-finite offset or origin, another intensity_source, rgb asked of a format without it, NULL records
 *                              with num_points > 0, num_points < 0, a NULL integrator.  UNPINNED against laspy / PDAL and real files.
 *   nidreg_integrator_las_timing  host wall-clock milliseconds of the calling thread's last nidreg_integrator_insert_las: [0] checks,
 *                              allocation and upload, [1] the decode kernel, launch to idle, [2] the integrator's passes.
 *   nidreg_lzf_decompress      host only (csrc/nid_lzf_host.hpp): the LZF stream of a PCD file's `DATA binary_compressed` body into
 *                              out_size bytes; *written (nullable) = bytes produced.  Input that ends inside a token, a reference to
 *                              before the output and an output overrun are NIDREG_ERR_INVALID, the input offset in
 *                              nidreg_last_error().  UNPINNED against liblzf / PCL and real files.
 *   nidreg_integrator_size     voxelgrid.size()
 *   nidreg_integrator_get      get_points (:49-62): num_voxels records of 16 bytes, float x y z intensity = `cast<float>()` of the
 *                              entry (the PLY record: feeds nidreg_cloud_create_f32 and a PLY writer without a repack); seq
 *                              (nullable): the winners' sequence numbers.  ORDER: ascending sequence number (the reference's is
 *                              std::unordered_map iteration order, i.e. unspecified): deterministic, identical from run to run.
 *   nidreg_integrator_info     [0] voxels, [1] slots of the table, [2] points offered so far, [3] bytes per slot
 * THE ONE NARROWING against the reference: a voxel is identified by its full integer coordinate (never by a hash of it), packed
 * into 64 bits at 21 bits per axis, so the voxel index must lie in [-2^20, 2^20) = [-1048576, 1048576) on every axis (+-2.1 km at
 * the reference's 2 mm map resolution; the reference's key is three ints).  A frame that holds a point beyond that, or a point with
 * a non-finite coordinate (where the reference converts NaN / an overflowing double to int: undefined behaviour), is refused as a
 * whole with NIDREG_ERR_INVALID BEFORE anything is inserted -- a check pass over the frame runs first --; the integrator is
 * unchanged, the refused frame's points do not count as offered, and nidreg_last_error() names the limit.
 * Device memory: the table (32 bytes per slot, at most half full, the winner's record inside its slot), one frame's upload and
 * 4 bytes per point of a 1M-point chunk; earlier frames are not kept.  Not thread-safe per integrator. */
typedef struct nidreg_integrator nidreg_integrator;
int nidreg_integrator_create(int device_id, double voxel_resolution, double min_distance, nidreg_integrator** out);
int nidreg_integrator_insert(nidreg_integrator* h, const double* points, int64_t point_stride, const double* intensities, int64_t n);
int nidreg_integrator_insert_f32(nidreg_integrator* h, const float* points, int64_t point_stride, const float* intensities, int64_t intensity_stride, int64_t n);
int nidreg_integrator_insert_cloud2(nidreg_integrator* h, const void* data, int64_t num_points, int32_t point_step, int32_t x_offset, int32_t y_offset, int32_t z_offset, int32_t xyz_datatype,
                                    int32_t intensity_offset, int32_t intensity_datatype, int64_t* num_skipped);
int nidreg_integrator_insert_las(nidreg_integrator* h, const void* records, int64_t num_points, int32_t record_length, int32_t point_format, const double* scale3, const double* offset3,
                                 const double* origin3, int32_t intensity_source /* 0 = intensity, 1 = rgb */, const uint64_t* exclude_classes4 /* nullable: 256 bits, bit c = drop class c */,
                                 int32_t keep_withheld, int64_t* num_skipped);
int nidreg_integrator_las_timing(double* ms3);
int nidreg_lzf_decompress(const uint8_t* in, int64_t in_size, uint8_t* out, int64_t out_size, int64_t* written);
int nidreg_integrator_size(nidreg_integrator* h, int64_t* num_voxels);
int nidreg_integrator_get(nidreg_integrator* h, float* records16 /* num_voxels x {x, y, z, intensity} */, int64_t* seq /* optional, may be NULL */);
int nidreg_integrator_info(nidreg_integrator* h, int64_t* info4);
void nidreg_integrator_destroy(nidreg_integrator* h);

/* ---- scan-to-model odometry: vlcal::DynamicPointCloudIntegrator (src/vlcal/preprocess/dynamic_point_cloud_integrator.cpp) ------------
 * The device side of `preprocess -d` (csrc/nid_odom_kernels.hpp); the Levenberg-Marquardt loop over the 12 unknowns runs on the host
 * (odometry.py).  All arrays are host memory, all arithmetic fp64, no floating-point atomics: every output has the same bits from run
 * to run.  Points are x y z (3 doubles), covariances xx xy xz yy yz zz (6 doubles).
 *   nidreg_odom_create        the model: iVox(voxel_resolution, insertion_dist_thresh) (src/vlcal/common/ivox.cpp; the reference uses
 *                             1.0 and 0.05) -- a hash of voxels under the integrator's packed 64-bit key, each voxel an ordered list of
 *                             points in chained blocks of 64 from a pool that grows up to max_blocks (1..2^24; 4.6 KB a block).  The
 *                             LRU eviction is off until nidreg_odom_set_lru turns it on: the model then only grows.
 *   nidreg_odom_set_lru       iVox's lru_thresh and lru_cycle (the reference: 100 and 10; ivox.cpp:144-178, :223).  Every
 *                             nidreg_odom_model_insert that reaches the device raises lru_count by one and stamps the voxels it offers
 *                             a point to (a refused point included); nidreg_odom_linearize stamps every face-neighbour voxel its search
 *                             finds.  After an insert with lru_count - lru_thresh > 0 and lru_count % lru_cycle == 0, every voxel whose
 *                             stamp is < lru_count - lru_thresh leaves the model and its blocks are handed out again before the pool
 *                             grows.  lru_thresh = 0 (the state after create): off, nothing is stamped by a search.  NIDREG_ERR_INVALID
 *                             for lru_thresh < 0, lru_cycle < 1, or after the first insert (a model must not carry stamps that were
 *                             never written).  NOT built: the reference's "too many voxels" branch (:181-197; 2^32 - 1 voxels).  A call
 *                             with m = 0 does not reach the device and does not count (the reference counts it).
 *   nidreg_odom_lru_info      [0] lru_count, [1] voxels evicted in total, [2] free blocks now, [3] eviction passes run
 *   nidreg_odom_knn_covariances  for m points the k nearest of each among them (itself included; 2 <= k <= 32 and k <= m, else
 *                             NIDREG_ERR_INVALID), ordered by ascending (squared distance, index), into neighbors (m x k, nullable);
 *                             then CloudCovarianceEstimation::estimate(points, neighbors) (cloud_covariance_estimation.cpp:77-112): the
 *                             neighbour set's covariance (/ (k - 1)), PLANE-regularised: covs = I - 0.999 n n^T with n (normals, m x 3,
 *                             nullable) the unit eigenvector of its smallest eigenvalue by a closed-form 3x3 solver (sign unspecified).
 *   nidreg_odom_covariances   the same from a GIVEN neighbour list (the reference reuses the lists on the deskewed points)
 *   nidreg_odom_model_insert  iVox::insert: points in ascending index; a point enters its voxel iff its squared distance to every point
 *                             already there is > insertion_dist_thresh^2.  A non-finite point or a voxel index outside [-2^20, 2^20)
 *                             refuses the call (NIDREG_ERR_INVALID, nothing inserted); an exhausted pool is NIDREG_ERR_FULL (points of
 *                             this call are then missing from the model: never silently).  A voxel enters the table only with its
 *                             first block (the table has >= 2 x max_blocks slots, so it stays at most half full), so a dry pool
 *                             leaves nothing behind and every later call that still needs a block reports NIDREG_ERR_FULL again.
 *   nidreg_odom_model_info    [0] voxels, [1] points, [2] blocks in use (handed out and not free), [3] max_blocks
 *   nidreg_odom_model_get     every point of the model: voxels in ascending key order, a voxel's points in list order
 *   nidreg_odom_set_source    the scan's sampled points, their covariances and time-table indices (>= 0), uploaded once per scan
 *   nidreg_odom_linearize     IntegratedCT_GICPFactor_::linearize (include/vlcal/common/integrated_ct_gicp_factor_impl.hpp:70-177).  poses:
 *                             per time-table entry 84 doubles -- the pose (R row-major 9, t 3) and its 6 x 6 derivatives by pose 0 and by
 *                             pose 1 (row-major, gtsam's [omega, v] order).  Per source point: the nearest model point over the 7
 *                             face-neighbour voxels of the transformed point (a tie goes to the later one, as in the reference), rejected
 *                             when none or further than max_correspondence_dist_sq; (C_B + R C_A R^T)^-1; the terms of out122 = H_00 (36,
 *                             row-major) H_01 (36) H_11 (36) b_0 (6) b_1 (6) error count.  (gtsam's HessianFactor takes -b.)  Per-wave
 *                             partials summed in wave order.  Correspondences and Mahalanobis matrices are kept.
 *   nidreg_odom_error         ::error (:40-67) at other poses (12 doubles per entry) on the kept correspondences: out2 = error, count
 *   nidreg_odom_correspondences  per source point: found (0 / 1), the matched model point (3), the Mahalanobis matrix (9); nullable
 *   nidreg_odom_deskew_insert voxelgrid_task (:123-155) for one raw PointCloud2 frame into a voxel integrator: the arguments of
 *                             nidreg_integrator_insert_cloud2, the time field (time_datatype UINT32 (6), FLOAT32 (7) or FLOAT64 (8): time =
 *                             value * time_scale + time_shift [s]; 0 = no field: time = time_scale * index / num_points), max_time (<= 0:
 *                             every point at t = 0), and the motion: begin12 = T_begin (R row-major, t), rotvec3 = Logmap(R_begin^T
 *                             R_end), dtrans3 = t_end - t_begin.  Per point t = time / max_time, the pose interpolateRt(T_begin, T_end, t),
 *                             the transformed point; then the integrator's own passes: non-finite points skipped and counted,
 *                             |p| < min_distance in the odometry frame skipped, sequence number = offered + index in the message.
 *                             Two differences from the reference: it refreshes the pose only every 1e-4 of normalised time along the
 *                             time-sorted order, and within a frame its latest-in-time point of a voxel wins (here: the highest index). */
typedef struct nidreg_odom nidreg_odom;
int nidreg_odom_create(int device_id, double voxel_resolution, double insertion_dist_thresh, int32_t max_blocks, nidreg_odom** out);
void nidreg_odom_destroy(nidreg_odom* h);
int nidreg_odom_knn_covariances(nidreg_odom* h, const double* points, int32_t m, int32_t k, int32_t* neighbors, double* normals, double* covs);
int nidreg_odom_covariances(nidreg_odom* h, const double* points, int32_t m, int32_t k, const int32_t* neighbors, double* normals, double* covs);
int nidreg_odom_model_insert(nidreg_odom* h, const double* points, const double* covs, int32_t m);
int nidreg_odom_model_info(nidreg_odom* h, int64_t* info4);
int nidreg_odom_set_lru(nidreg_odom* h, int32_t lru_thresh, int32_t lru_cycle);
int nidreg_odom_lru_info(nidreg_odom* h, int64_t* info4);
int nidreg_odom_model_get(nidreg_odom* h, int32_t* voxels /* points x 3 */, double* points /* points x 3 */, double* covs /* points x 6, nullable */);
int nidreg_odom_set_source(nidreg_odom* h, const double* points, const double* covs, const int32_t* time_index, int32_t m);
int nidreg_odom_linearize(nidreg_odom* h, const double* poses /* num_poses x 84 */, int32_t num_poses, double max_correspondence_dist_sq, double* out122);
int nidreg_odom_error(nidreg_odom* h, const double* poses12 /* num_poses x 12 */, int32_t num_poses, double* out2);
int nidreg_odom_correspondences(nidreg_odom* h, int32_t* found, double* target, double* mahalanobis);
int nidreg_odom_deskew_insert(nidreg_integrator* integrator, const void* data, int64_t num_points, int32_t point_step, int32_t x_offset, int32_t y_offset, int32_t z_offset, int32_t xyz_datatype,
                              int32_t intensity_offset, int32_t intensity_datatype, int32_t time_offset, int32_t time_datatype, double time_scale, double time_shift, double max_time,
                              const double* begin12, const double* rotvec3, const double* dtrans3, int64_t* num_skipped);

/* ---- find_matches: keypoints and 2D-2D matches between the camera image and the LiDAR intensity image -------------------------------
 * What initial_guess_auto reads (<bag>_matches.json) the reference produces with scripts/find_matches_superglue.py (SuperGlue: learned
 * weights under a non-commercial licence, OpenCV).  This is a classical, licence-free STAND-IN, not a port: FAST-9 corners over an
 * image pyramid, upright BRIEF-256 descriptors, mutual-best Hamming matching with a ratio test (csrc/nid_match_kernels.hpp).  Of the
 * reference script only the command line and the JSON keys are kept (find_matches.py).  Its quality on real camera / LiDAR pairs is
 * UNMEASURED.  All arithmetic is integer on 8-bit pixels and no kernel uses an atomic: the outputs equal tests/matching_oracle.py bit
 * for bit and are the same bytes from run to run.  All arrays are host memory.
 *   nidreg_features_detect    image: height rows of width 8-bit pixels, row_stride bytes apart.
 *                             mask (nullable; non-zero = valid, mask_row_stride bytes a row): fill_passes passes first replace every
 *                             invalid pixel that has a valid 3x3 neighbour by the mean of its valid neighbours, rounded half up, and
 *                             mark it valid (each pass reads the previous pass's result only); a keypoint is reported only when its
 *                             level-0 pixel is valid in the mask AS GIVEN (it still suppresses its neighbours).
 *                             Pyramid: level l + 1 = bilinear from level l at ratio 6/5 -- destination x at source (12 x + 1) / 10, weights
 *                             in tenths, (sum + 50) / 100, taps clamped --, size floor(5 size / 6); a level with a side <= 32 and all
 *                             above it hold no keypoint and are not built.  Descriptors read a smoothed copy of the level: the separable
 *                             binomial [1 4 6 4 1] along x and y (the 5 x 5 kernel of weight 256) rounded once, (sum + 128) >> 8, borders
 *                             replicated.  Detector (on the unsmoothed level): a pixel is a corner at threshold t when 9 contiguous
 *                             pixels of the 16-pixel radius-3 circle are all >= centre + t or all <= centre - t; its score is the largest
 *                             such t (0: none); pixels closer than 16 to the level's edge score 0.  A pixel with score >= fast_threshold
 *                             survives when no pixel of its (2 nms_radius + 1)^2 window scores higher and no earlier one in (y, x) order
 *                             scores the same.  Survivors are ordered by (score descending, level, y, x) with a radix sort of one 64-bit
 *                             key each; the first max_keypoints are kept (-1: all, capped at NIDREG_FEATURES_CAPACITY; the output arrays
 *                             must hold that many).  kpts_out: n x {x0, y0, level, score}, x0 = ((2 x + 1) 6^l) / (2 5^l) in integer
 *                             division clamped to the image (y0 alike); desc_out: n x 8 words, bit k of word k / 32 set when the first
 *                             sample of BRIEF pair k (csrc/nid_brief_table.hpp, offsets in [-15, 15]^2 around the keypoint on the smoothed
 *                             level) is less than the second.  No orientation: in-plane rotation is the caller's (find_matches
 *                             --rotate_camera / --rotate_lidar).  *count_out = n.
 *   nidreg_features_match     per row descriptor of desc0 the best and second-best Hamming distance over desc1 (a tie goes to the lowest
 *                             column; one column: second = 257), the same with the sides swapped, then match01_out[i] = j when j is i's
 *                             best, i is j's best, d1 <= max_distance and d1 ratio_den < d2 ratio_num; else -1.  dist_out[i] = d1 whether
 *                             accepted or not, second_out (nullable) = d2.  n0 == 0 or n1 == 0 is valid: no match (distances 257), no
 *                             launch.
 * NIDREG_ERR_INVALID before any device call: a NULL array, a non-positive size (or one above 32768), a stride below the width,
 * levels outside [1, 16], fast_threshold outside [1, 255], nms_radius outside [0, 16], fill_passes outside [0, 64], max_keypoints 0
 * or above the capacity, ratio_den <= 0, ratio_num < 0, max_distance < 0, a negative descriptor count. */
#define NIDREG_FEATURES_CAPACITY 65536
int nidreg_features_detect(int device_id, const uint8_t* image, int width, int height, int64_t row_stride, const uint8_t* mask /* nullable */, int64_t mask_row_stride, int levels,
                           int fast_threshold, int nms_radius, int fill_passes, int max_keypoints, int32_t* kpts_out /* n x 4: x0 y0 level score */, uint32_t* desc_out /* n x 8 */,
                           int32_t* count_out);
int nidreg_features_match(int device_id, const uint32_t* desc0, int n0, const uint32_t* desc1, int n1, int max_distance, int ratio_num, int ratio_den,
                          int32_t* match01_out /* n0: column or -1 */, int32_t* dist_out /* n0: best distance */, int32_t* second_out /* n0, nullable */);

/* ---- baseline JPEG images to 8-bit gray ------------------------------------------------------------------------------------------
 * The reference reads its camera image with cv::imread(image_path, 0) (src/preprocess_map.cpp:69) and, from a bag, with
 * cv_bridge::toCvCopy(*msg, "mono8") (src/preprocess_ros1.cpp:104-134); for JPEG bytes the two give DIFFERENT gray values, and this
 * decoder has a mode for each:
 *   NIDREG_JPEG_GRAY_LUMA   cv::imread(path, 0): libjpeg is asked for JCS_GRAYSCALE and returns the Y plane; chroma is never decoded
 *                           (no chroma kernel is launched).  EXIF orientation is NOT applied here (dataset.read_image_gray applies it).
 *   NIDREG_JPEG_GRAY_BGR    cv_bridge: decode to BGR -- fancy chroma upsampling, libjpeg's YCbCr -> RGB tables --, then OpenCV's
 *                           fixed-point luma (4899 R + 9617 G + 1868 B + 8192) >> 14.
 * A one-component stream gives its plane in both modes.  Marker parsing and Huffman decoding run on the host
 * (csrc/nid_jpeg_host.hpp); dequantisation, libjpeg's jpeg_idct_islow, upsampling, colour and luma are integer device kernels
 * (csrc/nid_jpeg_kernels.hpp, which states the arithmetic).  The outputs equal tests/jpeg_oracle.py bit for bit.
 * PINNED against libjpeg-turbo as Pillow bundles it (tests/golden/jpeg_cases.npz) plus this project's luma constants; UNPINNED
 * against OpenCV itself, which was not available to compare with.
 * Accepted: SOF0, and SOF1 with 8-bit samples and Huffman coding; 1 component, or 3 coded as YCbCr (libjpeg's rule: a JFIF marker or
 * no marker at all means YCbCr, an Adobe APP14 marker must say transform 1); one interleaved scan; chroma sampled 1x1 with luma 1x1
 * (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0); DQT with 8- or 16-bit entries; several tables per DHT / DQT segment and redefinition before
 * SOS; DRI with RST0-7; 0xFF00 stuffing and 0xFF fill bytes before markers; APPn and COM are skipped; whatever follows the last MCU
 * (EOI or not) is ignored.
 * Refused with NIDREG_ERR_INVALID, nothing written and BEFORE any device call (all parsing, entropy decoding included, comes first),
 * the message being "<function>: JPEG images are not decoded here unless they are baseline 8-bit Huffman streams (<reason>)":
 * progressive, arithmetic-coded, lossless, hierarchical and 12-bit streams; 4 components, Adobe transform 0 (RGB) or 2 (YCCK),
 * component identifiers R G B without a marker; a scan that holds only some of the components; every other sampling combination
 * (4:4:0, 4:1:1, ...); a width or height of 0 or above 32768; a missing table; a Huffman table that is no prefix code.
 * DELIBERATE DIFFERENCES from libjpeg, which decodes on with a warning in each case: entropy data that ends before the last MCU
 * (libjpeg pads with zero bits), a Huffman code that does not exist (libjpeg substitutes 0), a zero run that carries a coefficient
 * past position 63 (libjpeg stores it at 63) and a restart marker that is missing or out of sequence (libjpeg resynchronises) are
 * all refused.  RANGE LIMIT: the inverse DCT saturates to [0, 255] like libjpeg-turbo's SIMD code, where libjpeg's C table wraps
 * modulo 1024 beyond +-512; beyond the domain in which the SIMD code's int16 intermediates hold (dequantised coefficients and
 * column-pass outputs within int16) the result is this decoder's own (int32 throughout) and pinned to nothing.
 *   nidreg_jpeg_info          host only.  subsampling: NIDREG_JPEG_SUB_*; exif_orientation: tag 0x0112 of the first Exif APP1 segment
 *                             (big- or little-endian TIFF header), 1 when absent or outside 1..8.  Any output may be NULL.
 *   nidreg_jpeg_coefficients  host only: the QUANTISED blocks of one component, 64 int16 in natural (row-major) order per block, in
 *                             raster order over the component's whole block grid -- ceil(width / (8 hmax)) * h blocks a row,
 *                             ceil(height / (8 vmax)) * v rows --, and its quantisation table in natural order (nullable).  capacity:
 *                             int16 values `out` holds.  The entropy stage can be checked with it on a machine without a GPU.
 *   nidreg_jpeg_decode_gray   out: height rows of width bytes, row_stride bytes apart (0: packed); bytes between rows are not
 *                             written.  data and out are host memory.
 *   nidreg_jpeg_get_timing    host wall-clock milliseconds of the calling thread's last nidreg_jpeg_decode_gray: [0] parsing and
 *                             entropy decode, [1] allocation and upload, [2] kernels (launch to idle), [3] copy back. */
#define NIDREG_JPEG_GRAY_LUMA 0
#define NIDREG_JPEG_GRAY_BGR 1
#define NIDREG_JPEG_SUB_GRAY 0
#define NIDREG_JPEG_SUB_444 1
#define NIDREG_JPEG_SUB_422 2
#define NIDREG_JPEG_SUB_420 3
int nidreg_jpeg_info(const uint8_t* data, int64_t size, int32_t* width, int32_t* height, int32_t* components, int32_t* subsampling, int32_t* exif_orientation);
int nidreg_jpeg_coefficients(const uint8_t* data, int64_t size, int component, int16_t* out, int64_t capacity, uint16_t* qtable_out /* 64, nullable */);
int nidreg_jpeg_decode_gray(int device_id, const uint8_t* data, int64_t size, int mode, uint8_t* out, int64_t row_stride);
int nidreg_jpeg_get_timing(double* ms4);

/* ---- raw sensor_msgs/Image encodings to 8-bit gray (csrc/nid_raw_kernels.hpp; Python: rosbag1.image_to_mono8) ---------------------
 * What cv_bridge::toCvCopy(msg, "mono8") (src/preprocess_ros1.cpp:126-135) makes of an uncompressed image: besides the five 8-bit
 * encodings, the Bayer mosaics, packed YUV 4:2:2 and the 16-bit images machine-vision cameras publish on image_raw.  Stateless; data
 * and out are host memory; integer arithmetic only on the device (unsigned 32-bit), one launch, no atomics: the same bytes on every
 * run, restated byte for byte in tests/raw_image_oracle.py.  The rules below restate cv_bridge and OpenCV (the bilinear Bayer2Gray,
 * channel extraction for packed YUV, convertTo for the depth change) from memory: the result is UNPINNED against OpenCV and
 * cv_bridge, neither of which was available to compare with.
 * SOURCE  data: the message's bytes as stored, height rows of step bytes (size of them at least height * step); step may be odd and
 * data may lie at any address.  luma(R, G, B) = (4899 R + 9617 G + 1868 B + 8192) >> 14.
 * DEPTH CHANGE  every 16-bit encoding ends with (v + 128) / 257, floored: cv_bridge's convertTo(CV_8U, 255 / 65535) in float32 with
 * round-half-even, for all 65536 values.  With is_bigendian != 0 every 16-bit sample is byte-swapped first; 8-bit encodings ignore it.
 *   mono8, mono16                     the sample (mono16: the depth change alone)
 *   rgb8 bgr8 rgba8 bgra8             luma; alpha is ignored (the bytes rosbag1.to_mono8 gives)
 *   rgb16 bgr16 rgba16 bgra16         luma on the 16-bit samples, then the depth change
 *   yuv422, uyvy                      two bytes a pixel: byte 2x + 1 of the row, the stored Y without range scaling
 *   yuv422_yuy2, yuyv                 byte 2x; any width
 *   bayer_{rggb,bggr,gbrg,grbg}{8,16} the four letters are the colours of row 0 (columns 0, 1), then row 1 (columns 0, 1) of the
 *                                     mosaic p.  Interior pixel (1 <= x <= W - 2, 1 <= y <= H - 2), c_r, c_g, c_b = 4899, 9617, 1868:
 *       at a red or blue pixel of colour C (O the other of the two)
 *           (c_C 4p + c_g (left + right + up + down) + c_O (sum of the four diagonal neighbours) + 2^15) >> 16
 *       at a green pixel whose horizontal neighbours have colour Ch and whose vertical neighbours have colour Cv
 *           (c_Ch (left + right) + c_Cv (up + down) + c_g 2p + 2^14) >> 15
 *     -- the bilinear demosaic and the luma with ONE rounding.  A border pixel takes the value of the interior pixel at
 *     (clamp(x, 1, W - 2), clamp(y, 1, H - 2)), the pattern's phase being that of the clamped coordinate: row 0 repeats row 1, a
 *     corner its diagonal neighbour.  The 16-bit mosaics: the same on 16-bit samples, then the depth change.
 * Refused with NIDREG_ERR_INVALID, nothing written and BEFORE any device call: every other encoding -- 8UC1, 16UC1, 32FC1, nv21,
 * nv24, ...; cv_bridge refuses the generic types for this target too --, the message being "nidreg_image_to_mono8: sensor_msgs/Image
 * encoding '<enc>' is not converted here (<the list> are)"; a width or height outside [1, 16384]; a mosaic with W < 3 or H < 3 (no
 * interior: a DELIBERATE DIFFERENCE); a step below W * bytes per pixel; size below height * step; a NULL pointer; an out_row_stride
 * below the width (0 means packed).
 *   nidreg_image_to_mono8    out: height rows of width bytes, out_row_stride bytes apart; bytes between rows are not written.
 *   nidreg_image_get_timing  host wall-clock milliseconds of the calling thread's last nidreg_image_to_mono8: [0] allocation and
 *                            upload, [1] the kernel (launch to idle), [2] copy back. */
int nidreg_image_to_mono8(int device_id, const uint8_t* data, int64_t size, int width, int height, int64_t step, const char* encoding, int is_bigendian, uint8_t* out,
                          int64_t out_row_stride);
int nidreg_image_get_timing(double* ms3);

/* ---- Velodyne data packets to point records (csrc/nid_packet_kernels.hpp; Python: lidar_messages.py) ----------------------------
 * What the vendor driver does between a bag of velodyne_msgs/VelodyneScan -- the raw UDP packets, 3 bytes a return -- and
 * extract_raw_points (ros_cloud_converter.hpp): velodyne_pointcloud's RawData::unpack / unpack_vlp16, which turn packets into the
 * x, y, z, intensity, time cloud the reference expects on its points topic.  Stateless (the device keeps only two 36000-entry
 * cosine / sine tables, built once on the host with libm); all pointers are host memory; one workgroup per packet, no atomics: the
 * same bytes on every run, restated byte for byte in tests/velodyne_oracle.py.  The rules restate the VLP-16 / HDL-32E manuals
 * and velodyne_pointcloud's rawdata.cc from memory: the result is UNPINNED against velodyne_pointcloud and real recordings.
 * SOURCE  packets: num_packets packets of 1206 data bytes, packet_stride bytes apart (1214 in a ROS1 message, 1216 in CDR), at any
 * address; little-endian.  A packet is 12 blocks of 100 bytes -- uint16 flag (bytes FF EE), uint16 azimuth a[b] in 0.01 degree,
 * 32 x (uint16 distance, uint8 reflectivity) --, the device's timestamp (4 bytes, unused), the return mode and the product id.
 * OUTPUT  record (packet * 12 + block) * 32 + slot -- the byte order of the packet -- is 5 float32: x y z intensity time.
 *   num_lasers 16 (two firings a block)  f = s / 16, l = s % 16, firing k = 2b + f; diff[b] = (a[b+1] - a[b] + 36000) % 36000 for
 *                                        b < 11, diff[11] = diff[10], whatever the flags; % is the FLOORED modulo (Python's), so
 *                                        diff and az lie in [0, 35999] for ANY uint16 azimuth fields, 36000..65535 included; az = (a[b] + (2 diff[b] (l + 24 f) + 48)
 *                                        / 96) % 36000, floored: the driver's interpolation by (2.304 l + 55.296 f) / 110.592,
 *                                        rounded half up
 *   num_lasers 32 (one firing a block)   l = s, k = b, az = a[b] % 36000
 *   time = float32(packet_times[p] + (k firing_period + l laser_period)), in double, in that order
 *   a block whose flag is not 0xEEFF, or a raw distance of 0: x = y = z = quiet NaN (0x7FC00000), intensity 0, the time as above
 *   else, in fp64 without contraction, with C, S = cos, sin of az * (pi / 18000) from the tables and the laser's row of `lasers`
 *   (cos_vert, sin_vert, cos_rot_corr, sin_rot_corr, vert_offset, horiz_offset, dist_corr, 0):
 *       d = raw distance_resolution + dist_corr;  cr = C cos_rc + S sin_rc;  sr = S cos_rc - C sin_rc;  xy = d cos_v - voff sin_v
 *       xv = xy sr - hoff cr;  yv = xy cr + hoff sr;  zv = d sin_v + voff cos_v
 *       x = float32(yv), y = float32(-xv), z = float32(zv) (the driver's turn into the ROS frame), intensity = float32(reflectivity)
 *   returns_per_packet (nullable): per packet, the number of records that are not "no return".
 * Refused with NIDREG_ERR_INVALID and a message, before the device is touched and with nothing written: num_lasers other than 16 or
 * 32; packet_stride below 1206 or above 4096; num_packets outside [0, 65536]; a NULL packets, packet_times, lasers or records_out with
 * num_packets > 0; a table entry, resolution or period that is not finite.  num_packets == 0 succeeds without a device.
 *   nidreg_velodyne_get_timing  host wall-clock milliseconds of the calling thread's last nidreg_velodyne_decode: [0] allocation and
 *                               upload, [1] the kernel (launch to idle), [2] copy back. */
int nidreg_velodyne_decode(int device_id, const uint8_t* packets, int64_t num_packets, int64_t packet_stride, const double* packet_times, const double* lasers, int num_lasers,
                           double distance_resolution, double firing_period, double laser_period, float* records_out, int32_t* returns_per_packet);
int nidreg_velodyne_get_timing(double* ms3);

/* ---- Ouster lidar packets to point records (csrc/nid_ouster_kernels.hpp; Python: lidar_messages.py) ------------------------------
 * What ouster_ros does between a bag of ouster_ros/PacketMsg -- one UDP packet a message, batched into scans by the caller -- and
 * extract_raw_points: the packets of one scan become 32-byte point records.  Stateless (nothing stays on a device); all pointers
 * are host memory; one workgroup per column, no atomics: the same bytes on every run, restated byte for byte in
 * tests/ouster_oracle.py.  The layouts and the geometry restate the sensor's software manual and the SDK's field tables from
 * memory: the result is UNPINNED against ouster_ros, the Ouster SDK and real recordings.
 * SOURCE  packets: num_packets packets, packet_stride bytes apart, at any address; little-endian.  H pixels per column, C columns
 * per packet, W columns per frame.
 *   NIDREG_OUSTER_LEGACY  no packet header.  A column is 16 + 12 H + 4 bytes: uint64 timestamp [ns] @0, uint16 measurement_id @8,
 *       uint16 frame_id @10, uint32 encoder @12 (unused); H pixels of 12 bytes -- range = uint32 @0 & 0x000FFFFF [mm], reflectivity
 *       uint16 @4, signal uint16 @6, near_ir uint16 @8 --; a uint32 status, the column being valid iff it is 0xFFFFFFFF.
 *       Packet: C (20 + 12 H) bytes.
 *   NIDREG_OUSTER_RNG19_RFL8_SIG16_NIR16  32-byte packet header (frame_id: uint16 @2), 32-byte footer, both ignored here.  A column
 *       is 12 + 12 H bytes: uint64 timestamp @0, uint16 measurement_id @8, uint16 status @10, valid iff bit 0 is set; pixels of 12
 *       bytes -- range = uint32 @0 & 0x0007FFFF, reflectivity uint8 @4, signal uint16 @6, near_ir uint16 @8.  Packet: 64 + C (12 + 12 H).
 *   NIDREG_OUSTER_RNG15_RFL8_NIR8  the same headers; pixels of 4 bytes -- range = (uint16 @0 & 0x7FFF) << 3, reflectivity uint8 @2,
 *       near_ir = uint8 @3 << 4, signal = 0.  Packet: 64 + C (12 + 4 H).
 * TABLES  the caller's, built with libm: column_table[m] = (cos E, sin E), E = 2 pi (1 - m / W), m = 0..W-1; beam_table[i] =
 * (cos A, sin A, cos P, sin P), A = -radians(beam_azimuth_angles[i]), P = radians(beam_altitude_angles[i]), i = 0..H-1; n_mm =
 * lidar_origin_to_beam_origin_mm; transform12 = the first three rows of the row-major 4 x 4 lidar_to_sensor_transform (R00 R01 R02 t0,
 * R10 ..., millimetres), or of the identity for records in the lidar frame.
 * OUTPUT  record (packet * C + column) * H + pixel -- the byte order of the packets, NOT the driver's destaggered H x W image -- is
 * 32 bytes: x, y, z float32 [m] @0 4 8, intensity float32 @12 (= signal), t uint32 [ns] @16, reflectivity uint16 @20, ring uint16 @22
 * (= pixel), ambient uint16 @24 (= near_ir), zero @26..27, range uint32 [mm] @28.
 *   t = min(timestamp - ts0, 2^32 - 1) in unsigned 64-bit arithmetic; the caller passes the smallest timestamp of the valid columns
 *   a pixel is "no return" when its column is not valid, or measurement_id >= W (the column table is then not read), or range = 0:
 *   x = y = z = quiet NaN (0x7FC00000), every other field zero but ring and t
 *   else, in fp64 without contraction, m = measurement_id, (cosE, sinE) = column_table[m], (cosA, sinA, cosP, sinP) = beam_table[i]:
 *       c = cosE cosA - sinE sinA;  s = sinE cosA + cosE sinA;  d = double(range) - n
 *       lx = d (c cosP) + n cosE;  ly = d (s cosP) + n sinE;  lz = d sinP
 *       X = ((R00 lx + R01 ly) + R02 lz) + t0, rows 1 and 2 alike;  x = float32(X 0.001)
 *   returns_per_packet (nullable): per packet, the number of records that are not "no return".
 * Refused with NIDREG_ERR_INVALID and a message, before the device is touched and with nothing written: a profile other than the
 * three; H not 16, 32, 64 or 128; W outside [16, 4096]; C outside [1, 16]; packet_stride below the packet size or above 32768;
 * num_packets outside [0, 4096]; a NULL packets, column_table, beam_table, transform12 or records_out with num_packets > 0; a table
 * entry, transform entry or n_mm that is not finite.  num_packets == 0 succeeds without a device.
 *   nidreg_ouster_get_timing  host wall-clock milliseconds of the calling thread's last nidreg_ouster_decode: [0] allocation and
 *                             upload, [1] the kernels (launch to idle), [2] copy back. */
#define NIDREG_OUSTER_LEGACY 0
#define NIDREG_OUSTER_RNG19_RFL8_SIG16_NIR16 1
#define NIDREG_OUSTER_RNG15_RFL8_NIR8 2
int nidreg_ouster_decode(int device_id, const uint8_t* packets, int64_t num_packets, int64_t packet_stride, int profile, int H, int W, int C, const double* column_table,
                         const double* beam_table, double n_mm, const double* transform12, uint64_t ts0, void* records_out, int32_t* returns_per_packet);
int nidreg_ouster_get_timing(double* ms3);

/* ---- match pictures: a 2-D primitive rasteriser (csrc/nid_draw_kernels.hpp; Python: draw.py) ------------------------------------
 * What find_matches --picture and initial_guess_auto --picture draw with, in place of the reference script's OpenCV calls
 * (scripts/find_matches_superglue.py: both images side by side, keypoints circled, matches as lines).  Stateless; all pointers are
 * host memory; integer arithmetic only on the device, so the picture is the same on every run and restated byte for byte in
 * tests/draw_oracle.py.
 * CANVAS  out_rgb: left_h rows of canvas_w pixels of 3 bytes (R, G, B), packed.  canvas_w = left_w when right_gray is NULL (right_w,
 * right_h and right_row_stride are then ignored), else 2 * left_w.  Left panel: the gray value in all three channels.  Right panel:
 * the right image resized to left_w x left_h by exact integer bilinear interpolation with pixel-centre alignment -- per axis, for
 * destination index i and sizes n_d (destination) and n_s (source): num = (2 i + 1) n_s - n_d, den = 2 n_d, i0 = floor(num / den),
 * f = num - i0 den, the taps i0 (weight den - f) and i0 + 1 (weight f) clamped to [0, n_s - 1]; the value is
 * (sum of taps x weights + den_x den_y / 2) / (den_x den_y), floored, in 64-bit integers.  Equal sizes give the identity.
 * PRIMITIVES  8 int32 each: {kind, x0, y0, a, b, rgb (0xRRGGBB), reserved, reserved}; the reserved words are ignored.  Coordinates
 * are relative to the whole canvas (a caller that draws on the right panel adds left_w itself).  A pixel outside the canvas is
 * dropped on its own, not the primitive with it.
 *   NIDREG_DRAW_LINE  from (x0, y0) to (a, b): n = max(|dx|, |dy|); for k = 0..n the pixel
 *                     (x0 + sgn(dx) ((2 k |dx| + n) / (2 n)), y0 + sgn(dy) ((2 k |dy| + n) / (2 n))), divisions floored; n = 0 is the one
 *                     pixel.  Every k stands on its own and the line is defined FROM its first point: the reversed line may cover
 *                     other pixels.  Not symmetrised, not anti-aliased, one pixel wide.
 *   NIDREG_DRAW_RING  centre (x0, y0), radius a (b is ignored): with d2 = dx^2 + dy^2 the pixels of 4 d2 < (2 a + 1)^2 and
 *                     (a == 0 or 4 d2 >= (2 a - 1)^2) -- 1, 8, 12, 16 pixels at radius 0, 1, 2, 3.
 *   NIDREG_DRAW_DISC  4 d2 < (2 a + 1)^2.
 * ORDER  the painter's rule: where several primitives cover a pixel, the one with the LARGEST index in prims wins, on every run.
 * Refused with NIDREG_ERR_INVALID and a message, before the device is touched and with nothing written: a NULL left_gray or
 * out_rgb, or NULL prims with num_prims > 0; a width or height outside [1, 16384]; a row stride below the width; num_prims outside
 * [0, 2^24]; an unknown kind; a coordinate outside [-32768, 32767]; a radius outside [0, 16]; rgb above 0xFFFFFF. */
#define NIDREG_DRAW_LINE 0
#define NIDREG_DRAW_RING 1
#define NIDREG_DRAW_DISC 2
int nidreg_draw(int device_id, const uint8_t* left_gray, int left_w, int left_h, int64_t left_row_stride, const uint8_t* right_gray /* nullable */, int right_w, int right_h,
                int64_t right_row_stride, int64_t num_prims, const int32_t* prims /* 8 int32 per primitive */, uint8_t* out_rgb /* left_h x canvas_w x 3 */);

/* ---- split-phase evaluation for a pair whose points are sharded across GPUs --------------
 * rank r:  nidreg_shard_hist(h, se3)      zero + accumulate this shard's fixed-point histogram
 *          <caller: all-reduce(sum, int64) of ext_hist over ranks, ordered on ext_stream>
 *          nidreg_shard_entropy(h)        entropy tail on the full histogram -> cost
 *          nidreg_shard_grad(h)           this shard's gradient partial -> out[1..7]
 *          <caller: all-reduce(sum, f64) of out[1..7]>
 *          nidreg_shard_finish(h, ...)    stream sync + read back
 * All shard calls are asynchronous on the handle's stream except nidreg_shard_finish. */
/* 64-bit words in a histogram buffer (desc.ext_hist must hold this many): bins*bins joint cells [bin_points][bin_image], 8 tail
 * words (0: inlier count, 1: fixed-point joint entropy), roundup8(bins) column sums (added by the histogram kernels' flush) and
 * roundup8(bins) row sums (added by k_entropy) -- bins*bins + 8 + 2*roundup8(bins) */
int64_t nidreg_hist_words(int bins);
int nidreg_shard_hist(nidreg_handle* h, const double* se3);
int nidreg_shard_entropy(nidreg_handle* h);
int nidreg_shard_grad(nidreg_handle* h);
int nidreg_shard_finish(nidreg_handle* h, double* cost, double* grad7);

/* ---- the same protocol with RCCL inside the library (one process per GPU; BASELINE north_star: "disjoint point slices with
 * a final RCCL all-reduce of the 2D histogram over xGMI") -----------------------------------------------------------------
 * Every rank creates a plain handle over ITS slice of the pair's cloud (desc.scale_points = the pair's total point count, so
 * that every rank uses the same fixed-point unit; no ext_hist / ext_out / device_ids) and gives it a communicator; from then on
 * nidreg_eval / nidreg_eval_iso / nidreg_eval_batch on that handle are COLLECTIVE calls (every rank, same pose) that run
 *     histogram kernel -> ncclAllReduce(int64 sum, nidreg_hist_words(bins) words) -> entropy tail ->
 *     gradient kernel  -> ncclAllReduce(float64 sum, 7 words)
 * on the handle's stream.  Replaces nothing in the reference (its only parallelism is the OpenMP loop over pairs,
 * src/vlcal/calib/visual_camera_calibration.cpp:161); the cost is bit-identical on every rank and to the unsharded handle's,
 * the gradient equal up to the order of the partial sums.  librccl.so is opened with dlopen at the first of these calls
 * (NIDREG_RCCL_LIB overrides the name); libnidreg.so does not link it.
 *   nidreg_rccl_unique_id     rank 0: ncclGetUniqueId into 128 bytes, which the caller hands to the other ranks (MPI, a file,
 *                             torch.distributed -- any way it likes)
 *   nidreg_shard_comm_init    every rank: ncclCommInitRank(world_size, id, rank) on the handle's device; the handle owns the
 *                             communicator and destroys it with itself
 *   nidreg_shard_attach_rccl  a communicator the caller owns (an ncclComm_t, passed as void*); NULL detaches
 * Both run ONE collective themselves before they accept the communicator: the ranks' table parameters (fixed-point fraction bits --
 * i.e. desc.scale_points --, bins, nidreg_hist_words, mode) are max-/min-reduced and every rank refuses alike
 * (NIDREG_ERR_INVALID, the handle stays detached) when they differ; a rank created with another unit would otherwise add
 * incompatible integers into a cost that is wrong yet identical on every rank.
 * FAILURE SEMANTICS: an evaluation is a sequence of collectives.  A rank that returns early with a negative status (a launch error,
 * a lost device) leaves its peers inside ncclAllReduce; the caller must then abort the communicator on the other ranks
 * (ncclCommAbort) -- RCCL has no timeout of its own -- and rebuild it before evaluating again. */
#define NIDREG_RCCL_ID_BYTES 128
int nidreg_rccl_unique_id(unsigned char* id128);
int nidreg_shard_comm_init(nidreg_handle* h, int world_size, int rank, const unsigned char* id128);
int nidreg_shard_attach_rccl(nidreg_handle* h, void* nccl_comm);

/* number of GPUs a handle is sharded over (1 = plain handle) and their device ordinals */
int nidreg_num_shards(nidreg_handle* h);
int nidreg_shard_devices(nidreg_handle* h, int* device_ids, int capacity);

/* release what the library keeps per device between handles: the scratch arenas of handle construction (upload staging, sort
 * keys) and the streams / host-mapped result blocks of destroyed handles (the next handle takes them: the reference builds new
 * cost objects in every outer iteration, visual_camera_calibration.cpp:199-208) */
void nidreg_trim(void);

/* device-side timing of the most recent nidreg_eval / nidreg_eval_iso in milliseconds (HIP events
 * recorded on the handle's stream, i.e. the stream the kernels run on):
 * [0]=whole launch sequence [1]=histogram memset [2]=histogram kernel [3]=entropy kernels
 * [4]=gradient kernel (0 if not run) [5]=gradient finalisation.
 * nidreg_set_timing(h, 1): an event after every kernel; (h, 2): only [0], around the whole evaluation; (h, 0): off. */
int nidreg_set_timing(nidreg_handle* h, int enable);
int nidreg_get_timing(nidreg_handle* h, float* ms6);

/* layout facts for DESIGN.md / bench: [0]=record bytes per point on device, [1]=number of chunks,
 * [2]=columns per group, [3]=fixed-point fraction bits, [4]=LDS bytes per workgroup,
 * [5]=padded image pitch, [6]=points stored, [7]=bit0: float32 records, bit1: the gradient-pass chunk table has chunks that run
 * across column groups (the looped kernel instantiations, csrc/nid_kernels.hpp Segments), bit2: so has the WIDE histogram
 * kernel's table, bit3: NEAREST handle whose evaluations use the fast decision tier (plumb_bob with a FoV cone below ~84 degrees,
 * fisheye, omnidir with xi >= 0, equirectangular; the other models and degenerate cones run the exact tier only;
 * csrc/nid_kernels.hpp NearestFast), bit4: cost+Jacobian evaluations launch no entropy kernel (bins <= 32: the gradient workgroups
 * sum the table themselves, csrc/nid_kernels.hpp kSelfEntropyCells), bit5: a synchronous cost+Jacobian evaluation that has its device to
 * itself runs as ONE launch (csrc/nid_fused.hpp: bins <= 32 and a cloud whose chunks fit the LDS stash), bits 8..15: LDS copies per
 * histogram cell, bits 16..27: workgroups of that launch, bit 28: its stash holds the projection context too (not only u, v) */
int nidreg_get_info(nidreg_handle* h, int64_t* info8);

const char* nidreg_last_error(void);
const char* nidreg_version(void);
/* 16 hex digits: sha256 over the kernel sources (csrc/nid_*.hpp, nid_kernels_*.hip, Makefile) this library was BUILT from.  The
 * measurement tooling stamps rocprofv3 summaries with it and refuses to stamp when it differs from the sources next to the library
 * (tools/kernel_stats_json.py, tools/traffic_from_pmc.py): a summary can then only ever describe the kernels that produced it. */
const char* nidreg_kernel_build(void);

#ifdef __cplusplus
}
#endif
#endif /* NIDREG_H */
