"""ctypes loader for csrc/libnidreg.so (the C ABI of include/nidreg.h).

There is no Python or CPU fallback: if the HIP library is missing or no GPU is usable, loading /
handle creation raises.  Build it with ``__graft_entry__.build()`` (``make -C csrc``).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC_DIR = os.path.join(_HERE, "csrc")
# NIDREG_LIB lets development tools (tools/ablate.py) load an instrumented build of the same ABI
LIB_PATH = os.environ.get("NIDREG_LIB", os.path.join(CSRC_DIR, "libnidreg.so"))

NIDREG_OK = 0
NIDREG_FALSE = 1
NIDREG_ERR_INVALID = -1
NIDREG_ERR_FULL = -4
NIDREG_OUT_DOUBLES = 16
FEATURES_CAPACITY = 65536  # NIDREG_FEATURES_CAPACITY
SELECT_TILE = 1024  # NIDREG_SELECT_TILE
FOLD_MAX = 1024  # NIDREG_FOLD_MAX

MODE_SPLINE, MODE_NEAREST = 0, 1
PREC_FP64 = 0  # (1 = NIDREG_PREC_FP32: removed in round 5, refused by nidreg_create)
IMAGE_F64, IMAGE_U8 = 0, 1
FLAG_INPUT_ORDER = 1
FLAG_EXT_STREAM = 2
FLAG_NEAREST_EXACT = 4
JPEG_GRAY_LUMA, JPEG_GRAY_BGR = 0, 1  # NIDREG_JPEG_GRAY_*
JPEG_SUB_GRAY, JPEG_SUB_444, JPEG_SUB_422, JPEG_SUB_420 = 0, 1, 2, 3  # NIDREG_JPEG_SUB_*

c_double_p = ctypes.POINTER(ctypes.c_double)
c_int64_p = ctypes.POINTER(ctypes.c_int64)
c_float_p = ctypes.POINTER(ctypes.c_float)


class NidregDesc(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_int32),
        ("device_id", ctypes.c_int32),
        ("model_id", ctypes.c_int32),
        ("mode", ctypes.c_int32),
        ("precision", ctypes.c_int32),
        ("bins", ctypes.c_int32),
        ("intrinsics", ctypes.c_double * 5),
        ("distortion", ctypes.c_double * 8),
        ("width", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("image_dtype", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("image", ctypes.c_void_p),
        ("image_row_stride", ctypes.c_int64),
        ("num_points", ctypes.c_int64),
        ("points", ctypes.c_void_p),
        ("point_stride", ctypes.c_int64),
        ("intensities", ctypes.c_void_p),
        ("max_fov", ctypes.c_double),
        ("columns_per_group", ctypes.c_int32),
        ("target_blocks", ctypes.c_int32),
        ("lds_copies", ctypes.c_int32),
        ("reserved1", ctypes.c_int32),
        ("scale_points", ctypes.c_int64),
        ("ext_stream", ctypes.c_void_p),
        ("ext_hist", ctypes.c_void_p),
        ("ext_out", ctypes.c_void_p),
        ("num_devices", ctypes.c_int32),
        ("device_ids", ctypes.c_int32 * 16),
    ]


EXPORTS = [
    "nidreg_model_from_name", "nidreg_device_count", "nidreg_create", "nidreg_destroy", "nidreg_cloud_create", "nidreg_cloud_create_f32", "nidreg_cloud_destroy", "nidreg_create_from_cloud", "nidreg_eval", "nidreg_eval_iso", "nidreg_eval_multi",
    "nidreg_eval_iso_multi", "nidreg_get_hist", "nidreg_get_hist_fixed", "nidreg_project", "nidreg_project_model", "nidreg_view_culling", "nidreg_hist_words", "nidreg_shard_hist",
    "nidreg_shard_entropy", "nidreg_shard_grad", "nidreg_shard_finish", "nidreg_set_timing", "nidreg_get_timing", "nidreg_get_info", "nidreg_last_error",
    "nidreg_version", "nidreg_colorizer_create", "nidreg_colorizer_update", "nidreg_colorizer_device_colors", "nidreg_colorizer_destroy", "nidreg_generate_lidar_image",
    "nidreg_equalize_intensities", "nidreg_num_shards", "nidreg_shard_devices", "nidreg_trim", "nidreg_eval_batch", "nidreg_submit", "nidreg_submit_iso", "nidreg_wait", "nidreg_eval_pipelined",
    "nidreg_estimate_camera_fov", "nidreg_rccl_unique_id", "nidreg_shard_comm_init", "nidreg_shard_attach_rccl", "nidreg_kernel_build",
    "nidreg_estimate_directions", "nidreg_ransac_sample_pairs", "nidreg_estimate_rotation_ransac",
    "nidreg_integrator_create", "nidreg_integrator_insert", "nidreg_integrator_insert_f32", "nidreg_integrator_insert_cloud2", "nidreg_integrator_size", "nidreg_integrator_get", "nidreg_integrator_info",
    "nidreg_integrator_destroy", "nidreg_integrator_insert_las", "nidreg_integrator_las_timing", "nidreg_lzf_decompress",
    "nidreg_odom_create", "nidreg_odom_destroy", "nidreg_odom_knn_covariances", "nidreg_odom_covariances", "nidreg_odom_model_insert", "nidreg_odom_model_info", "nidreg_odom_model_get", "nidreg_odom_set_lru", "nidreg_odom_lru_info",
    "nidreg_odom_set_source", "nidreg_odom_linearize", "nidreg_odom_error", "nidreg_odom_correspondences", "nidreg_odom_deskew_insert",
    "nidreg_features_detect", "nidreg_features_match",
    "nidreg_splat_create", "nidreg_splat_set_colors", "nidreg_splat_draw", "nidreg_splat_destroy",
    "nidreg_jpeg_info", "nidreg_jpeg_coefficients", "nidreg_jpeg_decode_gray", "nidreg_jpeg_get_timing",
    "nidreg_image_to_mono8", "nidreg_image_get_timing",
    "nidreg_velodyne_decode", "nidreg_velodyne_get_timing",
    "nidreg_ouster_decode", "nidreg_ouster_get_timing",
    "nidreg_draw",
    "nidreg_mask_create", "nidreg_mask_get", "nidreg_mask_destroy", "nidreg_cloud_select", "nidreg_cloud_select_counts", "nidreg_cloud_size", "nidreg_cloud_get",
    "nidreg_cloud_fold_ids", "nidreg_cloud_fold",
]

_lib = None


def load():
    """Load libnidreg.so.  Raises (loudly) when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: the NID core has no CPU fallback; run __graft_entry__.build() (make -C {CSRC_DIR})")
    lib = ctypes.CDLL(LIB_PATH)
    lib.nidreg_last_error.restype = ctypes.c_char_p
    lib.nidreg_version.restype = ctypes.c_char_p
    lib.nidreg_hist_words.restype = ctypes.c_int64
    lib.nidreg_hist_words.argtypes = [ctypes.c_int]
    lib.nidreg_destroy.restype = None
    lib.nidreg_destroy.argtypes = [ctypes.c_void_p]
    lib.nidreg_create.argtypes = [ctypes.POINTER(NidregDesc), ctypes.POINTER(ctypes.c_void_p)]
    lib.nidreg_cloud_create.argtypes = [ctypes.c_int, c_double_p, ctypes.c_int64, c_double_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p)]
    lib.nidreg_cloud_create_f32.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p)]
    lib.nidreg_cloud_destroy.restype = None
    lib.nidreg_cloud_destroy.argtypes = [ctypes.c_void_p]
    lib.nidreg_create_from_cloud.argtypes = [ctypes.POINTER(NidregDesc), ctypes.c_void_p, c_double_p, ctypes.c_double, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    lib.nidreg_eval.argtypes = [ctypes.c_void_p, c_double_p, c_double_p, c_double_p]
    lib.nidreg_eval_iso.argtypes = [ctypes.c_void_p, c_double_p, c_double_p]
    lib.nidreg_eval_batch.argtypes = [ctypes.c_void_p, c_double_p, ctypes.c_int, c_double_p, c_double_p]
    lib.nidreg_eval_pipelined.argtypes = [ctypes.c_void_p, c_double_p, ctypes.c_int, c_double_p, c_double_p]
    lib.nidreg_submit.argtypes = [ctypes.c_void_p, c_double_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]
    lib.nidreg_submit_iso.argtypes = [ctypes.c_void_p, c_double_p, ctypes.POINTER(ctypes.c_int64)]
    lib.nidreg_wait.argtypes = [ctypes.c_void_p, ctypes.c_int64, c_double_p, c_double_p]
    lib.nidreg_eval_multi.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p]
    lib.nidreg_eval_iso_multi.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, c_double_p, c_double_p]
    lib.nidreg_get_hist.argtypes = [ctypes.c_void_p, c_double_p, c_double_p, c_double_p]
    lib.nidreg_get_hist_fixed.argtypes = [ctypes.c_void_p, c_int64_p, c_int64_p, ctypes.POINTER(ctypes.c_int)]
    lib.nidreg_project.argtypes = [ctypes.c_void_p, c_double_p, ctypes.c_int64, c_double_p, c_double_p]
    lib.nidreg_project_model.argtypes = [ctypes.c_int, c_double_p, c_double_p, ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_int64, c_double_p, c_double_p]
    lib.nidreg_view_culling.restype = ctypes.c_int64
    lib.nidreg_view_culling.argtypes = [ctypes.c_int, c_double_p, c_double_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, c_double_p, ctypes.c_int64,
                                        ctypes.c_int64, c_double_p, ctypes.POINTER(ctypes.c_int32)]
    lib.nidreg_shard_hist.argtypes = [ctypes.c_void_p, c_double_p]
    lib.nidreg_shard_entropy.argtypes = [ctypes.c_void_p]
    lib.nidreg_shard_grad.argtypes = [ctypes.c_void_p]
    lib.nidreg_shard_finish.argtypes = [ctypes.c_void_p, c_double_p, c_double_p]
    lib.nidreg_set_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.nidreg_get_timing.argtypes = [ctypes.c_void_p, c_float_p]
    lib.nidreg_get_info.argtypes = [ctypes.c_void_p, c_int64_p]
    lib.nidreg_model_from_name.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.nidreg_colorizer_create.argtypes = [ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, c_double_p,
                                            ctypes.c_int64, c_float_p, ctypes.c_double, ctypes.POINTER(ctypes.c_void_p)]
    lib.nidreg_colorizer_update.argtypes = [ctypes.c_void_p, c_double_p, ctypes.c_double, c_float_p]
    lib.nidreg_colorizer_device_colors.restype = ctypes.c_void_p
    lib.nidreg_colorizer_device_colors.argtypes = [ctypes.c_void_p]
    lib.nidreg_colorizer_destroy.restype = None
    lib.nidreg_colorizer_destroy.argtypes = [ctypes.c_void_p]
    lib.nidreg_generate_lidar_image.argtypes = [ctypes.c_int, c_double_p, c_double_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, c_double_p, ctypes.c_int64, c_double_p,
                                                ctypes.c_int64, c_double_p, c_double_p, ctypes.POINTER(ctypes.c_int32)]
    lib.nidreg_equalize_intensities.argtypes = [ctypes.c_int, c_double_p, ctypes.c_int64]
    lib.nidreg_num_shards.argtypes = [ctypes.c_void_p]
    lib.nidreg_shard_devices.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    lib.nidreg_trim.restype = None
    lib.nidreg_trim.argtypes = []
    lib.nidreg_estimate_camera_fov.argtypes = [ctypes.c_int, c_double_p, c_double_p, ctypes.c_int, ctypes.c_int, c_double_p]
    lib.nidreg_estimate_directions.argtypes = [ctypes.c_int, c_double_p, c_double_p, c_double_p, ctypes.c_int64, c_double_p]
    lib.nidreg_ransac_sample_pairs.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int32)]
    lib.nidreg_estimate_rotation_ransac.argtypes = [ctypes.c_int, c_double_p, c_double_p, ctypes.c_int, c_double_p, c_double_p, c_double_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double,
                                                    ctypes.c_uint64, ctypes.POINTER(ctypes.c_int32), c_double_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                                    ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32)]
    lib.nidreg_integrator_create.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_void_p)]
    lib.nidreg_integrator_insert.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
    lib.nidreg_integrator_insert_f32.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64]
    lib.nidreg_integrator_insert_cloud2.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                    ctypes.c_int32, c_int64_p]
    lib.nidreg_integrator_insert_las.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, c_double_p, c_double_p, c_double_p, ctypes.c_int32,
                                                 ctypes.POINTER(ctypes.c_uint64), ctypes.c_int32, c_int64_p]
    lib.nidreg_integrator_las_timing.argtypes = [c_double_p]
    lib.nidreg_lzf_decompress.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, c_int64_p]
    lib.nidreg_integrator_size.argtypes = [ctypes.c_void_p, c_int64_p]
    lib.nidreg_integrator_get.argtypes = [ctypes.c_void_p, c_float_p, c_int64_p]
    lib.nidreg_integrator_info.argtypes = [ctypes.c_void_p, c_int64_p]
    lib.nidreg_integrator_destroy.restype = None
    lib.nidreg_integrator_destroy.argtypes = [ctypes.c_void_p]
    c_int32_p = ctypes.POINTER(ctypes.c_int32)
    lib.nidreg_odom_create.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]
    lib.nidreg_odom_destroy.restype = None
    lib.nidreg_odom_destroy.argtypes = [ctypes.c_void_p]
    lib.nidreg_odom_knn_covariances.argtypes = [ctypes.c_void_p, c_double_p, ctypes.c_int32, ctypes.c_int32, c_int32_p, c_double_p, c_double_p]
    lib.nidreg_odom_covariances.argtypes = [ctypes.c_void_p, c_double_p, ctypes.c_int32, ctypes.c_int32, c_int32_p, c_double_p, c_double_p]
    lib.nidreg_odom_model_insert.argtypes = [ctypes.c_void_p, c_double_p, c_double_p, ctypes.c_int32]
    lib.nidreg_odom_model_info.argtypes = [ctypes.c_void_p, c_int64_p]
    lib.nidreg_odom_set_lru.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
    lib.nidreg_odom_lru_info.argtypes = [ctypes.c_void_p, c_int64_p]
    lib.nidreg_odom_model_get.argtypes = [ctypes.c_void_p, c_int32_p, c_double_p, c_double_p]
    lib.nidreg_odom_set_source.argtypes = [ctypes.c_void_p, c_double_p, c_double_p, c_int32_p, ctypes.c_int32]
    lib.nidreg_odom_linearize.argtypes = [ctypes.c_void_p, c_double_p, ctypes.c_int32, ctypes.c_double, c_double_p]
    lib.nidreg_odom_error.argtypes = [ctypes.c_void_p, c_double_p, ctypes.c_int32, c_double_p]
    lib.nidreg_odom_correspondences.argtypes = [ctypes.c_void_p, c_int32_p, c_double_p, c_double_p]
    lib.nidreg_odom_deskew_insert.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_int32] * 9 + [ctypes.c_double] * 3 + [c_double_p] * 3 + [c_int64_p]
    c_uint8_p, c_uint32_p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)
    lib.nidreg_features_detect.argtypes = [ctypes.c_int, c_uint8_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64, c_uint8_p, ctypes.c_int64] + [ctypes.c_int] * 5 + [c_int32_p, c_uint32_p, c_int32_p]
    lib.nidreg_features_match.argtypes = [ctypes.c_int, c_uint32_p, ctypes.c_int, c_uint32_p, ctypes.c_int] + [ctypes.c_int] * 3 + [c_int32_p] * 3
    lib.nidreg_splat_create.argtypes = [ctypes.c_int, ctypes.c_int64, c_double_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p)]
    lib.nidreg_splat_set_colors.argtypes = [ctypes.c_void_p, c_uint8_p]
    lib.nidreg_splat_draw.argtypes = [ctypes.c_void_p, ctypes.c_int, c_double_p, c_double_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, c_double_p, ctypes.c_int, c_uint8_p, ctypes.c_int64,
                                      ctypes.c_int, c_uint8_p, c_int32_p]
    lib.nidreg_splat_destroy.restype = None
    lib.nidreg_splat_destroy.argtypes = [ctypes.c_void_p]
    lib.nidreg_jpeg_info.argtypes = [ctypes.c_char_p, ctypes.c_int64] + [c_int32_p] * 5
    lib.nidreg_jpeg_coefficients.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int16), ctypes.c_int64, ctypes.POINTER(ctypes.c_uint16)]
    lib.nidreg_jpeg_decode_gray.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int64, ctypes.c_int, c_uint8_p, ctypes.c_int64]
    lib.nidreg_jpeg_get_timing.argtypes = [c_double_p]
    # data as an address: the bytes may be a read-only view into a mapped bag file
    lib.nidreg_image_to_mono8.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_char_p, ctypes.c_int, c_uint8_p, ctypes.c_int64]
    lib.nidreg_image_get_timing.argtypes = [c_double_p]
    # packets as an address: a read-only view into a mapped bag file, at any alignment
    lib.nidreg_velodyne_decode.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, c_double_p, c_double_p, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                           c_float_p, c_int32_p]
    lib.nidreg_velodyne_get_timing.argtypes = [c_double_p]
    lib.nidreg_ouster_decode.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p,
                                         ctypes.c_double, c_double_p, ctypes.c_uint64, ctypes.c_void_p, c_int32_p]
    lib.nidreg_ouster_get_timing.argtypes = [c_double_p]
    lib.nidreg_draw.argtypes = [ctypes.c_int, c_uint8_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64, c_uint8_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, c_int32_p, c_uint8_p]
    lib.nidreg_mask_create.argtypes = [ctypes.c_int, c_uint8_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    lib.nidreg_mask_get.argtypes = [ctypes.c_void_p, c_uint8_p, ctypes.c_int64]
    lib.nidreg_mask_destroy.restype = None
    lib.nidreg_mask_destroy.argtypes = [ctypes.c_void_p]
    lib.nidreg_cloud_select.argtypes = [ctypes.c_void_p, ctypes.c_int, c_double_p, c_double_p, ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_double,
                                        ctypes.c_double, ctypes.POINTER(ctypes.c_void_p), c_int32_p, c_int64_p]
    lib.nidreg_cloud_size.argtypes = [ctypes.c_void_p, c_int64_p]
    lib.nidreg_cloud_get.argtypes = [ctypes.c_void_p, c_double_p, c_double_p]
    lib.nidreg_cloud_select_counts.argtypes = [ctypes.c_void_p, c_int64_p]
    lib.nidreg_cloud_fold_ids.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_double, ctypes.c_int, c_int32_p, c_int64_p]
    lib.nidreg_cloud_fold.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), c_int32_p, c_int64_p]
    # test hook (csrc/nidreg_abi.hip, not declared in include/nidreg.h): a plain handle's records as the builder left them
    lib.nidreg_debug_records.argtypes = [ctypes.c_void_p, c_int64_p, c_int64_p, ctypes.c_int64, c_double_p, c_int32_p, ctypes.c_int64]
    lib.nidreg_rccl_unique_id.argtypes = [ctypes.c_char_p]
    lib.nidreg_shard_comm_init.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]
    lib.nidreg_shard_attach_rccl.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    _lib = lib
    return lib


def kernel_source_hash():
    """sha256 (16 hex digits) over the sources of the evaluation kernels (device code, launch wrappers, build flags --
    not the host side of the ABI): stamps PMC summaries so that bench.py never reports counter traffic measured on a
    different kernel build."""
    import hashlib

    h = hashlib.sha256()
    names = ["nid_device.hpp", "nid_atan_table.hpp", "nid_log_table.hpp", "nid_multi.hpp", "nid_kernels.hpp", "nid_fused.hpp", "nid_launch_impl.hpp", "nid_kernels_f64.hip", "nid_kernels_f64_exact.hip", "nid_kernels_fused.hip", "nid_select_kernels.hpp", "nidreg_select.hip", "nid_fold_kernels.hpp", "nidreg_fold.hip", "Makefile"]
    for path in [os.path.join(CSRC_DIR, n) for n in names]:
        h.update(os.path.basename(path).encode())
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def library_kernel_build():
    """The kernel-source hash libnidreg.so was BUILT from (nidreg_kernel_build): equals kernel_source_hash() unless the library is
    stale against the sources next to it."""
    lib = load()
    lib.nidreg_kernel_build.restype = ctypes.c_char_p
    return lib.nidreg_kernel_build().decode()


def stamp_or_refuse():
    """For the measurement tools: the hash to stamp a summary with -- refuses (SystemExit) when the loaded library was not built from the
    sources on disk, because the summary would then be attributed to kernels that did not produce it."""
    built, tree = library_kernel_build(), kernel_source_hash()
    if built != tree:
        raise SystemExit(f"refusing to stamp: libnidreg.so was built from kernel sources {built}, the tree holds {tree} (rebuild, then measure again)")
    return built


def debug_records(handle):
    """``nidreg_debug_records`` (a test hook): what the device record builder left in a plain handle, copied to the host --
    ``dict(num_records, NG, GW, gcount int64[NG + 1], xyz float64 (n, 3), bin int32 (n,))``, records in stored order, float32
    records widened (exact).  ``handle``: a ``nid`` cost object or a raw ``nidreg_handle``."""
    import numpy as np

    lib = load()
    h = getattr(handle, "h", handle)
    c3 = (ctypes.c_int64 * 3)()
    check(lib.nidreg_debug_records(h, c3, None, 0, None, None, 0), "nidreg_debug_records")
    n, NG, GW = int(c3[0]), int(c3[1]), int(c3[2])
    gcount = np.zeros(NG + 1, dtype=np.int64)
    xyz = np.zeros((n, 3), dtype=np.float64)
    bins = np.zeros(n, dtype=np.int32)
    check(lib.nidreg_debug_records(h, c3, gcount.ctypes.data_as(c_int64_p), NG + 1, xyz.ctypes.data_as(c_double_p), bins.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n), "nidreg_debug_records")
    return dict(num_records=n, NG=NG, GW=GW, gcount=gcount, xyz=xyz, bin=bins)


def last_error():
    return load().nidreg_last_error().decode()


def check(rc, what):
    if rc < 0:
        raise RuntimeError(f"{what} failed ({rc}): {last_error()}")
    return rc
