"""The building blocks of preprocessing that had no counterpart here yet: the voxel integrator, ``cv::equalizeHist`` and the
LiDAR field of view.

==================================================  =========================================================
here                                                reference
==================================================  =========================================================
``StaticPointCloudIntegrator(res, min_distance)``   ``vlcal::StaticPointCloudIntegrator`` (static_point_cloud_integrator.cpp:8-62)
``equalize_hist(image_u8)``                         ``cv::equalizeHist`` (OpenCV, not in the reference tree; preprocess_map.cpp:75)
``StaticPointCloudIntegrator.insert_cloud2(msg, ch)``  ``extract_raw_points`` (ros_cloud_converter.hpp:62-175) + the finite filter
                                                    (preprocess.cpp:457) + ``insert_points``, on the message's raw bytes
``estimate_lidar_fov(points)``                      ``vlcal::estimate_lidar_fov`` (src/vlcal/common/estimate_fov.cpp:53-91)
``TimeKeeper().process(stamp, first, last, min)``   ``vlcal::TimeKeeper::process`` (src/vlcal/common/time_keeper.cpp:44-160)
``equalized_cloud`` / ``save_preprocessed``         what ``preprocess`` and ``preprocess_map`` share after the voxel filter
                                                    (preprocess.cpp:464-473 and :160-232; preprocess_map.cpp:158-215)
==================================================  =========================================================

The integrator is a hash table on the GPU behind ``include/nidreg.h`` (``nidreg_integrator_*``, csrc/nid_voxel_kernels.hpp); there
is no CPU implementation of it here.  ``equalize_hist`` is host work in the reference too (one pass over one image).
"""
import ctypes
import math
import sys

import numpy as np

from . import _lib


def _check(rc, what):
    """NIDREG_ERR_INVALID (a refused frame, a bad argument) is the caller's ValueError; anything else is a runtime failure."""
    if rc == _lib.NIDREG_ERR_INVALID:
        raise ValueError(f"{what}: {_lib.last_error()}")
    return _lib.check(rc, what)


def cloud2_layout(msg_or_fields, intensity_channel, who="insert_cloud2"):
    """What the PointCloud2 routes need of a message (``StaticPointCloudIntegrator.insert_cloud2`` says which forms it may have):
    ``(data uint8 array, number of points, point_step, {field name: (offset, datatype)})``, after the checks they share."""
    get = msg_or_fields.get if isinstance(msg_or_fields, dict) else lambda k, d=None: getattr(msg_or_fields, k, d)
    table = {}
    for f in get("fields"):
        name, offset, datatype = (f[0], f[1], f[2]) if isinstance(f, (tuple, list)) else (f.name, f.offset, f.datatype)
        table[name] = (int(offset), int(datatype))  # (a name listed twice keeps its last entry, as in the reference)
    if get("is_bigendian"):
        raise ValueError(f"{who}: big-endian point data is not read")
    for k in ("x", "y", "z"):
        if k not in table:
            raise ValueError(f"{who}: the cloud has no '{k}' field (fields: {', '.join(table)})")
    if intensity_channel not in table:
        raise ValueError(f"{who}: the cloud has no '{intensity_channel}' field to take intensities from (fields: {', '.join(table)})")
    if not (table["x"][1] == table["y"][1] == table["z"][1]):
        raise ValueError(f"{who}: x, y and z have different datatypes")
    n = get("num_points")
    n = int(get("width")) * int(get("height")) if n is None else int(n)
    step = int(get("point_step"))
    data = get("data")
    data = data if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
    if data.dtype != np.uint8 or data.ndim != 1 or not data.flags.c_contiguous:
        raise ValueError(f"{who}: data must be a contiguous run of bytes")
    if n < 0 or step < 1 or data.size < n * step:
        raise ValueError(f"{who}: {data.size} data bytes for {n} points of {step} bytes")
    return data, n, step, table


class StaticPointCloudIntegrator:
    """``vlcal::StaticPointCloudIntegrator``: one entry per occupied voxel, the LAST point inserted into it (the reference
    overwrites, static_point_cloud_integrator.cpp:35).  Defaults as the reference's (:8-12).

    ``get_points`` / ``get_records`` return the voxels in ascending order of the winners' sequence numbers (``last_seq``; the
    reference's order is ``std::unordered_map`` iteration order).  One narrowing: a voxel index must lie in [-2^20, 2^20) on
    every axis; a frame with a point beyond that, or with a non-finite coordinate, raises ``ValueError`` and inserts nothing."""

    def __init__(self, voxel_resolution=0.05, min_distance=1.0, device=0):
        self._lib = _lib.load()
        self._h = None
        h = ctypes.c_void_p()
        _check(self._lib.nidreg_integrator_create(int(device), float(voxel_resolution), float(min_distance), ctypes.byref(h)), "nidreg_integrator_create")
        self._h = h
        self.voxel_resolution, self.min_distance, self.device = float(voxel_resolution), float(min_distance), int(device)
        self.last_seq = None

    def insert_points(self, points, intensities):
        """``insert_points``: ``points`` (n, 3) or (n, 4) (a fourth column is ignored: ``Frame::points`` is x y z 1),
        ``intensities`` (n,).  float32 arrays (rows and intensities of any 4-byte stride, e.g. both views of one buffer of PLY
        records) are uploaded as float32 and widened on the GPU; anything else goes through float64."""
        points = np.asarray(points)
        intensities = np.asarray(intensities)
        if points.ndim != 2 or points.shape[1] not in (3, 4) or intensities.shape != (points.shape[0],):
            raise ValueError("points must be (n, 3) or (n, 4) and intensities (n,)")
        n = points.shape[0]
        f32 = all(a.dtype == np.float32 and a.dtype.isnative for a in (points, intensities))
        if f32 and (n <= 1 or (points.strides[1] == 4 and points.strides[0] % 4 == 0 and intensities.strides[0] % 4 == 0)):
            pstride, istride = (points.strides[0], intensities.strides[0]) if n > 1 else (12, 4)
            rc = self._lib.nidreg_integrator_insert_f32(self._h, points.ctypes.data, pstride, intensities.ctypes.data, istride, n)
            return _check(rc, "nidreg_integrator_insert_f32")
        if f32:
            points, intensities = np.ascontiguousarray(points), np.ascontiguousarray(intensities)
            rc = self._lib.nidreg_integrator_insert_f32(self._h, points.ctypes.data, points.strides[0], intensities.ctypes.data, 4, n)
            return _check(rc, "nidreg_integrator_insert_f32")
        points = np.ascontiguousarray(points, dtype=np.float64)
        intensities = np.ascontiguousarray(intensities, dtype=np.float64)
        rc = self._lib.nidreg_integrator_insert(self._h, points.ctypes.data, 8 * points.shape[1], intensities.ctypes.data, n)
        return _check(rc, "nidreg_integrator_insert")

    def insert_cloud2(self, msg_or_fields, intensity_channel):
        """One ``sensor_msgs/PointCloud2`` frame from its raw bytes: ``extract_raw_points`` (ros_cloud_converter.hpp:62-175), the
        finite filter of preprocess.cpp:457 and ``insert_points``, with the records uploaded as they lie in the message and
        decoded on the GPU.  ``msg_or_fields``: a decoded message (``rosbag1.decode_pointcloud2``) or a dict with the same
        names -- ``fields`` (entries with name / offset / datatype, or such tuples), ``point_step``, ``data`` (bytes-like, at
        least width x height x point_step bytes), ``width`` and ``height`` (or ``num_points``), ``is_bigendian``.  Returns the
        number of points skipped for a non-finite coordinate; they still take a sequence number.  Missing x / y / z, a missing
        intensity channel, mixed or unsupported datatypes and big-endian data raise ``ValueError``."""
        data, n, step, table = cloud2_layout(msg_or_fields, intensity_channel)
        skipped = ctypes.c_int64()
        rc = self._lib.nidreg_integrator_insert_cloud2(self._h, data.ctypes.data if n else None, n, step, table["x"][0], table["y"][0], table["z"][0], table["x"][1],
                                                       table[intensity_channel][0], table[intensity_channel][1], ctypes.byref(skipped))
        _check(rc, "nidreg_integrator_insert_cloud2")
        return int(skipped.value)

    def insert_las(self, records, record_length, point_format, scale, offset, origin=(0.0, 0.0, 0.0), intensity="intensity", exclude_classes=(), keep_withheld=False):
        """Point records of an ASPRS LAS file as they lie in the file (``dataset.read_las_chunks``): ``records`` a contiguous uint8
        array of whole ``record_length``-byte records of ``point_format`` 0..10, uploaded as they are and decoded on the GPU --
        ``(int32 * scale + offset) - origin`` in fp64, so a georeferenced map is recentred before anything is narrowed to float32.
        ``intensity``: ``"intensity"`` (the 16-bit field) or ``"rgb"`` (77 R + 150 G + 29 B; formats with colour only).  Points
        whose class is in ``exclude_classes`` (0..255) and, unless ``keep_withheld``, withheld points are skipped like non-finite
        PointCloud2 points: they take a sequence number and are counted in the return value."""
        records = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1)
        step = int(record_length)
        if step < 1 or records.size % step:
            raise ValueError(f"insert_las: {records.size} bytes are not whole records of {step} bytes")
        if intensity not in ("intensity", "rgb"):
            raise ValueError(f"insert_las: intensity must be 'intensity' or 'rgb', got {intensity!r}")
        mask = (ctypes.c_uint64 * 4)()
        for c in exclude_classes:
            if not 0 <= int(c) <= 255:
                raise ValueError(f"insert_las: class {c} is outside 0..255")
            mask[int(c) >> 6] |= 1 << (int(c) & 63)
        n = records.size // step
        triples = [(ctypes.c_double * 3)(*[float(v) for v in t]) for t in (scale, offset, origin)]
        skipped = ctypes.c_int64()
        rc = self._lib.nidreg_integrator_insert_las(self._h, records.ctypes.data if n else None, n, step, int(point_format), triples[0], triples[1], triples[2],
                                                    1 if intensity == "rgb" else 0, mask, 1 if keep_withheld else 0, ctypes.byref(skipped))
        _check(rc, "nidreg_integrator_insert_las")
        return int(skipped.value)

    def size(self):
        m = ctypes.c_int64()
        _check(self._lib.nidreg_integrator_size(self._h, ctypes.byref(m)), "nidreg_integrator_size")
        return int(m.value)

    def info(self):
        """``{"voxels", "capacity" (slots of the table), "offered" (points offered so far), "slot_bytes"}``"""
        v = (ctypes.c_int64 * 4)()
        _check(self._lib.nidreg_integrator_info(self._h, v), "nidreg_integrator_info")
        return {"voxels": int(v[0]), "capacity": int(v[1]), "offered": int(v[2]), "slot_bytes": int(v[3])}

    def get_records(self):
        """The (m, 4) float32 array as stored: x y z intensity per voxel (the PLY record); sets ``last_seq`` (m,) int64."""
        m = self.size()
        rec = np.empty((m, 4), dtype=np.float32)
        seq = np.empty(m, dtype=np.int64)
        rc = self._lib.nidreg_integrator_get(self._h, rec.ctypes.data_as(_lib.c_float_p), seq.ctypes.data_as(_lib.c_int64_p))
        _check(rc, "nidreg_integrator_get")
        self.last_seq = seq
        return rec

    def get_points(self):
        """``get_points`` (:49-62): ``(points float32 (m, 3), intensities float32 (m,))``"""
        rec = self.get_records()
        return np.ascontiguousarray(rec[:, :3]), np.ascontiguousarray(rec[:, 3])

    def close(self):
        if getattr(self, "_h", None):
            self._lib.nidreg_integrator_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def equalize_hist(image_u8):
    """``cv::equalizeHist`` of an 8-bit single-channel image: lookup table from the cumulative histogram, the first non-zero
    bin as the offset, ``round(scale * (cdf - cdf_min))`` with scale = 255 / (pixels - cdf_min); a constant image is returned
    unchanged.  The same bytes as ``synth.equalize_hist_u8`` on every input."""
    img = np.asarray(image_u8)
    if img.dtype != np.uint8:
        raise ValueError("equalize_hist: an 8-bit image expected")
    if img.size == 0:
        return img.copy()
    hist = np.bincount(img.reshape(-1), minlength=256).astype(np.float64)
    i0 = int(np.flatnonzero(hist)[0])
    total = float(hist.sum())
    if total == float(hist[i0]):
        return np.full_like(img, i0)
    scale = 255.0 / (total - float(hist[i0]))
    csum = np.cumsum(hist) - hist[: i0 + 1].sum()
    lut = np.clip(np.rint(csum * scale), 0, 255)
    lut[: i0 + 1] = 0
    return lut.astype(np.uint8)[img]


def estimate_lidar_fov(points, device=0):
    """``vlcal::estimate_lidar_fov`` (estimate_fov.cpp:53-91) [rad]: downsample at 0.2 m, round the representatives to float32,
    drop those closer than 1 m (float norm, :66), take the convex hull (``scipy.spatial.ConvexHull``: qhull, as in PCL) and
    return ``acos`` of the smallest dot product between the normalised directions of two hull vertices (:80-90, including the
    reference's ``min_cosine = M_PI`` initial value).

    Two differences from the reference: the representative of a 0.2 m voxel is the last point that fell into it (the voxel
    integrator above with ``min_distance`` 0), not the centroid ``pcl::VoxelGrid`` computes (PCL is not in the reference tree:
    its arithmetic is not pinned); and fewer than 4 non-coplanar points raise ``ValueError`` (PCL's hull of such input is
    whatever qhull's error path leaves)."""
    from scipy.spatial import ConvexHull, QhullError

    pts = np.asarray(points)
    if pts.ndim != 2 or pts.shape[1] not in (3, 4):
        raise ValueError("estimate_lidar_fov: points (n, 3) or (n, 4) expected")
    if pts.dtype != np.float32:
        pts = np.ascontiguousarray(pts, dtype=np.float64)
    integ = StaticPointCloudIntegrator(voxel_resolution=0.2, min_distance=0.0, device=device)
    try:
        integ.insert_points(pts, np.zeros(pts.shape[0], dtype=pts.dtype))
        reps, _ = integ.get_points()
    finally:
        integ.close()
    x, y, z = reps[:, 0], reps[:, 1], reps[:, 2]
    reps = reps[~(np.sqrt(x * x + y * y + z * z) < np.float32(1.0))]
    if reps.shape[0] < 4:
        raise ValueError(f"estimate_lidar_fov: {reps.shape[0]} points further than 1 m after the 0.2 m downsampling; a convex hull needs 4 that are not coplanar")
    try:
        hull = ConvexHull(reps.astype(np.float64))
    except QhullError as e:
        raise ValueError(f"estimate_lidar_fov: no convex hull (coplanar points?): {str(e).splitlines()[0]}") from None
    dirs = reps[hull.vertices].astype(np.float64)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    min_cosine = math.pi
    for s in range(0, dirs.shape[0], 1024):  # all pairs, 1024 rows at a time
        min_cosine = min(min_cosine, float((dirs[s : s + 1024] @ dirs.T).min()))
    # (a pair (i, i) has cosine 1 up to rounding and never is the minimum of a hull of four or more vertices)
    return math.acos(max(-1.0, min_cosine))


def lidar_camera(lidar_fov):
    """preprocess_map.cpp:184-200: the virtual camera the LiDAR image is rendered through, from the LiDAR's field of view [rad].
    Returns ``(camera_model, intrinsics, (width, height), T_lidar_camera 4x4)``: below 150 degrees a 1024 x 1024 pinhole whose
    optical axis is the LiDAR's x (AngleAxis(pi/2, Y) AngleAxis(-pi/2, Z), :193) with fx = 1024 / (2 tan(fov / 2)); else a
    1920 x 960 equirectangular camera (AngleAxis(-pi/2, X), :199).  The rotations are the closed forms (entries 0 and +-1), where
    Eigen's carry cos(pi/2) = 6e-17."""
    T = np.eye(4)
    if lidar_fov < 150.0 * math.pi / 180.0:
        size = (1024, 1024)
        ry = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
        rz = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
        T[:3, :3] = ry @ rz
        fx = size[0] / (2.0 * math.tan(lidar_fov / 2.0))
        return "plumb_bob", [fx, fx, size[0] / 2.0, size[1] / 2.0], size, T
    size = (1920, 960)
    T[:3, :3] = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])
    return "equirectangular", [float(size[0]), float(size[1])], size, T


class TimeKeeper:
    """``vlcal::TimeKeeper::process`` (time_keeper.cpp:44-160) with the default ``AbsPointTimeParams`` (time_keeper.hpp:13-16:
    both true), reduced to what decides whether a frame is kept: the frame's stamp after ``replace_points_stamp``, which reads
    only the first, the last and the smallest per-point time.  The per-point times themselves are used by the dynamic
    integrator alone: ``process_times`` returns them as an affine map of the raw column, which the GPU applies to the raw field.
    Warnings go to ``log`` once, as the reference's ``first_warning``."""

    def __init__(self, log=None):
        self.log = log if log is not None else (lambda msg: print(msg, file=sys.stderr))
        self.first_warning = True
        self.last_points_stamp = -1.0
        self.point_time_offset = 0.0
        self.stamp = None  # the stamp of the last processed frame after replacement
        self.num_scans = 0  # estimate_scan_duration (:162-180), used by process_times alone
        self.first_points_stamp = 0.0
        self.estimated_scan_duration = -1.0

    def process(self, stamp, first=None, last=None, min_time=None):
        """``stamp`` [s]; ``first`` / ``last`` / ``min_time``: per-point times of the first and last point and their minimum
        (callable or value; read only on the negative-time path), ``first=None`` when the cloud has no time field.  Returns
        ``False`` when the frame must be skipped (its stamp rewinds)."""
        stamp = self._replace_points_stamp(float(stamp), first, last, min_time)
        self.stamp = stamp
        diff = stamp - self.last_points_stamp
        if self.last_points_stamp < 0.0:
            pass  # first LiDAR frame
        elif diff < 0.0:
            self.log("warning: point timestamp rewind detected!!")
            self.log(f"       : current:{stamp:.6f} last:{self.last_points_stamp:.6f} diff:{diff:.6f}")
            return False
        elif diff > 0.5:
            self.log("warning: large time gap between consecutive LiDAR frames!!")
            self.log(f"       : current:{stamp:.6f} last:{self.last_points_stamp:.6f} diff:{diff:.6f}")
        self.last_points_stamp = stamp
        return True

    def process_times(self, stamp, first=None, last=None, min_time=None, raw_scale=1.0):
        """``process`` and, with it, the per-point times ``replace_points_stamp`` leaves (:64-160) as an affine map of the raw
        time column: returns ``(keep, scale, shift)`` with ``time[i] = raw[i] * scale + shift`` [s].  ``first`` / ``last`` /
        ``min_time`` are ``raw * raw_scale`` (``raw_scale`` = 1e-9 for the nanoseconds of a uint32 field).  Without a time field
        (``first=None``) the times are the pseudo times ``scale * i / n`` with ``scale`` the estimated scan duration -- 0 for the
        first frame, whose times are all zero."""
        if first is None:
            duration = self._estimate_scan_duration(float(stamp))
            return self.process(stamp), (duration if duration > 0.0 else 0.0), 0.0
        cache = []

        def min_once():
            if not cache:
                cache.append(float(min_time() if callable(min_time) else min_time))
            return cache[0]

        scale, shift = float(raw_scale), 0.0
        f, l = float(first), float(last)
        if f < 0.0 or l < 0.0:  # :92-103
            shift -= min_once()
            f -= min_once()
        if f >= 1.0:  # :106-157: absolute times
            if f > 1e16:  # :118-128
                scale, shift, f = scale * 1e-9, shift * 1e-9, f * 1e-9
            shift -= f  # :153-156
        return self.process(stamp, first, last, min_once), scale, shift

    def _estimate_scan_duration(self, stamp):
        if self.estimated_scan_duration > 0.0:
            return self.estimated_scan_duration
        self.num_scans += 1
        if self.num_scans == 1:
            self.first_points_stamp = stamp
            return -1.0
        duration = (stamp - self.first_points_stamp) / (self.num_scans - 1)
        if self.num_scans == 1000:
            self.log(f"estimated scan duration:{duration}")
            self.estimated_scan_duration = duration
        return duration

    def _replace_points_stamp(self, stamp, first, last, min_time):
        if first is None:  # :67-83: pseudo per-point times; the stamp stays
            if self.first_warning:
                self.log("warning: per-point timestamps are not given!!")
                self.log("       : use pseudo per-point timestamps based on the order of points")
                self.first_warning = False
            return stamp
        first, last = float(first), float(last)
        if first < 0.0 or last < 0.0:  # :92-103
            self.log(f"warning: negative per-point timestamp ({first:.6f} or {last:.6f}) found!!")
            m = float(min_time() if callable(min_time) else min_time)
            self.log(f"       : min_stamp={m:.6f}")
            first, last, stamp = first - m, last - m, stamp - m
        if first < 1.0:  # :106-108: already relative to the first point
            return stamp
        if self.first_warning:
            self.log(f"warning: large point timestamp ({last:.6f} > 1.0) found!!")
            self.log("       : assume that point times are absolute and convert them to relative")
            self.log("       : replace_frame_stamp=1 wrt_first_frame_timestamp=1")
        if first > 1e16:  # :118-128: nanoseconds
            if self.first_warning:
                self.log(f"warning: too large point timestamp ({first:.6f} > 1e16) found!!")
                self.log("       : maybe using a Livox LiDAR that use FLOAT64 nanosec per-point timestamps")
                self.log("       : convert per-point timestamps from nanosec to sec")
            first, last = first * 1e-9, last * 1e-9
        if abs(stamp - first) < 1.0:  # :132-139
            if self.first_warning:
                self.log("warning: use first point timestamp as frame timestamp")
                self.log(f"       : frame={stamp:.6f} point={first:.6f}")
            self.point_time_offset = 0.0
            stamp = first
        else:  # :140-151 (the offset is taken inside the first-warning block only, as in the reference)
            if self.first_warning:
                self.log("warning: point timestamp is too apart from frame timestamp!!")
                self.log("       : use time offset w.r.t. the first frame timestamp")
                self.log(f"       : frame={stamp:.6f} point={first:.6f} diff={stamp - first:.6f}")
                self.point_time_offset = stamp - first
            stamp = first + self.point_time_offset
        self.first_warning = False
        return stamp


def equalized_cloud(records, device=0):
    """The integrator's records -> ``(points (m, 4) float64 homogeneous, intensities (m,) float64)`` with the intensities
    rank-equalised into 256 levels (preprocess.cpp:464-473, preprocess_map.cpp:158-168); the points are float32 values."""
    from . import render

    points = np.ones((records.shape[0], 4), dtype=np.float64)
    points[:, :3] = records[:, :3]
    intensities = render.equalize_intensities(records[:, 3].astype(np.float64), device=device)
    return points, intensities


def save_preprocessed(dst_path, camera, bags, meta, device=0, log=print):
    """preprocess.cpp:160-232 / preprocess_map.cpp:173-215: the LiDAR's field of view from the FIRST bag's points, the virtual
    camera it selects, both LiDAR images of every bag through that camera, and the directory (``dataset.write_preprocessed``).
    ``bags`` = [(bag_name, image_u8, points (m, 4), intensities (m,))].  Returns ``(config, lidar_fov)``."""
    from . import dataset, nid, render

    lidar_fov = estimate_lidar_fov(bags[0][2], device=device)
    log(f"LiDAR FoV: {lidar_fov * 180.0 / math.pi:g}[deg]")
    model, lidar_intrinsics, size, T_lidar_camera = lidar_camera(lidar_fov)
    lidar_proj = nid.create_camera(model, lidar_intrinsics, [])
    T_camera_lidar = np.linalg.inv(T_lidar_camera)
    lidar_images = {name: render.generate_lidar_image(lidar_proj, size, T_camera_lidar, points, intensities, device=device) for name, _, points, intensities in bags}
    config = dataset.write_preprocessed(dst_path, camera, bags, meta=meta, lidar_images=lidar_images)
    return config, lidar_fov
