"""The three LiDAR message types that are recorded INSTEAD of ``sensor_msgs/PointCloud2``, read without the vendor drivers: every one
becomes a ``rosbag1.PointCloud2`` tuple, which is all the bag pipeline (``preprocess_ros1.run``) knows.

==========================================================  =====================================================================
``velodyne_msgs/VelodyneScan`` (``.../msg/VelodyneScan``)    the raw UDP packets of a VLP-16 / HDL-32E; decoded on the GPU
                                                             (``nidreg_velodyne_decode``, include/nidreg.h states the rules) into
                                                             x, y, z, intensity, time records of 20 bytes -- the cloud
                                                             ``velodyne_pointcloud`` publishes, no-return records as NaN
``livox_ros_driver(2)/CustomMsg`` (``.../msg/CustomMsg``)    a view of the message's own 19-byte (CDR: 20-byte) point records under
                                                             the fields t (uint32 ns), x, y, z, reflectivity, tag, line: no kernel
``ouster_ros/PacketMsg`` (``ouster_msgs/msg/PacketMsg``,     one UDP packet of an Ouster sensor a message -- a 64th or 128th of a turn --,
``ouster_sensor_msgs/msg/PacketMsg``)                        batched into scans by ``frame_id`` (``batch_points``) and decoded on the GPU
                                                             (``nidreg_ouster_decode``) into 32-byte records x, y, z, intensity, t,
                                                             reflectivity, ring, ambient, range in PACKET order (the driver's cloud is
                                                             the destaggered H x W image); the geometry comes from the sensor's
                                                             metadata JSON (``--ouster_metadata``, ``--ouster_frame``)
==========================================================  =====================================================================

Both layouts, the packet rules and the two laser tables below are restated from the message definitions, the VLP-16 / HDL-32E manuals
and ``velodyne_pointcloud``'s ``rawdata.cc`` from memory: they are UNPINNED against ``velodyne_pointcloud``, ``livox_ros_driver`` and real
recordings.  Out of scope, refused by name where they can be told: dual-return packets, VLP-32C, VLS-128, HDL-64E (the two-point
calibration) and Hesai packets.  The Livox ``tag`` (noise / return number), ``line``, ``lidar_id`` and ``timebase`` are carried or
dropped, never interpreted.

The Ouster packet layouts (LEGACY, RNG19_RFL8_SIG16_NIR16, RNG15_RFL8_NIR8), the metadata keys and the beam geometry are restated from
the sensor's software manual and the SDK's field tables from memory as well: UNPINNED against ``ouster_ros``, the Ouster SDK and real
recordings.  Refused by name: the dual-return and FUSA profiles.  Not read: the IMU packets (same message type; a buffer of another
length than the profile's packet is refused), the packet header's and footer's other fields, ``pixel_shift_by_row``.
"""
import ctypes
import json
import math
from collections import namedtuple

import numpy as np

from . import rosbag1
from .rosbag1 import FLOAT32, UINT8, UINT32, PointCloud2, PointField

PACKET_BYTES = 1206  # 12 blocks of 100 bytes, the device's timestamp (4), the return mode, the product id
PACKET_DATA_OFFSET = 8  # of the data inside a VelodynePacket: behind its stamp
POINTS_PER_PACKET = 384
RETURN_MODE_BYTE, PRODUCT_ID_BYTE = 1204, 1205
DUAL_RETURN = 0x39
MAX_PACKETS = 65536  # nidreg_velodyne_decode's limit

# data: uint8 view from the first packet ELEMENT on (a packet's 1206 bytes start PACKET_DATA_OFFSET into its element, elements lie
# ``stride`` bytes apart); stamps: [(sec, nsec)] per packet
VelodyneScan = namedtuple("VelodyneScan", "stamp frame_id num_packets stride data stamps")

VELODYNE_FIELDS = [PointField("x", 0, FLOAT32, 1), PointField("y", 4, FLOAT32, 1), PointField("z", 8, FLOAT32, 1), PointField("intensity", 12, FLOAT32, 1),
                   PointField("time", 16, FLOAT32, 1)]
LIVOX_FIELDS = [PointField("t", 0, UINT32, 1), PointField("x", 4, FLOAT32, 1), PointField("y", 8, FLOAT32, 1), PointField("z", 12, FLOAT32, 1),
                PointField("reflectivity", 16, UINT8, 1), PointField("tag", 17, UINT8, 1), PointField("line", 18, UINT8, 1)]


def points_kind(type_name):
    """``"PointCloud2"``, ``"VelodyneScan"``, ``"CustomMsg"`` or ``"PacketMsg"`` for a connection type this module turns into a cloud, else
    ``None``"""
    if type_name.endswith("/PointCloud2") or type_name == "PointCloud2":
        return "PointCloud2"
    for kind in ("VelodyneScan", "CustomMsg", "PacketMsg"):
        if type_name.endswith("/" + kind) or type_name == kind:
            return kind
    return None


# ---------------------------------------------------------------------------------------------- message layouts
def _reader(data, what, cdr):
    from . import rosbag2

    return rosbag2._Cdr(data, what) if cdr else rosbag1._Reader(data, what)


def parse_velodyne_scan(data, cdr=False):
    """``Header header, VelodynePacket[] packets``; a packet is ``time stamp, uint8[1206] data`` -- a fixed array, no length prefix --, so
    the elements lie 1214 bytes apart in a ROS1 message and, the next stamp being aligned to 4, 1216 bytes apart in CDR (the last
    element may end without its padding).  Zero-copy."""
    what = "velodyne_msgs/msg/VelodyneScan" if cdr else "velodyne_msgs/VelodyneScan"
    r = _reader(data, what, cdr)
    stamp, frame_id = r.header()
    n = r.u32()
    stride = 1216 if cdr else 1214
    if n == 0:
        return VelodyneScan(stamp, frame_id, 0, stride, np.zeros(0, dtype=np.uint8), [])
    area = r.take((n - 1) * stride + PACKET_DATA_OFFSET + PACKET_BYTES, 4) if cdr else r.take((n - 1) * stride + PACKET_DATA_OFFSET + PACKET_BYTES)
    view = np.frombuffer(area, dtype=np.uint8)
    head = np.lib.stride_tricks.as_strided(view, shape=(n, 8), strides=(stride, 1))
    secs_nsecs = np.ascontiguousarray(head).view("<i4" if cdr else "<u4").reshape(n, 2)
    stamps = [(int(s), int(ns) & 0xFFFFFFFF) for s, ns in secs_nsecs]
    return VelodyneScan(stamp, frame_id, n, stride, view, stamps)


def parse_livox_custom(data, cdr=False):
    """``Header header, uint64 timebase, uint32 point_num, uint8 lidar_id, uint8[3] rsvd, CustomPoint[] points``; a point is ``uint32
    offset_time`` [ns], ``float32 x, y, z``, ``uint8 reflectivity, tag, line``: 19 bytes, 19 apart in a ROS1 message, 20 apart in CDR
    (``timebase`` aligned to 8, every element to 4).  The result is the synthesised cloud; its ``data`` is a zero-copy view of the
    message, except for a CDR message that ends without the last element's padding byte, which is copied into a padded buffer."""
    what = "livox_ros_driver2/msg/CustomMsg" if cdr else "livox_ros_driver/CustomMsg"
    r = _reader(data, what, cdr)
    stamp, frame_id = r.header()
    if cdr:
        r.take(8, 8)  # timebase
        r.take(8, 4)  # point_num, lidar_id, rsvd
        n = r.u32()
        step = 20
        left = len(r.buf) - (r.pos + (4 - r.pos) % 4)
        if n == 0:
            payload = np.zeros(0, dtype=np.uint8)
        elif left == n * step - 1:
            payload = np.zeros(n * step, dtype=np.uint8)
            payload[: n * step - 1] = np.frombuffer(r.take(n * step - 1, 4), dtype=np.uint8)
        else:
            payload = np.frombuffer(r.take(n * step, 4), dtype=np.uint8)
    else:
        r.take(8 + 4 + 1 + 3)
        n = r.u32()
        step = 19
        payload = np.frombuffer(r.take(n * step), dtype=np.uint8)
    return PointCloud2(stamp, frame_id, 1, n, list(LIVOX_FIELDS), 0, step, step * n, payload, 1)


# ---------------------------------------------------------------------------------------------- Velodyne models
# mechanical elevation [deg] and vertical offset [m] per laser, in firing order; rot_corr, horiz_offset and dist_corr are 0
VLP16_VERT_OFFSETS = (0.0112, -0.0007, 0.0097, -0.0022, 0.0081, -0.0037, 0.0066, -0.0051, 0.0051, -0.0066, 0.0037, -0.0081, 0.0022, -0.0097, 0.0007, -0.0112)
PRODUCT_IDS = {0x22: "vlp16", 0x21: "hdl32e"}
LIDAR_MODELS = ("vlp16", "hdl32e")
PERIODS = {16: (55.296e-6, 2.304e-6), 32: (46.080e-6, 1.152e-6)}  # num_lasers -> (firing period, laser period) [s]: the packet layout's
HDL64E_KEYS = ("dist_correction_x", "dist_correction_y", "focal_distance", "focal_slope")

# table: (num_lasers, 8) float64 rows cos_vert, sin_vert, cos_rot_corr, sin_rot_corr, vert_offset, horiz_offset, dist_corr, 0
VelodyneModel = namedtuple("VelodyneModel", "name table distance_resolution firing_period laser_period")


def laser_table(vert_rad, rot_rad, vert_offset, horiz_offset, dist_corr):
    t = np.zeros((len(vert_rad), 8), dtype=np.float64)
    for i in range(len(vert_rad)):
        t[i, :7] = (math.cos(vert_rad[i]), math.sin(vert_rad[i]), math.cos(rot_rad[i]), math.sin(rot_rad[i]), vert_offset[i], horiz_offset[i], dist_corr[i])
    return t


def builtin_model(name):
    if name == "vlp16":
        deg = [float(i) if i % 2 else -15.0 + i for i in range(16)]
        offsets = list(VLP16_VERT_OFFSETS)
    elif name == "hdl32e":
        deg = [-28.0 / 3.0 + (4.0 / 3.0) * ((i - 1) // 2) if i % 2 else -92.0 / 3.0 + (4.0 / 3.0) * (i // 2) for i in range(32)]
        offsets = [0.0] * 32
    else:
        raise ValueError(f"error: --lidar_model {name}: auto, vlp16 and hdl32e are the options")
    n = len(deg)
    zero = [0.0] * n
    return VelodyneModel(name, laser_table([math.radians(d) for d in deg], zero, offsets, zero, zero), 0.002, *PERIODS[n])


def model_from_product_id(product_id):
    """``--lidar_model auto``: byte 1205 of the first packet"""
    if product_id not in PRODUCT_IDS:
        raise ValueError(f"error: the packets' product id is 0x{product_id:02X}, which is neither 0x22 (VLP-16) nor 0x21 (HDL-32E): name the packet layout with "
                         "--lidar_model vlp16 or --lidar_model hdl32e (and the sensor's angles with --velodyne_calibration where they differ)")
    return builtin_model(PRODUCT_IDS[product_id])


def load_calibration(path):
    """The driver's calibration YAML (``velodyne_pointcloud/params/*.yaml``): ``num_lasers`` 16 or 32, ``distance_resolution`` and per laser
    ``laser_id``, ``vert_correction`` / ``rot_correction`` [rad], ``vert_offset_correction``, ``horiz_offset_correction``, ``dist_correction``
    [m].  The packet layout and the firing periods follow ``num_lasers``."""
    import yaml

    with open(path) as f:
        doc = yaml.safe_load(f)
    if not isinstance(doc, dict) or not isinstance(doc.get("lasers"), list):
        raise ValueError(f"error: {path}: not a velodyne calibration file (no 'lasers' list)")
    n = doc.get("num_lasers", len(doc["lasers"]))
    if n not in PERIODS or len(doc["lasers"]) != n:
        raise ValueError(f"error: {path}: num_lasers {n} with {len(doc['lasers'])} laser entries: calibrations of 16 (VLP-16 layout) and 32 lasers (HDL-32E layout) are read")
    rows = {}
    for entry in doc["lasers"]:
        if not isinstance(entry, dict) or "laser_id" not in entry or "vert_correction" not in entry:
            raise ValueError(f"error: {path}: a laser entry without laser_id or vert_correction")
        for key in HDL64E_KEYS:
            if float(entry.get(key, 0.0) or 0.0) != 0.0:
                raise ValueError(f"error: {path}: laser {entry['laser_id']} has a non-zero {key}: the HDL-64E two-point calibration is not applied here")
        rows[int(entry["laser_id"])] = [float(entry.get(k, 0.0) or 0.0) for k in ("vert_correction", "rot_correction", "vert_offset_correction", "horiz_offset_correction", "dist_correction")]
    if sorted(rows) != list(range(n)):
        raise ValueError(f"error: {path}: the laser_id values are not 0..{n - 1}, each once")
    cols = list(zip(*(rows[i] for i in range(n))))
    table = laser_table(*cols)
    resolution = float(doc.get("distance_resolution", 0.002))
    if not np.isfinite(table).all() or not math.isfinite(resolution):
        raise ValueError(f"error: {path}: a value that is not finite")
    return VelodyneModel(f"calibration {path}", table, resolution, *PERIODS[n])


class LidarOptions:
    """``--lidar_model`` and ``--velodyne_calibration`` of one run: the calibration file is read once, here; with ``auto`` the model is
    fixed by the first packet decoded.  ``ouster``: the ``OusterInfo`` of ``--ouster_metadata`` / ``--ouster_frame`` for a PacketMsg topic."""

    def __init__(self, lidar_model="auto", velodyne_calibration=None, ouster=None):
        self.ouster = ouster  # the ``OusterInfo`` of a PacketMsg topic (``--ouster_metadata``, ``--ouster_frame``), else ``None``
        if lidar_model != "auto" and lidar_model not in LIDAR_MODELS:
            raise ValueError(f"error: --lidar_model {lidar_model}: auto, vlp16 and hdl32e are the options")
        self.model = None
        if velodyne_calibration:
            self.model = load_calibration(velodyne_calibration)
            if lidar_model != "auto" and self.model.table.shape[0] != builtin_model(lidar_model).table.shape[0]:
                raise ValueError(f"error: --lidar_model {lidar_model} and the {self.model.table.shape[0]} lasers of {velodyne_calibration} name different packet layouts")
        elif lidar_model != "auto":
            self.model = builtin_model(lidar_model)

    def model_for(self, product_id):
        if self.model is None:
            self.model = model_from_product_id(product_id)
        return self.model


# ---------------------------------------------------------------------------------------------- Ouster: message, metadata, batching
OUSTER_PROFILES = {"LEGACY": 0, "RNG19_RFL8_SIG16_NIR16": 1, "RNG15_RFL8_NIR8": 2}  # NIDREG_OUSTER_* of include/nidreg.h
OUSTER_MAX_PACKETS = 4096  # nidreg_ouster_decode's limit
OUSTER_RECORD_BYTES = 32
OUSTER_FRAMES = ("sensor", "lidar")
OUSTER_GROUPS = ("beam_intrinsics", "lidar_data_format", "data_format", "lidar_intrinsics", "config_params")
UINT16 = 4  # sensor_msgs/PointField
OUSTER_FIELDS = [PointField("x", 0, FLOAT32, 1), PointField("y", 4, FLOAT32, 1), PointField("z", 8, FLOAT32, 1), PointField("intensity", 12, FLOAT32, 1),
                 PointField("t", 16, UINT32, 1), PointField("reflectivity", 20, UINT16, 1), PointField("ring", 22, UINT16, 1), PointField("ambient", 24, UINT16, 1),
                 PointField("range", 28, UINT32, 1)]

# profile: the index of OUSTER_PROFILES; column_table (W, 2), beam_table (H, 4), transform12 (12,): nidreg_ouster_decode's arguments
OusterInfo = namedtuple("OusterInfo", "profile_name profile H W C packet_size column_table beam_table n_mm transform12 frame")
# packets: the scan's packets in ONE contiguous uint8 array, ``packet_size`` apart; ts0: the smallest timestamp [ns] of a valid column
OusterBatch = namedtuple("OusterBatch", "packets num_packets ts0")


def ouster_packet_size(profile_name, H, C):
    """LEGACY ``C (20 + 12 H)``; RNG19_RFL8_SIG16_NIR16 ``64 + C (12 + 12 H)``; RNG15_RFL8_NIR8 ``64 + C (12 + 4 H)``"""
    if profile_name == "LEGACY":
        return C * (20 + 12 * H)
    return 64 + C * (12 + (12 if profile_name == "RNG19_RFL8_SIG16_NIR16" else 4) * H)


def parse_packet_msg(data, cdr=False):
    """``uint8[] buf``: a uint32 length and the bytes (CDR: behind the encapsulation header).  A zero-copy uint8 view of the packet."""
    r = _reader(data, "ouster_msgs/msg/PacketMsg" if cdr else "ouster_ros/PacketMsg", cdr)
    n = r.u32()
    return np.frombuffer(r.take(n), dtype=np.uint8)


def ouster_info(text, frame="sensor", where="the Ouster metadata"):
    """The sensor's metadata JSON, flat (firmware 2) or in the groups of firmware 3, as the decode's tables.  ``frame``: ``sensor`` applies
    ``lidar_to_sensor_transform``, ``lidar`` the identity.  Everything out of scope is refused by name, before any device is touched."""
    if frame not in OUSTER_FRAMES:
        raise ValueError(f"error: --ouster_frame {frame}: sensor and lidar are the options")
    try:
        doc = json.loads(text)
    except ValueError as e:
        raise ValueError(f"error: {where} is not JSON ({e})") from None
    if not isinstance(doc, dict):
        raise ValueError(f"error: {where} is not a JSON object")

    def get(key, default=None):
        for holder in [doc] + [doc[g] for g in OUSTER_GROUPS if isinstance(doc.get(g), dict)]:
            if key in holder:
                return holder[key]
        return default

    def numbers(key, value):
        if not isinstance(value, list) or any(isinstance(v, bool) or not isinstance(v, (int, float)) for v in value):
            raise ValueError(f"error: {where}: {key} is not a list of numbers")
        if not all(math.isfinite(v) for v in value):
            raise ValueError(f"error: {where}: {key} holds a value that is not finite")
        return [float(v) for v in value]

    def integer(key, default=None):
        v = get(key, default)
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"error: {where}: {key} is {'missing' if v is None else 'not an integer'}")
        return v

    name = get("udp_profile_lidar", "LEGACY")
    if name not in OUSTER_PROFILES:
        if isinstance(name, str) and "FUSA" in name:
            raise ValueError(f"error: {where}: udp_profile_lidar {name}: the FUSA profiles are not decoded here ({', '.join(OUSTER_PROFILES)} are)")
        if isinstance(name, str) and "DUAL" in name:
            raise ValueError(f"error: {where}: udp_profile_lidar {name}: dual-return profiles are not decoded here ({', '.join(OUSTER_PROFILES)} are)")
        raise ValueError(f"error: {where}: unknown udp_profile_lidar {name!r} ({', '.join(OUSTER_PROFILES)} are decoded here)")
    altitude, azimuth = get("beam_altitude_angles"), get("beam_azimuth_angles")
    if altitude is None or azimuth is None:
        raise ValueError(f"error: {where}: no beam_altitude_angles / beam_azimuth_angles: not the metadata of an Ouster sensor")
    altitude, azimuth = numbers("beam_altitude_angles", altitude), numbers("beam_azimuth_angles", azimuth)
    H = integer("pixels_per_column", len(altitude))
    if H not in (16, 32, 64, 128):
        raise ValueError(f"error: {where}: pixels_per_column {H}: sensors of 16, 32, 64 and 128 beams are decoded here")
    W = integer("columns_per_frame")
    if not 16 <= W <= 4096:
        raise ValueError(f"error: {where}: columns_per_frame {W} outside [16, 4096]")
    C = integer("columns_per_packet", 16)
    if not 1 <= C <= 16:
        raise ValueError(f"error: {where}: columns_per_packet {C} outside [1, 16]")
    if len(altitude) != H or len(azimuth) != H:
        raise ValueError(f"error: {where}: {len(altitude)} beam_altitude_angles and {len(azimuth)} beam_azimuth_angles for pixels_per_column {H}")
    n_mm = get("lidar_origin_to_beam_origin_mm", 0.0)
    if isinstance(n_mm, bool) or not isinstance(n_mm, (int, float)) or not math.isfinite(n_mm):
        raise ValueError(f"error: {where}: lidar_origin_to_beam_origin_mm is not a finite number")
    if frame == "sensor":
        transform = get("lidar_to_sensor_transform")
        if transform is None:
            raise ValueError(f"error: {where}: no lidar_to_sensor_transform, which --ouster_frame sensor applies (--ouster_frame lidar does without)")
        transform = numbers("lidar_to_sensor_transform", transform)
        if len(transform) != 16:
            raise ValueError(f"error: {where}: lidar_to_sensor_transform has {len(transform)} entries, not 16")
    else:
        transform = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    column_table = np.array([(math.cos(2.0 * math.pi * (1.0 - m / W)), math.sin(2.0 * math.pi * (1.0 - m / W))) for m in range(W)], dtype=np.float64)
    beam_table = np.array([(math.cos(-math.radians(azimuth[i])), math.sin(-math.radians(azimuth[i])), math.cos(math.radians(altitude[i])), math.sin(math.radians(altitude[i])))
                           for i in range(H)], dtype=np.float64)
    return OusterInfo(name, OUSTER_PROFILES[name], H, W, C, ouster_packet_size(name, H, C), column_table, beam_table, float(n_mm), np.array(transform[:12], dtype=np.float64), frame)


def ouster_columns(packets, info):
    """Of a (n, packet_size) uint8 array: ``(timestamp uint64, measurement_id, valid)`` per column, each (n, C), and the ``frame_id`` (n,)"""
    n = packets.shape[0]
    legacy = info.profile_name == "LEGACY"
    column_bytes = (info.packet_size - (0 if legacy else 64)) // info.C
    cols = packets[:, (0 if legacy else 32) : (0 if legacy else 32) + info.C * column_bytes].reshape(n, info.C, column_bytes)
    timestamp = np.ascontiguousarray(cols[:, :, 0:8]).view("<u8").reshape(n, info.C)
    measurement_id = np.ascontiguousarray(cols[:, :, 8:10]).view("<u2").reshape(n, info.C)
    if legacy:
        valid = np.ascontiguousarray(cols[:, :, column_bytes - 4 :]).view("<u4").reshape(n, info.C) == 0xFFFFFFFF
        frame_id = np.ascontiguousarray(packets[:, 10:12]).view("<u2").reshape(n)
    else:
        valid = (np.ascontiguousarray(cols[:, :, 10:12]).view("<u2").reshape(n, info.C) & 1) != 0
        frame_id = np.ascontiguousarray(packets[:, 2:4]).view("<u2").reshape(n)
    return timestamp, measurement_id, valid, frame_id


def batch_points(messages, cdr=False, lidar=None, warn=None, where=""):
    """The messages of a points topic with the PacketMsg ones grouped into scans: every other message passes through untouched and in
    order; a run of PacketMsg messages becomes one message per scan -- same connection, topic and type, the record time of the scan's
    first packet -- whose ``data`` is an ``OusterBatch``.  A scan closes when the packets' ``frame_id`` changes (LEGACY: uint16 at byte
    10 of the first column header; else uint16 at byte 2 of the packet header), when the topic ends or a message of another kind
    comes, or when it holds ``2 ceil(W / C)`` packets (one warning per bag).  Partial first and last scans are kept; a scan without a valid
    column is skipped with a warning.  A buffer that is not ``packet_size`` long is refused."""
    warn = warn or (lambda msg: None)
    info = getattr(lidar, "ouster", None)
    pending, frame_id, capped = [], None, [False]

    def close():
        first = pending[0][0]
        packets = np.empty((len(pending), info.packet_size), dtype=np.uint8)  # the one copy: contiguous, stride = packet size
        for k, (_, buf) in enumerate(pending):
            packets[k] = buf
        pending.clear()
        timestamp, _, valid, _ = ouster_columns(packets, info)
        if not valid.any():
            warn(f"warning: skip a scan of {packets.shape[0]} Ouster packet(s) without a valid column {where}")
            return None
        return first._replace(data=OusterBatch(packets.reshape(-1), packets.shape[0], int(timestamp[valid].min())))

    for k, m in enumerate(messages):
        if points_kind(m.type) != "PacketMsg":
            if pending:
                out = close()
                if out is not None:
                    yield out
            yield m
            continue
        if info is None:
            raise ValueError(f"error: Ouster packets on topic '{m.topic}' {where} need the sensor's metadata: --ouster_metadata auto (a std_msgs/String topic whose name ends in "
                             "'metadata') or --ouster_metadata FILE.json")
        buf = parse_packet_msg(m.data, cdr)
        if buf.size != info.packet_size:
            raise ValueError(f"error: message {k} of topic '{m.topic}' {where} holds a buffer of {buf.size} bytes, where a {info.profile_name} lidar packet of "
                             f"{info.H} x {info.C} pixels has {info.packet_size}: not a lidar packet of this sensor (the IMU packets are 48 bytes)")
        fid = int(buf[10]) | int(buf[11]) << 8 if info.profile_name == "LEGACY" else int(buf[2]) | int(buf[3]) << 8
        if pending and fid != frame_id:
            out = close()
            if out is not None:
                yield out
        frame_id = fid
        pending.append((m, buf))
        if len(pending) == 2 * -(-info.W // info.C):
            if not capped[0]:
                warn(f"warning: {len(pending)} Ouster packets with frame_id {fid}, two turns of {info.W} columns, {where}: the scan is closed there")
                capped[0] = True
            out = close()
            if out is not None:
                yield out
    if pending:
        out = close()
        if out is not None:
            yield out


def ouster_decode(packets, num_packets, stride, info, ts0, device=0, returns=False):
    """``nidreg_ouster_decode``: ``packets`` a uint8 array whose packet p lies at byte ``p * stride`` (any address).  Returns the
    (num_packets * C * H, 8) uint32 records (32 bytes each: x y z intensity t reflectivity|ring ambient range), with ``returns=True`` also
    the per-packet counts of decoded returns.  A refusal of the entry point is a ``ValueError``."""
    from . import _lib

    n = int(num_packets)
    packets = np.asarray(packets)
    if packets.dtype != np.uint8 or packets.ndim != 1 or (packets.size > 1 and packets.strides[0] != 1):
        raise ValueError("ouster_decode: packets must be a contiguous uint8 array")
    ok = 0 <= n <= OUSTER_MAX_PACKETS and info.H in (16, 32, 64, 128) and 1 <= info.C <= 16
    if ok and n > 0 and stride >= info.packet_size and packets.size < (n - 1) * stride + info.packet_size:
        raise ValueError(f"ouster_decode: {packets.size} bytes for {n} packets of stride {stride}")
    column_table = np.ascontiguousarray(info.column_table, dtype=np.float64)
    beam_table = np.ascontiguousarray(info.beam_table, dtype=np.float64)
    transform12 = np.ascontiguousarray(info.transform12, dtype=np.float64)
    if ok and (column_table.shape != (info.W, 2) or beam_table.shape != (info.H, 4) or transform12.shape != (12,)):
        raise ValueError(f"ouster_decode: tables of shapes {column_table.shape}, {beam_table.shape}, {transform12.shape} for W = {info.W}, H = {info.H}")
    records = np.empty((n * info.C * info.H if ok else 0, 8), dtype=np.uint32)  # (a call the entry point will refuse gets no buffer)
    counts = np.zeros(n if ok else 0, dtype=np.int32) if returns else None
    lib = _lib.load()
    rc = lib.nidreg_ouster_decode(int(device), packets.ctypes.data if packets.size else None, n, int(stride), int(info.profile), int(info.H), int(info.W), int(info.C),
                                  column_table.ctypes.data_as(_lib.c_double_p), beam_table.ctypes.data_as(_lib.c_double_p), float(info.n_mm), transform12.ctypes.data_as(_lib.c_double_p),
                                  int(ts0), records.ctypes.data if records.size else None, None if counts is None else counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    if rc == _lib.NIDREG_ERR_INVALID:
        raise ValueError(_lib.last_error())
    _lib.check(rc, "nidreg_ouster_decode")
    return (records, counts) if returns else records


def ouster_cloud(batch, info, device=0, header_only=False, frame_id="os_sensor"):
    """The cloud of one scan: 32-byte records, one per pixel of every received column in the order packet, column, pixel, height 1, the
    stamp ``ts0`` -- the smallest timestamp of a valid column -- as (sec, nsec).  ``header_only``: the fields without the records."""
    if header_only or batch is None or batch.num_packets == 0:
        return PointCloud2((0, 0), frame_id, 1, 0, list(OUSTER_FIELDS), 0, OUSTER_RECORD_BYTES, 0, np.zeros(0, dtype=np.uint8), 0)
    if batch.num_packets > OUSTER_MAX_PACKETS:
        raise ValueError(f"error: a scan of {batch.num_packets} Ouster packets: at most {OUSTER_MAX_PACKETS} are decoded in one call")
    records = ouster_decode(batch.packets, batch.num_packets, info.packet_size, info, batch.ts0, device=device)
    width = records.shape[0]
    stamp = (batch.ts0 // 1000000000, batch.ts0 % 1000000000)
    return PointCloud2(stamp, "os_lidar" if info.frame == "lidar" else frame_id, 1, width, list(OUSTER_FIELDS), 0, OUSTER_RECORD_BYTES, OUSTER_RECORD_BYTES * width,
                       records.reshape(-1).view(np.uint8), 0)


# ---------------------------------------------------------------------------------------------- the GPU decode
def velodyne_decode(packets, num_packets, stride, packet_times, model, device=0, returns=False):
    """``nidreg_velodyne_decode``: ``packets`` a uint8 array whose packet p lies at byte ``p * stride`` (any address), ``packet_times``
    seconds relative to the scan.  Returns the (num_packets * 384, 5) float32 records x y z intensity time, with ``returns=True`` also
    the per-packet counts of decoded returns.  A refusal of the entry point is a ``ValueError``."""
    from . import _lib

    n = int(num_packets)
    packets = np.asarray(packets)
    if packets.dtype != np.uint8 or packets.ndim != 1 or (packets.size > 1 and packets.strides[0] != 1):
        raise ValueError("velodyne_decode: packets must be a contiguous uint8 array")
    if 0 < n <= MAX_PACKETS and stride >= PACKET_BYTES and packets.size < (n - 1) * stride + PACKET_BYTES:
        raise ValueError(f"velodyne_decode: {packets.size} bytes for {n} packets of stride {stride}")
    times = np.ascontiguousarray(packet_times, dtype=np.float64)
    if times.shape != (n,) and 0 <= n <= MAX_PACKETS:
        raise ValueError(f"velodyne_decode: {times.shape} packet times for {n} packets")
    table = np.ascontiguousarray(model.table, dtype=np.float64)
    records = np.empty((max(0, min(n, MAX_PACKETS)) * POINTS_PER_PACKET, 5), dtype=np.float32)
    counts = np.zeros(max(0, min(n, MAX_PACKETS)), dtype=np.int32) if returns else None
    lib = _lib.load()
    rc = lib.nidreg_velodyne_decode(int(device), packets.ctypes.data if packets.size else None, n, int(stride), times.ctypes.data_as(_lib.c_double_p), table.ctypes.data_as(_lib.c_double_p),
                                    int(table.shape[0]), float(model.distance_resolution), float(model.firing_period), float(model.laser_period),
                                    records.ctypes.data_as(_lib.c_float_p), None if counts is None else counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    if rc == _lib.NIDREG_ERR_INVALID:
        raise ValueError(_lib.last_error())
    _lib.check(rc, "nidreg_velodyne_decode")
    return (records, counts) if returns else records


def packet_times(stamps):
    """Packet stamp - the message's first packet stamp, in seconds: the nanosecond difference, an integer, times 1e-9"""
    if not stamps:
        return np.zeros(0)
    s0, n0 = stamps[0]
    return np.array([float((s - s0) * 1000000000 + (n - n0)) * 1e-9 for s, n in stamps], dtype=np.float64)


def velodyne_cloud(scan, lidar, device=0, where="", header_only=False):
    """The cloud of one scan: x, y, z, intensity, time (float32 at 0, 4, 8, 12, 16), 384 records a packet in packet order, the stamp
    the header's.  Dual-return packets (return mode 0x39) are refused by name.  ``header_only``: the fields without the records."""
    n = scan.num_packets
    if header_only or n == 0:
        return PointCloud2(scan.stamp, scan.frame_id, 1, 0, list(VELODYNE_FIELDS), 0, 20, 0, np.zeros(0, dtype=np.uint8), 0)
    if n > MAX_PACKETS:
        raise ValueError(f"error: a VelodyneScan of {n} packets {where}: at most {MAX_PACKETS} are decoded in one message")
    data = scan.data[PACKET_DATA_OFFSET:]
    factory = np.lib.stride_tricks.as_strided(data[RETURN_MODE_BYTE:], shape=(n, 2), strides=(scan.stride, 1))
    if (factory[:, 0] == DUAL_RETURN).any():
        raise ValueError(f"error: dual return packets (return mode 0x39) {where}: dual-return recordings are not decoded here; record strongest or last return")
    model = (lidar or LidarOptions()).model_for(int(factory[0, 1]))
    records = velodyne_decode(data, n, scan.stride, packet_times(scan.stamps), model, device=device)
    width = n * POINTS_PER_PACKET
    return PointCloud2(scan.stamp, scan.frame_id, 1, width, list(VELODYNE_FIELDS), 0, 20, 20 * width, records.reshape(-1).view(np.uint8), 0)


def decode_points(type_name, data, cdr=False, lidar=None, device=0, where="", header_only=False):
    """The message of a points topic as a ``PointCloud2`` tuple by its connection type, or ``None`` for a type that is not read"""
    kind = points_kind(type_name)
    if kind == "PointCloud2":
        from . import rosbag2

        return (rosbag2 if cdr else rosbag1).decode_pointcloud2(data)
    if kind == "VelodyneScan":
        return velodyne_cloud(parse_velodyne_scan(data, cdr), lidar, device=device, where=where, header_only=header_only)
    if kind == "CustomMsg":
        return parse_livox_custom(data, cdr)
    if kind == "PacketMsg":
        if header_only:
            return ouster_cloud(None, None, header_only=True)
        info = getattr(lidar, "ouster", None)
        if info is None:
            raise ValueError(f"error: Ouster packets {where} need the sensor's metadata: --ouster_metadata auto (a std_msgs/String topic whose name ends in 'metadata') or "
                             "--ouster_metadata FILE.json")
        if not isinstance(data, OusterBatch):  # one message on its own: a scan of one packet
            data = next(iter(batch_points([rosbag1.Message(0, "", type_name, (0, 0), data)], cdr=cdr, lidar=lidar, where=where)), None)
            if data is None:
                return ouster_cloud(None, None, header_only=True)
            data = data.data
        return ouster_cloud(data, info, device=device)
    return None
