"""Host tests of the VelodyneScan / CustomMsg route (direct_visual_lidar_calibration_amd/lidar_messages.py): the two message layouts
on hand-packed bytes, the CustomMsg view through the PointCloud2 accessors, model selection and the calibration file, the topic rule
of ``get_topics -a``, the numpy restatement (tests/velodyne_oracle.py) against two positions worked out from the manual's formulas
alone, the integer azimuth rule against exact fractions, and the refusals of nidreg_velodyne_decode, none of which needs a device."""
import ctypes
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

import lidar_message_fixture as lfx
import rosbag1_fixture as fx1
import rosbag2_fixture as fx2
import velodyne_oracle as vo
from direct_visual_lidar_calibration_amd import _lib, lidar_messages, preprocess_dynamic, preprocess_ros1, preprocess_ros2, rosbag1, rosbag2


def _packet(fill, product_id=0x22, mode=0x37):
    return bytes([fill]) * 1204 + bytes([mode, product_id])


# ---------------------------------------------------------------------------------------------- 1. the layouts
def test_velodyne_scan_ros1_literal_stride_1214():
    p0, p1 = _packet(0x11), _packet(0x22)
    blob = (struct.pack("<III", 7, 100, 500) + struct.pack("<I", 8) + b"velodyne" + struct.pack("<I", 2) + struct.pack("<II", 100, 1000) + p0 + struct.pack("<II", 100, 2000) + p1)
    assert blob == lfx.velodyne_scan_ros1((100, 500), [((100, 1000), p0), ((100, 2000), p1)], seq=7)
    scan = lidar_messages.parse_velodyne_scan(memoryview(blob))
    assert (scan.stamp, scan.frame_id, scan.num_packets, scan.stride, scan.stamps) == ((100, 500), "velodyne", 2, 1214, [(100, 1000), (100, 2000)])
    host = np.frombuffer(blob, dtype=np.uint8)
    assert np.shares_memory(scan.data, host) and scan.data.size == 1214 + 8 + 1206
    assert scan.data[8 : 8 + 1206].tobytes() == p0 and scan.data[1214 + 8 : 1214 + 8 + 1206].tobytes() == p1
    empty = lidar_messages.parse_velodyne_scan(lfx.velodyne_scan_ros1((1, 2), []))
    assert empty.num_packets == 0 and empty.stamps == []


@pytest.mark.parametrize("frame_id", ["velodyne", "velodyn", "lidar0", "v"])
@pytest.mark.parametrize("final_padding", [False, True])
def test_velodyne_scan_cdr_stride_1216_whatever_the_frame_id_does_to_the_alignment(frame_id, final_padding):
    p = [_packet(0x10 + k) for k in range(3)]
    blob = lfx.velodyne_scan_cdr((5, 6), [((5, 100 + k), p[k]) for k in range(3)], frame_id=frame_id, final_padding=final_padding)
    # by hand: encapsulation, stamp, the string with its NUL, padding to 4, the count, then elements 1216 apart
    head = b"\x00\x01\x00\x00" + struct.pack("<iI", 5, 6) + struct.pack("<I", len(frame_id) + 1) + frame_id.encode() + b"\x00"
    head += b"\x00" * ((4 - (len(head) - 4) % 4) % 4) + struct.pack("<I", 3)
    assert blob[: len(head)] == head and blob[len(head) + 1216 : len(head) + 1216 + 8] == struct.pack("<iI", 5, 101)
    assert len(blob) == len(head) + 2 * 1216 + 1214 + (2 if final_padding else 0)
    scan = lidar_messages.parse_velodyne_scan(memoryview(blob), cdr=True)
    assert (scan.stamp, scan.frame_id, scan.num_packets, scan.stride) == ((5, 6), frame_id, 3, 1216)
    assert scan.stamps == [(5, 100), (5, 101), (5, 102)] and np.shares_memory(scan.data, np.frombuffer(blob, dtype=np.uint8))
    for k in range(3):
        assert scan.data[k * 1216 + 8 : k * 1216 + 8 + 1206].tobytes() == p[k]


def _points(n, seed=3):
    rng = np.random.default_rng(seed)
    pts = np.zeros(n, dtype=lfx.CUSTOM_POINT)
    pts["t"] = np.sort(rng.integers(0, 100000000, n)).astype(np.uint32)
    for c in "xyz":
        pts[c] = rng.uniform(-20.0, 20.0, n).astype(np.float32)
    pts["reflectivity"], pts["tag"], pts["line"] = rng.integers(0, 256, n), rng.integers(0, 256, n), rng.integers(0, 6, n)
    return pts


def test_custom_msg_ros1_literal_step_19():
    pts = _points(3)
    blob = struct.pack("<III", 1, 200, 9) + struct.pack("<I", 5) + b"livox" + struct.pack("<Q", 123456789012) + struct.pack("<I", 3) + b"\x02\x00\x00\x00" + struct.pack("<I", 3)
    for q in pts:
        blob += struct.pack("<IfffBBB", *q.tolist())
    assert blob == lfx.custom_msg_ros1((200, 9), pts, frame_id="livox", seq=1, timebase=123456789012, lidar_id=2)
    cloud = lidar_messages.parse_livox_custom(memoryview(blob))
    assert (cloud.stamp, cloud.frame_id, cloud.height, cloud.width, cloud.point_step, cloud.is_bigendian) == ((200, 9), "livox", 1, 3, 19, 0)
    assert [(f.name, f.offset, f.datatype) for f in cloud.fields] == [("t", 0, 6), ("x", 4, 7), ("y", 8, 7), ("z", 12, 7), ("reflectivity", 16, 2), ("tag", 17, 2), ("line", 18, 2)]
    assert np.shares_memory(cloud.data, np.frombuffer(blob, dtype=np.uint8)) and cloud.data.tobytes() == pts.tobytes()
    assert lidar_messages.parse_livox_custom(lfx.custom_msg_ros1((1, 0), _points(0))).width == 0


@pytest.mark.parametrize("frame_id", ["livox_frame", "livox", "l"])
def test_custom_msg_cdr_step_20_with_and_without_the_final_padding_byte(frame_id):
    pts = _points(5)
    padded = np.zeros((5, 20), dtype=np.uint8)
    padded[:, :19] = np.frombuffer(pts.tobytes(), dtype=np.uint8).reshape(5, 19)
    full = lfx.custom_msg_cdr((7, 8), pts, frame_id=frame_id, timebase=99, lidar_id=1)
    short = lfx.custom_msg_cdr((7, 8), pts, frame_id=frame_id, timebase=99, lidar_id=1, final_padding=False)
    assert len(full) == len(short) + 1
    # timebase is aligned to 8 from the byte after the encapsulation header
    string_end = 4 + 8 + 4 + len(frame_id) + 1
    timebase_at = string_end + (8 - (string_end - 4) % 8) % 8
    assert struct.unpack_from("<Q", full, timebase_at)[0] == 99 and struct.unpack_from("<IB", full, timebase_at + 8) == (5, 1)
    for blob, zero_copy in ((full, True), (short, False)):
        cloud = lidar_messages.parse_livox_custom(memoryview(blob), cdr=True)
        assert (cloud.stamp, cloud.frame_id, cloud.width, cloud.point_step, cloud.row_step) == ((7, 8), frame_id, 5, 20, 100)
        assert cloud.data.size == 100 and np.array_equal(cloud.data.reshape(5, 20), padded)
        assert np.shares_memory(cloud.data, np.frombuffer(blob, dtype=np.uint8)) == zero_copy
    assert lidar_messages.parse_livox_custom(lfx.custom_msg_cdr((1, 0), _points(0)), cdr=True).width == 0


def test_truncated_messages_are_value_errors():
    scan1 = lfx.velodyne_scan_ros1((1, 2), [((1, 3), _packet(1)), ((1, 4), _packet(2))])
    scan2 = lfx.velodyne_scan_cdr((1, 2), [((1, 3), _packet(1)), ((1, 4), _packet(2))])
    livox1 = lfx.custom_msg_ros1((1, 2), _points(4))
    livox2 = lfx.custom_msg_cdr((1, 2), _points(4), final_padding=False)
    for parse, blob, cdr in ((lidar_messages.parse_velodyne_scan, scan1, False), (lidar_messages.parse_velodyne_scan, scan2, True), (lidar_messages.parse_livox_custom, livox1, False),
                             (lidar_messages.parse_livox_custom, livox2, True)):
        parse(blob, cdr=cdr)
        for cut in (1, 3, 700, len(blob) - 10, len(blob) - 4):
            with pytest.raises(ValueError, match="truncated"):
                parse(blob[: len(blob) - cut], cdr=cdr)
    huge = bytearray(scan1)
    struct.pack_into("<I", huge, 12 + 4 + 8, 0xFFFFFFFF)  # the packet count
    with pytest.raises(ValueError, match="truncated"):
        lidar_messages.parse_velodyne_scan(bytes(huge))


def test_decode_points_is_on_both_readers_and_goes_by_type():
    pts = _points(6)
    for reader, type_, blob in ((rosbag1, lfx.LIVOX1, lfx.custom_msg_ros1((3, 4), pts)), (rosbag1, lfx.LIVOX1_V2, lfx.custom_msg_ros1((3, 4), pts)),
                                (rosbag2, lfx.LIVOX2, lfx.custom_msg_cdr((3, 4), pts))):
        cloud = reader.decode_points(type_, blob)
        assert cloud.width == 6 and cloud.point_step == (19 if reader is rosbag1 else 20)
    rec = np.zeros(2, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
    assert rosbag1.decode_points("sensor_msgs/PointCloud2", fx1.cloud_from_struct((1, 0), rec)).width == 2
    assert rosbag2.decode_points(fx2.PC2, fx2.cloud_from_struct((1, 0), rec)).width == 2
    assert rosbag1.decode_points("sensor_msgs/Image", b"") is None and rosbag2.decode_points("sensor_msgs/msg/Imu", b"") is None
    # of a VelodyneScan the fields alone, without a device
    head = rosbag1.decode_points(lfx.SCAN1, lfx.velodyne_scan_ros1((1, 2), [((1, 3), _packet(1))]), header_only=True)
    assert [(f.name, f.offset, f.datatype) for f in head.fields] == [("x", 0, 7), ("y", 4, 7), ("z", 8, 7), ("intensity", 12, 7), ("time", 16, 7)] and head.point_step == 20


# ---------------------------------------------------------------------------------------------- 2. the CustomMsg view
@pytest.mark.parametrize("cdr", [False, True])
def test_custom_msg_view_gives_the_packed_columns_back_exactly(cdr):
    pts = _points(50, seed=9)
    cloud = lidar_messages.parse_livox_custom(lfx.custom_msg_cdr((12, 500000000), pts, final_padding=False) if cdr else lfx.custom_msg_ros1((12, 500000000), pts), cdr=cdr)
    table = rosbag1.field_table(cloud)
    for name in ("x", "y", "z", "reflectivity", "t", "tag", "line"):
        assert np.array_equal(rosbag1.read_field_all(cloud, table[name]), pts[name].astype(np.float64)), name
    assert preprocess_ros1.time_field(cloud).name == "t"
    stamp, first, last, min_time = preprocess_ros1.frame_times(cloud, "(here)")
    assert (stamp, first, last) == (12.5, float(pts["t"][0]) / 1e9, float(pts["t"][-1]) / 1e9) and min_time() == float(pts["t"].min()) / 1e9
    assert 0.0 <= first < last < 0.1


# ---------------------------------------------------------------------------------------------- 3. models
def test_model_selection_by_product_id_and_by_name():
    for pid, name, lasers, firing, laser in ((0x22, "vlp16", 16, 55.296e-6, 2.304e-6), (0x21, "hdl32e", 32, 46.080e-6, 1.152e-6)):
        m = lidar_messages.LidarOptions("auto").model_for(pid)
        assert (m.name, m.table.shape, m.distance_resolution, m.firing_period, m.laser_period) == (name, (lasers, 8), 0.002, firing, laser)
        table, res, f, l = vo.model(name)
        assert np.array_equal(m.table, table) and (res, f, l) == (0.002, firing, laser)
        assert lidar_messages.LidarOptions(name).model_for(0x99).name == name  # a named model does not look at the id
    vlp = lidar_messages.builtin_model("vlp16").table
    assert np.allclose(np.degrees(np.arctan2(vlp[:, 1], vlp[:, 0])), [-15, 1, -13, 3, -11, 5, -9, 7, -7, 9, -5, 11, -3, 13, -1, 15], atol=1e-12)
    assert vlp[:, 4].tolist() == vo.VLP16_VOFF and not vlp[:, 5:].any() and np.array_equal(vlp[:, 2:4], np.tile([1.0, 0.0], (16, 1)))
    hdl = lidar_messages.builtin_model("hdl32e").table
    deg = np.degrees(np.arctan2(hdl[:, 1], hdl[:, 0]))
    assert np.allclose(deg[[0, 1, 2, 3, 30, 31]], [-30.67, -9.33, -29.33, -8.0, -10.67, 10.67], atol=0.005) and not hdl[:, 4:].any()
    assert np.allclose(np.sort(deg), -92.0 / 3.0 + (4.0 / 3.0) * np.arange(32), atol=1e-12)
    for pid in (0x24, 0x28, 0xA1, 0x00):
        with pytest.raises(ValueError, match=rf"0x{pid:02X}.*--lidar_model vlp16 or --lidar_model hdl32e"):
            lidar_messages.LidarOptions("auto").model_for(pid)
    with pytest.raises(ValueError, match="auto, vlp16 and hdl32e"):
        lidar_messages.LidarOptions("vlp32c")


def test_dual_return_is_refused_by_name_before_any_device_call():
    packets = [((1, k), _packet(0, mode=0x39 if k == 2 else 0x37)) for k in range(4)]
    for reader, type_, blob in ((rosbag1, lfx.SCAN1, lfx.velodyne_scan_ros1((1, 0), packets)), (rosbag2, lfx.SCAN2, lfx.velodyne_scan_cdr((1, 0), packets))):
        with pytest.raises(ValueError, match="dual return"):
            reader.decode_points(type_, blob, where="(there)")


def _calibration(tmp_path, n=16, edit=lambda e: None, name="cal.yaml"):
    import yaml

    lasers = []
    for i in reversed(range(n)):  # listed in descending order: laser_id places a row, not its position in the file
        e = {"laser_id": i, "vert_correction": 0.01 * (i - 7), "rot_correction": 0.001 * i, "vert_offset_correction": 0.0001 * i, "horiz_offset_correction": -0.0002 * i,
             "dist_correction": 0.003 * i, "dist_correction_x": 0.0, "dist_correction_y": 0.0, "focal_distance": 0.0, "focal_slope": 0.0}
        edit(e)
        lasers.append(e)
    path = tmp_path / name
    path.write_text(yaml.safe_dump({"num_lasers": n, "distance_resolution": 0.004, "lasers": lasers}))
    return str(path)


def test_calibration_yaml_becomes_the_laser_table(tmp_path):
    m = lidar_messages.LidarOptions("auto", _calibration(tmp_path)).model_for(0x24)  # how a Puck Hi-Res is read: its id plays no part
    assert m.table.shape == (16, 8) and (m.distance_resolution, m.firing_period, m.laser_period) == (0.004, 55.296e-6, 2.304e-6)
    for i in range(16):
        want = [math.cos(0.01 * (i - 7)), math.sin(0.01 * (i - 7)), math.cos(0.001 * i), math.sin(0.001 * i), 0.0001 * i, -0.0002 * i, 0.003 * i, 0.0]
        assert m.table[i].tolist() == want
    m32 = lidar_messages.load_calibration(_calibration(tmp_path, 32, name="cal32.yaml"))
    assert m32.table.shape == (32, 8) and (m32.firing_period, m32.laser_period) == (46.080e-6, 1.152e-6)
    for key in ("dist_correction_x", "dist_correction_y", "focal_distance", "focal_slope"):
        with pytest.raises(ValueError, match=key):
            lidar_messages.load_calibration(_calibration(tmp_path, edit=lambda e: e.update({key: 0.25}) if e["laser_id"] == 5 else None, name=key + ".yaml"))
    with pytest.raises(ValueError, match="num_lasers 64"):
        lidar_messages.load_calibration(_calibration(tmp_path, 64, name="cal64.yaml"))
    with pytest.raises(ValueError, match="different packet layouts"):
        lidar_messages.LidarOptions("hdl32e", _calibration(tmp_path))


def test_the_three_commands_take_the_two_options():
    for module in (preprocess_ros1, preprocess_ros2, preprocess_dynamic):
        args = module.build_parser().parse_args(["src", "dst"])
        assert (args.lidar_model, args.velodyne_calibration) == ("auto", None)
        args = module.build_parser().parse_args(["src", "dst", "--lidar_model", "hdl32e", "--velodyne_calibration", "cal.yaml"])
        assert (args.lidar_model, args.velodyne_calibration) == ("hdl32e", "cal.yaml")


# ---------------------------------------------------------------------------------------------- 4. get_topics -a
class _Bag:
    path = "fake.bag"

    def __init__(self, topics):
        self._topics = topics

    def topics_and_types(self):
        return self._topics


CAMERA = [("/cam/info", "sensor_msgs/CameraInfo"), ("/cam/image", "sensor_msgs/Image")]


@pytest.mark.parametrize("topics,want,warnings", [
    ([("/velodyne_points", "sensor_msgs/PointCloud2")], "/velodyne_points", 0),
    ([("/velodyne_packets", "velodyne_msgs/VelodyneScan")], "/velodyne_packets", 0),
    ([("/velodyne_packets", "velodyne_msgs/msg/VelodyneScan")], "/velodyne_packets", 0),
    ([("/livox/lidar", "livox_ros_driver/CustomMsg")], "/livox/lidar", 0),
    ([("/livox/lidar", "livox_ros_driver2/msg/CustomMsg")], "/livox/lidar", 0),
    ([("/velodyne_packets", "velodyne_msgs/VelodyneScan"), ("/velodyne_points", "sensor_msgs/PointCloud2")], "/velodyne_points", 0),
    ([("/velodyne_points", "sensor_msgs/PointCloud2"), ("/velodyne_packets", "velodyne_msgs/VelodyneScan"), ("/livox/lidar", "livox_ros_driver/CustomMsg")], "/velodyne_points", 1),
    ([("/a", "velodyne_msgs/VelodyneScan"), ("/b", "livox_ros_driver2/CustomMsg")], "/b", 1),
])
def test_get_topics_auto_prefers_a_pointcloud2_topic(topics, want, warnings):
    args = preprocess_ros1.build_parser().parse_args(["src", "dst", "-a"])
    warned = []
    got = preprocess_ros1.get_topics(args, _Bag(CAMERA + topics), log=lambda m: None, warn=warned.append)
    assert got == ("/cam/info", "/cam/image", want)
    assert len([w for w in warned if "multiple points topics" in w]) == warnings
    # --points_topic may name a topic of any kind
    named = preprocess_ros1.build_parser().parse_args(["src", "dst", "--points_topic", topics[0][0], "--image_topic", "/cam/image", "--camera_info_topic", "/cam/info"])
    assert preprocess_ros1.get_topics(named, _Bag(CAMERA + topics), log=lambda m: None, warn=warned.append)[2] == topics[0][0]


def test_lidar_options_are_ignored_with_one_line_on_another_topic(tmp_path):
    logged = []
    args = preprocess_ros1.build_parser().parse_args(["src", "dst", "--lidar_model", "vlp16", "--velodyne_calibration", str(tmp_path / "missing.yaml")])
    assert preprocess_ros1.lidar_options(args, _Bag([("/p", "sensor_msgs/PointCloud2")]), "/p", log=logged.append) is None
    assert len(logged) == 1 and "ignored" in logged[0]
    quiet = preprocess_ros1.build_parser().parse_args(["src", "dst"])
    assert preprocess_ros1.lidar_options(quiet, _Bag([("/l", "livox_ros_driver/CustomMsg")]), "/l", log=logged.append) is None and len(logged) == 1
    args.velodyne_calibration = None
    assert preprocess_ros1.lidar_options(args, _Bag([("/v", "velodyne_msgs/VelodyneScan")]), "/v", log=logged.append).model.name == "vlp16" and len(logged) == 1


# ---------------------------------------------------------------------------------------------- 5. the restatement against the manual
def _single_azimuth_packet(azimuth, slot, raw):
    distances = np.zeros((12, 32), dtype=np.int64)
    distances[:, slot] = raw
    return vo.encode_packet([azimuth] * 12, distances, np.full((12, 32), 77))


@pytest.mark.parametrize("azimuth,slot,elevation_deg,offset,raw", [(9000, 1, 1.0, -0.0007, 5000), (0, 15, 15.0, -0.0112, 25000)])
def test_oracle_geometry_against_the_manual(azimuth, slot, elevation_deg, offset, raw):
    """The expected position comes from the manual's formulas with ``math`` alone: range R = raw * 2 mm along the laser's elevation w,
    the laser's origin ``offset`` above the sensor's, perpendicular to the beam: xy = R cos w - offset sin w, z = R sin w + offset cos w;
    azimuth a clockwise from +y in the sensor's frame, i.e. (x, y) = (xy cos a, -xy sin a) in the ROS frame.  1e-5 m: half a float32 ulp
    at 100 m (3.8e-6) with room for the double rounding; nothing else enters."""
    table, res, firing, laser = vo.model("vlp16")
    packet = _single_azimuth_packet(azimuth, slot, raw)
    rec, counts = vo.decode(np.frombuffer(packet, dtype=np.uint8), 1206, [0.0], table, res, firing, laser)
    R, w, a = raw * 0.002, math.radians(elevation_deg), math.radians(azimuth / 100.0)
    xy, z = R * math.cos(w) - offset * math.sin(w), R * math.sin(w) + offset * math.cos(w)
    want = (xy * math.cos(a), -xy * math.sin(a), z)
    if azimuth == 9000:
        assert abs(xy - 9.998489) < 1e-6 and abs(z - 0.173824) < 1e-6 and abs(want[0]) < 1e-12
    else:
        assert abs(want[0] - 48.299190) < 1e-6 and want[1] == 0.0 and abs(z - 12.930134) < 1e-6
    assert counts.tolist() == [12]
    for b in range(12):
        got = rec[b * 32 + slot]
        assert np.abs(got[:3].astype(np.float64) - want).max() < 1e-5, (b, got, want)
        assert got[3] == 77.0 and got[4] == np.float32((2 * b + slot // 16) * firing + (slot % 16) * laser)
    others = np.delete(rec, [b * 32 + slot for b in range(12)], axis=0)
    assert np.isnan(others[:, :3]).all() and not others[:, 3].any()


def test_integer_azimuth_rule_equals_the_rounded_fraction():
    """floor(a + diff (l + 24 f) / 48 + 1 / 2) mod 36000: (2.304 l + 55.296 f) / 110.592 = (l + 24 f) / 48, rounded half up"""
    halves = 0
    for diff in (0, 1, 23, 24, 40, 35999):
        for f in (0, 1):
            for l in range(16):
                exact = Fraction(diff * (l + 24 * f), 48) + Fraction(1, 2)
                halves += exact.denominator == 1 and (Fraction(diff * (l + 24 * f), 48)).denominator == 2
                for a in (0, 17, 35990, 35999):
                    assert vo.interpolated_azimuth(a, diff, l, f) == (a + math.floor(exact)) % 36000, (a, diff, l, f)
    assert halves > 0  # the exact halves are among them


def test_azimuth_rule_stays_in_the_table_for_any_uint16_fields():
    """The modulo of the rule is the floored one: with a[b+1] - a[b] + 36000 < 0 (fields above 35999) diff is still in [0, 35999]"""
    for a0, a1 in ((65535, 0), (65535, 36000), (0, 65535), (36000, 35999), (50000, 10000)):
        diff = (a1 - a0 + 36000) % 36000
        assert 0 <= diff < 36000 and diff == Fraction(a1 - a0, 1) - 36000 * math.floor(Fraction(a1 - a0, 36000))
        for l, f in ((0, 0), (1, 0), (15, 1)):
            assert 0 <= vo.interpolated_azimuth(a0, diff, l, f) < 36000
    packet = vo.encode_packet([100 * b for b in range(10)] + [65535, 0], np.full((12, 32), 1000), np.full((12, 32), 1))
    rec, counts = vo.decode(np.frombuffer(packet, dtype=np.uint8), 1206, [0.0], *vo.model("vlp16"))
    assert counts.tolist() == [384] and np.isfinite(rec).all()
    # block 11, laser 1 of the first firing: az = (0 + (2 * 6465 * 1 + 48) // 96) = 135 -> bearing 1.35 degrees
    assert abs(math.degrees(math.atan2(-rec[11 * 32 + 1, 1], rec[11 * 32 + 1, 0])) - 1.35) < 1e-3


def test_oracle_decodes_what_the_encoder_wrote_and_wraps_the_azimuth():
    rng = np.random.default_rng(5)
    az = [35960, 35980, 0, 20, 40, 60, 80, 100, 120, 140, 35990, 10]
    packet = vo.encode_packet(az, rng.integers(1, 65536, (12, 32)), rng.integers(0, 256, (12, 32)))
    assert packet[:4] == b"\xff\xee" + struct.pack("<H", 35960) and packet[1204:] == b"\x37\x22" and len(packet) == 1206
    table, res, firing, laser = vo.model("vlp16")
    rec, counts = vo.decode(np.frombuffer(packet, dtype=np.uint8), 1206, [0.25], table, res, firing, laser)
    assert counts.tolist() == [384] and np.isfinite(rec).all()
    # bearing of laser 1 (+1 degree, first firing of each block): atan2(-y, x) is the interpolated azimuth; blocks 10 and 11 share diff 20
    for b, want in ((0, 35960), (1, 35980), (2, 0), (10, 35990), (11, 10)):
        diff = 20 if b != 9 else (35990 - 140) % 36000
        got = math.degrees(math.atan2(-rec[b * 32 + 1, 1], rec[b * 32 + 1, 0])) % 360.0
        assert abs(got - vo.interpolated_azimuth(want, diff, 1, 0) / 100.0) < 1e-3, b
    assert rec[32 * 11 + 31, 4] == np.float32(0.25 + (23 * firing + 15 * laser))


# ---------------------------------------------------------------------------------------------- 6. refusals of the entry point
def _call(num_packets, stride=1206, lasers=16, packets=True, times=True, table=None, res=0.002, firing=55.296e-6, laser=2.304e-6, out=True, n_alloc=1):
    lib = _lib.load()
    buf = np.zeros(n_alloc * min(max(stride, 1206), 8192), dtype=np.uint8)  # (a refused stride is never read)
    t = np.zeros(n_alloc)
    tab = np.ascontiguousarray(vo.model("vlp16")[0] if table is None else table)
    rec = np.full((n_alloc * 384, 5), 7.0, dtype=np.float32)
    rc = lib.nidreg_velodyne_decode(0, buf.ctypes.data if packets else None, num_packets, stride, t.ctypes.data_as(_lib.c_double_p) if times else None, tab.ctypes.data_as(_lib.c_double_p), lasers,
                                    res, firing, laser, rec.ctypes.data_as(_lib.c_float_p) if out else None, None)
    assert (rec == 7.0).all()  # nothing is written by a refusal, or for 0 packets
    return rc, _lib.last_error()


def test_entry_point_refusals_need_no_device():
    assert hasattr(_lib.load(), "nidreg_velodyne_decode") and "nidreg_velodyne_decode" in _lib.EXPORTS
    assert _call(0)[0] == 0 and _call(0, packets=False, times=False, out=False)[0] == 0  # 0 packets: valid, no device
    for kw, text in ((dict(lasers=64), "num_lasers 64"), (dict(lasers=0), "num_lasers 0"), (dict(stride=1205), "packet_stride 1205"), (dict(stride=4097), "packet_stride 4097"), (dict(stride=2**62), "packet_stride"), (dict(num_packets=-1), "num_packets -1"),
                     (dict(num_packets=65537), "num_packets 65537"), (dict(packets=False), "null"), (dict(times=False), "null"), (dict(out=False), "null"),
                     (dict(res=float("nan")), "not finite"), (dict(firing=float("inf")), "not finite"), (dict(laser=float("-inf")), "not finite")):
        kw.setdefault("num_packets", 1)
        rc, err = _call(**kw)
        assert rc == _lib.NIDREG_ERR_INVALID and "nidreg_velodyne_decode" in err and text in err, (kw, err)
    bad = vo.model("vlp16")[0].copy()
    bad[9, 4] = np.nan
    rc, err = _call(1, table=bad)
    assert rc == _lib.NIDREG_ERR_INVALID and "laser 9" in err
    # 65536 packets pass the count check: the refusal that follows is the NULL pointer's, not the count's
    rc, err = _call(65536, packets=False)
    assert rc == _lib.NIDREG_ERR_INVALID and "null" in err and "num_packets" not in err
