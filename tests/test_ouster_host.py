"""Host-side tests of the Ouster route (no GPU): the PacketMsg parse, the metadata JSON in both shapes and every refusal, the batching of
packets into scans, the topic choice under -a, the options on another topic, the packet sizes, and tests/ouster_oracle.py against pixels
whose position follows from the formulas without a computer."""
import json
import math

import numpy as np
import pytest

import ouster_fixture as ofx
import ouster_oracle as oo
from direct_visual_lidar_calibration_amd import lidar_messages, preprocess_dynamic, preprocess_ros1, preprocess_ros2, rosbag1, rosbag2

H, W, C = 16, 512, 16
ALT, AZ = ofx.os_angles(H)


def _info(profile=ofx.RNG19, shape="flat", frame="sensor", **kw):
    args = dict(H=H, W=W, C=C, altitude=ALT, azimuth=AZ)
    args.update(kw)
    return lidar_messages.ouster_info(ofx.metadata(profile, shape=shape, **args), frame)


def _column(profile, m, t, valid=True, h=H, range_=1000):
    status = ofx.VALID[profile] if valid else 0
    return ofx.Column(t, m, status, [range_] * h, [1] * h, [2] * h, [3] * h)


def _packet(profile, frame_id, m0, t0, valid=True, c=C, h=H):
    return ofx.encode_packet(profile, [_column(profile, m0 + k, t0 + k, valid, h) for k in range(c)], frame_id)


# ---------------------------------------------------------------------------------------------- 1. the message
def test_points_kind_knows_the_three_packet_msg_types():
    for name in (ofx.PACKET1, ofx.PACKET2, ofx.PACKET2_SENSOR, "PacketMsg"):
        assert lidar_messages.points_kind(name) == "PacketMsg"
    assert lidar_messages.points_kind("ouster_ros/PacketMsgs") is None and lidar_messages.points_kind("std_msgs/String") is None


def test_packet_msg_parse_is_a_bounds_checked_view():
    buf = bytes(range(256)) * 3
    got = lidar_messages.parse_packet_msg(ofx.packet_msg_ros1(buf))
    assert got.dtype == np.uint8 and got.tobytes() == buf and not got.flags.owndata
    blob = ofx.packet_msg_cdr(buf)
    assert blob[:4] == b"\x00\x01\x00\x00" and lidar_messages.parse_packet_msg(blob, cdr=True).tobytes() == buf
    # a CDR blob at an odd offset of a larger buffer: a view, whatever its address
    big = np.frombuffer(b"\x77" * 3 + blob + b"\x77" * 5, dtype=np.uint8)
    view = memoryview(big)[3 : 3 + len(blob)]
    got = lidar_messages.parse_packet_msg(view, cdr=True)
    assert got.tobytes() == buf and got.ctypes.data == big.ctypes.data + 3 + 8 and got.ctypes.data % 2 == 1
    with pytest.raises(ValueError, match="truncated"):
        lidar_messages.parse_packet_msg(ofx.packet_msg_ros1(buf)[:-1])
    with pytest.raises(ValueError, match="truncated"):
        lidar_messages.parse_packet_msg(blob[:-1], cdr=True)
    assert lidar_messages.parse_packet_msg(ofx.packet_msg_ros1(b"")).size == 0


def test_string_messages():
    assert rosbag1.decode_string(ofx.string_ros1('{"a": 1}')) == '{"a": 1}'
    assert rosbag2.decode_string(ofx.string_cdr('{"a": 1}')) == '{"a": 1}'


# ---------------------------------------------------------------------------------------------- 2. packet sizes
def test_packet_sizes_against_the_hand_checked_values():
    assert [lidar_messages.ouster_packet_size(p, 64, 16) for p in (ofx.LEGACY, ofx.RNG19, ofx.RNG15)] == [12608, 12544, 4352]
    assert [oo.packet_size(p, 64, 16) for p in oo.PROFILES] == [12608, 12544, 4352]
    for p in (ofx.LEGACY, ofx.RNG19, ofx.RNG15):  # ... and the writer, which knows no formula
        for h, c in ((16, 16), (128, 4), (32, 1)):
            assert len(_packet(p, 1, 0, 0, c=c, h=h)) == lidar_messages.ouster_packet_size(p, h, c) == oo.packet_size(p, h, c)


# ---------------------------------------------------------------------------------------------- 3. metadata
@pytest.mark.parametrize("profile", [ofx.LEGACY, ofx.RNG19, ofx.RNG15])
def test_both_shapes_of_the_metadata_give_the_same_tables(profile):
    flat, nested = _info(profile, "flat"), _info(profile, "nested")
    assert "udp_profile_lidar" not in json.loads(ofx.metadata(ofx.LEGACY, H, W, C, ALT, AZ))  # absent means LEGACY
    for a, b in zip(flat, nested):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    assert (flat.profile_name, flat.H, flat.W, flat.C, flat.packet_size) == (profile, H, W, C, oo.packet_size(profile, H, C))
    assert flat.profile == oo.PROFILES.index(profile) and flat.n_mm == 15.806
    assert np.array_equal(flat.column_table, oo.column_table(W)) and np.array_equal(flat.beam_table, oo.beam_table(AZ, ALT))
    assert flat.transform12.tolist() == ofx.OS1_TRANSFORM[:12]
    assert _info(profile, frame="lidar").transform12.tolist() == list(oo.IDENTITY12)


def test_columns_per_packet_defaults_to_16():
    doc = json.loads(ofx.metadata(ofx.RNG19, H, W, C, ALT, AZ))
    del doc["columns_per_packet"]
    assert lidar_messages.ouster_info(json.dumps(doc)).C == 16


def _refused(match, **changes):
    doc = json.loads(ofx.metadata(ofx.RNG19, H, W, C, ALT, AZ))
    doc.update(changes)
    with pytest.raises(ValueError, match=match):
        lidar_messages.ouster_info(json.dumps(doc).replace('"NAN"', "NaN").replace('"INF"', "Infinity"))


def test_every_refusal_of_the_metadata_is_raised_by_name():
    _refused("dual-return", udp_profile_lidar="RNG19_RFL8_SIG16_NIR16_DUAL")
    _refused("FUSA", udp_profile_lidar="FUSA_RNG15_RFL8_NIR8_DUAL")
    _refused("unknown udp_profile_lidar 'RNG12_FOO'", udp_profile_lidar="RNG12_FOO")
    for h in (8, 48, 256):
        _refused(f"pixels_per_column {h}", pixels_per_column=h)
    _refused("columns_per_frame 15 outside", columns_per_frame=15)
    _refused("columns_per_frame 4097 outside", columns_per_frame=4097)
    _refused("columns_per_packet 0 outside", columns_per_packet=0)
    _refused("columns_per_packet 17 outside", columns_per_packet=17)
    _refused("15 beam_altitude_angles and 16 beam_azimuth_angles", beam_altitude_angles=ALT[:-1])
    _refused("16 beam_altitude_angles and 17 beam_azimuth_angles", beam_azimuth_angles=AZ + [0.0])
    _refused("beam_altitude_angles holds a value that is not finite", beam_altitude_angles=ALT[:-1] + ["NAN"])
    _refused("beam_azimuth_angles holds a value that is not finite", beam_azimuth_angles=["INF"] + AZ[1:])
    _refused("lidar_to_sensor_transform holds a value that is not finite", lidar_to_sensor_transform=ofx.OS1_TRANSFORM[:5] + ["NAN"] + ofx.OS1_TRANSFORM[6:])
    _refused("lidar_origin_to_beam_origin_mm is not a finite number", lidar_origin_to_beam_origin_mm="INF")
    _refused("lidar_to_sensor_transform has 12 entries", lidar_to_sensor_transform=ofx.OS1_TRANSFORM[:12])
    with pytest.raises(ValueError, match="not JSON"):
        lidar_messages.ouster_info("{")
    with pytest.raises(ValueError, match="--ouster_frame"):
        lidar_messages.ouster_info(ofx.metadata(ofx.RNG19, H, W, C, ALT, AZ), "base")
    # a nested document's refusals come from its groups
    with pytest.raises(ValueError, match="dual-return"):
        lidar_messages.ouster_info(ofx.metadata("RNG19_RFL8_SIG16_NIR16_DUAL", H, W, C, ALT, AZ, shape="nested"))


# ---------------------------------------------------------------------------------------------- 4. batching
def _messages(packets, type_=ofx.PACKET1, cdr=False):
    pack = ofx.packet_msg_cdr if cdr else ofx.packet_msg_ros1
    return [rosbag1.Message(7, "/ouster/lidar_packets", type_, (100, k), pack(p)) for k, p in enumerate(packets)]


def _batch(packets, profile=ofx.RNG19, cdr=False, **kw):
    lidar = lidar_messages.LidarOptions(ouster=_info(profile, **kw))
    warned = []
    out = list(lidar_messages.batch_points(_messages(packets, cdr=cdr), cdr=cdr, lidar=lidar, warn=warned.append, where="(in fake.bag)"))
    return out, warned


@pytest.mark.parametrize("profile", [ofx.LEGACY, ofx.RNG19, ofx.RNG15])
@pytest.mark.parametrize("cdr", [False, True])
def test_two_full_scans_behind_a_partial_first_one(profile, cdr):
    per_scan = W // C
    packets = [_packet(profile, 9, (per_scan - 3 + k) * C, 5000 + k * 100) for k in range(3)]  # the tail of scan 9
    packets += [_packet(profile, 10, k * C, 10000 + k * 100) for k in range(per_scan)] + [_packet(profile, 11, k * C, 20000 + k * 100) for k in range(per_scan)]
    out, warned = _batch(packets, profile, cdr)
    assert not warned and [m.data.num_packets for m in out] == [3, per_scan, per_scan] and [m.data.ts0 for m in out] == [5000, 10000, 20000]
    assert [m.time for m in out] == [(100, 0), (100, 3), (100, 3 + per_scan)] and all(m.conn == 7 and m.type == ofx.PACKET1 for m in out)
    size = len(packets[0])
    for m, (a, b) in zip(out, ((0, 3), (3, 3 + per_scan), (3 + per_scan, 3 + 2 * per_scan))):
        assert m.data.packets.dtype == np.uint8 and m.data.packets.flags.c_contiguous and m.data.packets.tobytes() == b"".join(packets[a:b])  # stride = packet size
        assert m.data.packets.size == (b - a) * size


def test_a_frame_id_that_wraps_closes_the_scan():
    packets = [_packet(ofx.LEGACY, 65535, k * C, 100 + k) for k in range(4)] + [_packet(ofx.LEGACY, 0, k * C, 200 + k) for k in range(2)]
    out, warned = _batch(packets, ofx.LEGACY)
    assert [m.data.num_packets for m in out] == [4, 2] and not warned


def test_the_cap_closes_a_scan_and_warns_once():
    cap = 2 * (W // C)
    packets = [_packet(ofx.RNG19, 3, (k * C) % W, 100 + k) for k in range(2 * cap + 5)]
    out, warned = _batch(packets)
    assert [m.data.num_packets for m in out] == [cap, cap, 5] and len(warned) == 1 and f"{cap} Ouster packets" in warned[0]
    # the cap is the CEILING of W / C
    out, warned = _batch([_packet(ofx.RNG19, 3, 0, 100 + k, c=7) for k in range(2 * 74 + 1)], C=7)
    assert [m.data.num_packets for m in out] == [2 * 74, 1] and -(-W // 7) == 74


def test_a_scan_without_a_valid_column_is_skipped_and_ts0_is_of_the_valid_columns():
    dead = [_packet(ofx.RNG19, 4, k * C, 50 + k, valid=False) for k in range(2)]
    cols = [_column(ofx.RNG19, k, 10 + k if k < 3 else 950 - k, valid=k >= 3) for k in range(C)]  # the smallest timestamps are on invalid columns
    live = [ofx.encode_packet(ofx.RNG19, cols, 5)]
    out, warned = _batch(dead + live)
    assert [m.data.num_packets for m in out] == [1] and out[0].data.ts0 == 950 - (C - 1) and out[0].time == (100, 2)
    assert len(warned) == 1 and "without a valid column" in warned[0]
    dead = [_packet(ofx.LEGACY, 4, 0, 50, valid=False)]
    assert _batch(dead, ofx.LEGACY)[0] == []


def test_other_messages_pass_through_untouched_and_in_order():
    cloud = rosbag1.Message(1, "/points", "sensor_msgs/PointCloud2", (1, 2), b"abc")
    other = rosbag1.Message(2, "/points", "std_msgs/String", (1, 3), b"def")
    out = list(lidar_messages.batch_points([cloud, other, cloud], lidar=None))
    assert out == [cloud, other, cloud] and out[0] is cloud
    packets = _messages([_packet(ofx.RNG19, 1, 0, 10), _packet(ofx.RNG19, 1, C, 20)])
    lidar = lidar_messages.LidarOptions(ouster=_info())
    out = list(lidar_messages.batch_points([cloud] + packets + [other], lidar=lidar))
    assert out[0] is cloud and out[2] is other and out[1].data.num_packets == 2
    with pytest.raises(ValueError, match="--ouster_metadata"):  # packets without the metadata
        list(lidar_messages.batch_points(packets, lidar=None))


def test_a_48_byte_buffer_is_refused_with_both_lengths():
    good = _packet(ofx.RNG19, 1, 0, 10)
    with pytest.raises(ValueError) as e:
        _batch([good, bytes(48)])
    msg = str(e.value)
    assert "message 1" in msg and "'/ouster/lidar_packets'" in msg and "48 bytes" in msg and str(len(good)) in msg and "fake.bag" in msg


# ---------------------------------------------------------------------------------------------- 5. topics and options
class _Bag:
    path = "fake.bag"

    def __init__(self, topics):
        self._topics = topics

    def topics_and_types(self):
        return self._topics


CAMERA = [("/cam/info", "sensor_msgs/CameraInfo"), ("/cam/image", "sensor_msgs/Image")]
OUSTER = [("/ouster/imu_packets", ofx.PACKET1), ("/ouster/lidar_packets", ofx.PACKET1), ("/ouster/metadata", ofx.STRING1)]


@pytest.mark.parametrize("order", [0, 1])
def test_auto_takes_the_lidar_packets_topic_by_its_name(order):
    auto = preprocess_ros1.build_parser().parse_args(["src", "dst", "-a"])
    warned = []
    topics = CAMERA + (OUSTER if order == 0 else OUSTER[::-1])
    assert preprocess_ros1.get_topics(auto, _Bag(topics), log=lambda m: None, warn=warned.append) == ("/cam/info", "/cam/image", "/ouster/lidar_packets")
    assert not warned
    # ... not beside a PointCloud2 topic
    assert preprocess_ros1.get_topics(auto, _Bag(topics + [("/points", "sensor_msgs/PointCloud2")]), log=lambda m: None, warn=warned.append)[2] == "/points"
    assert preprocess_ros1.get_topics(auto, _Bag([("/points", "sensor_msgs/PointCloud2")] + topics), log=lambda m: None, warn=warned.append)[2] == "/points"
    assert not warned
    # a PacketMsg topic of another name is not taken by -a, and is by --points_topic
    assert preprocess_ros1.get_topics(auto, _Bag(CAMERA + [("/os/packets", ofx.PACKET2)]), log=lambda m: None, warn=warned.append)[2] == ""
    named = preprocess_ros1.build_parser().parse_args(["src", "dst", "--points_topic", "/os/packets", "--image_topic", "/cam/image", "--camera_info_topic", "/cam/info"])
    assert preprocess_ros1.get_topics(named, _Bag(CAMERA + [("/os/packets", ofx.PACKET2)]), log=lambda m: None, warn=warned.append)[2] == "/os/packets"


def test_the_three_commands_take_the_options():
    for module in (preprocess_ros1, preprocess_ros2, preprocess_dynamic):
        args = module.build_parser().parse_args(["src", "dst"])
        assert (args.ouster_metadata, args.ouster_frame) == ("auto", "sensor")
        args = module.build_parser().parse_args(["src", "dst", "--ouster_metadata", "m.json", "--ouster_frame", "lidar"])
        assert (args.ouster_metadata, args.ouster_frame) == ("m.json", "lidar")


def test_ouster_options_are_ignored_with_one_line_on_another_topic(tmp_path):
    logged = []
    args = preprocess_ros1.build_parser().parse_args(["src", "dst", "--ouster_metadata", str(tmp_path / "missing.json"), "--ouster_frame", "lidar"])
    assert preprocess_ros1.lidar_options(args, _Bag([("/p", "sensor_msgs/PointCloud2")]), "/p", log=logged.append) is None
    assert len(logged) == 1 and "ignored" in logged[0] and "--ouster_metadata" in logged[0]
    quiet = preprocess_ros1.build_parser().parse_args(["src", "dst"])
    assert preprocess_ros1.lidar_options(quiet, _Bag([("/p", "sensor_msgs/PointCloud2")]), "/p", log=logged.append) is None and len(logged) == 1


def test_the_metadata_file_and_the_missing_topic(tmp_path):
    path = tmp_path / "meta.json"
    path.write_text(ofx.metadata(ofx.RNG15, H, W, 4, ALT, AZ, shape="nested"))
    args = preprocess_ros1.build_parser().parse_args(["src", "dst", "--ouster_metadata", str(path), "--ouster_frame", "lidar"])
    lidar = preprocess_ros1.lidar_options(args, _Bag(OUSTER[:2]), "/ouster/lidar_packets", log=lambda m: None)
    assert (lidar.ouster.profile_name, lidar.ouster.C, lidar.ouster.frame) == (ofx.RNG15, 4, "lidar") and lidar.model is None
    auto = preprocess_ros1.build_parser().parse_args(["src", "dst"])
    with pytest.raises(ValueError, match="--ouster_metadata FILE.json"):
        preprocess_ros1.lidar_options(auto, _Bag(OUSTER[:2]), "/ouster/lidar_packets", log=lambda m: None)


def test_header_only_needs_no_metadata():
    for cdr, pack in ((False, ofx.packet_msg_ros1), (True, ofx.packet_msg_cdr)):
        cloud = lidar_messages.decode_points(ofx.PACKET2 if cdr else ofx.PACKET1, pack(_packet(ofx.RNG19, 1, 0, 10)), cdr=cdr, header_only=True)
        assert [(f.name, f.offset, f.datatype) for f in cloud.fields] == [("x", 0, 7), ("y", 4, 7), ("z", 8, 7), ("intensity", 12, 7), ("t", 16, 6), ("reflectivity", 20, 4),
                                                                          ("ring", 22, 4), ("ambient", 24, 4), ("range", 28, 6)]
        assert cloud.point_step == 32 and cloud.height == 1 and cloud.width == 0


# ---------------------------------------------------------------------------------------------- 6. the restatement against the formulas
def _one_pixel(profile, m, range_mm, altitude=0.0, azimuth=0.0, n_mm=0.0, transform=oo.IDENTITY12, w=W, ts=1000, ts0=1000):
    """A 16-beam sensor whose beam 0 has the given angles; one column alone in a packet, its pixel 0 at ``range_mm``"""
    raw = range_mm >> 3 if profile == ofx.RNG15 else range_mm
    col = ofx.Column(ts, m, ofx.VALID[profile], [raw] + [0] * 15, [77] + [0] * 15, [1234] + [0] * 15, [5] + [0] * 15)
    packet = np.frombuffer(ofx.encode_packet(profile, [col], 1), dtype=np.uint8)
    rec, returns = oo.decode(packet, len(packet), 1, profile, 16, w, 1, oo.column_table(w), oo.beam_table([azimuth] + [0.0] * 15, [altitude] + [0.0] * 15), n_mm, transform, ts0)
    assert returns.tolist() == [1] and np.isnan(rec["x"][1:]).all() and rec["ring"].tolist() == list(range(16))
    return rec[0]


@pytest.mark.parametrize("profile", [ofx.LEGACY, ofx.RNG19, ofx.RNG15])
def test_the_oracle_on_pixels_one_can_compute_by_hand(profile):
    # beam on the axis, column 0: E = 2 pi, the beam looks along +x; 8000 mm
    r = _one_pixel(profile, 0, 8000)
    assert r["x"] == np.float32(8.0) and abs(r["y"]) < 1e-14 and r["z"] == 0.0 and r["range"] == 8000 and r["t"] == 0
    assert r["reflectivity"] == 77 and r["ambient"] == (5 << 4 if profile == ofx.RNG15 else 5) and r["intensity"] == (0.0 if profile == ofx.RNG15 else 1234.0)
    # column W / 4: E = 3 pi / 2, the encoder counts against the azimuth: the beam looks along -y
    r = _one_pixel(profile, W // 4, 8000)
    assert abs(r["x"]) < 1e-14 and r["y"] == np.float32(-8.0) and r["z"] == 0.0
    # column W / 2: along -x
    r = _one_pixel(profile, W // 2, 8000)
    assert r["x"] == np.float32(-8.0) and abs(r["y"]) < 1e-14
    # the OS1 transform turns x and y around and lifts z by 36.18 mm
    r = _one_pixel(profile, 0, 8000, transform=ofx.OS1_TRANSFORM[:12])
    assert r["x"] == np.float32(-8.0) and abs(r["y"]) < 1e-14 and r["z"] == np.float32(36.18 * 0.001)
    r = _one_pixel(profile, W // 4, 8000, transform=ofx.OS1_TRANSFORM[:12])
    assert abs(r["x"]) < 1e-14 and r["y"] == np.float32(8.0) and r["z"] == np.float32(36.18 * 0.001)
    # altitude 30 degrees: z = r / 2 and x = r sqrt(3) / 2; with the beam origin n off the axis, r - n of it along the beam
    r = _one_pixel(profile, 0, 8000, altitude=30.0)
    assert abs(float(r["z"]) - 4.0) < 1e-6 and abs(float(r["x"]) - 8.0 * math.sqrt(3.0) / 2.0) < 1e-6
    r = _one_pixel(profile, 0, 8000, altitude=30.0, n_mm=16.0)
    assert abs(float(r["z"]) - 7.984 / 2.0) < 1e-6 and abs(float(r["x"]) - (7.984 * math.sqrt(3.0) / 2.0 + 0.016)) < 1e-6
    # azimuth +90 degrees at column 0: A = -90 degrees, the beam looks along -y
    r = _one_pixel(profile, 0, 8000, azimuth=90.0)
    assert abs(r["x"]) < 1e-14 and r["y"] == np.float32(-8.0)
    # a permutation with distinct offsets: x <- lz + 1 mm, y <- lx + 2 mm, z <- ly + 3 mm
    r = _one_pixel(profile, 0, 8000, transform=(0, 0, 1, 1, 1, 0, 0, 2, 0, 1, 0, 3))
    assert r["x"] == np.float32(0.001) and r["y"] == np.float32(8.002) and abs(float(r["z"]) - 0.003) < 1e-9
    # the time: nanoseconds behind ts0, clamped
    assert _one_pixel(profile, 0, 8000, ts=5000, ts0=1000)["t"] == 4000
    assert _one_pixel(profile, 0, 8000, ts=1000 + 2**32 + 5, ts0=1000)["t"] == 2**32 - 1
