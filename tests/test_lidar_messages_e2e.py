"""End-to-end GPU tests of the VelodyneScan / CustomMsg route: a bag recorded as raw Velodyne packets, or as Livox CustomMsg, must come
out of preprocess_ros1, preprocess_ros2 and preprocess_dynamic as the SAME BYTES as a bag that holds, on the same topic name, the
PointCloud2 messages the vendor driver would have published: for the packets the 20-byte records of tests/velodyne_oracle.py, for
CustomMsg the message's own 19-byte points.  The PointCloud2 route is held to its oracle by tests/test_preprocess_ros1_gpu.py,
tests/test_preprocess_ros2_gpu.py and tests/test_odometry_gpu.py, whose room and trajectory this scene is."""
import filecmp
import json
import os

import numpy as np
import pytest

import lidar_message_fixture as lfx
import rosbag1_fixture as fx1
import rosbag2_fixture as fx2
import velodyne_oracle as vo
from direct_visual_lidar_calibration_amd import preprocess_dynamic, preprocess_ros1, preprocess_ros2
from test_odometry_gpu import ARGS, cast, true_pose
from test_preprocess_ros2_gpu import SUFFIXES

pytestmark = pytest.mark.gpu

MESSAGES, PACKETS, STEP = 4, 8, 187  # 8 packets x 24 firings, 1.87 degrees apart: one turn a message
SCAN = 0.1
PACKET_NS = 12500000
VELODYNE_FIELDS = [("x", 0, 7, 1), ("y", 4, 7, 1), ("z", 8, 7, 1), ("intensity", 12, 7, 1), ("time", 16, 7, 1)]
IMAGE = np.random.default_rng(3).integers(0, 256, size=(48, 64)).astype(np.uint8)
CAMERA_ARGS = [a for a in ARGS if a not in ("--image_topic", "/camera/image", "--points_topic", "/points")]


def _rays(az_centideg, elevation_deg):
    """Unit directions in the sensor's ROS frame: azimuth clockwise from +x"""
    a, w = np.radians(np.asarray(az_centideg) / 100.0), np.radians(elevation_deg)
    return np.stack([np.cos(w) * np.cos(a), -np.cos(w) * np.sin(a), np.sin(w)], axis=1)


def _velodyne_messages():
    """Per message ``(header stamp, [(packet stamp, 1206 bytes)])``: a VLP-16 carried through the room of tests/test_odometry_gpu.py, every
    packet cast from where the sensor is at its stamp; a few returns are lost (raw distance 0)"""
    elevation = np.array([vo.vlp16_elevation_deg(l) for l in range(16)])
    out = []
    for m in range(MESSAGES):
        packets = []
        for p in range(PACKETS):
            T = true_pose(m * SCAN + p * PACKET_NS * 1e-9)
            azimuths = [((p * 12 + b) * 2 * STEP) % 36000 for b in range(12)]
            dist = np.zeros((12, 32), dtype=np.int64)
            refl = np.zeros((12, 32), dtype=np.int64)
            for b in range(12):
                for f in range(2):
                    d = _rays([(azimuths[b] + f * STEP) % 36000] * 16, elevation)
                    r = cast(np.tile(T[:3, 3], (16, 1)), d @ T[:3, :3].T)
                    dist[b, 16 * f : 16 * f + 16] = np.clip(np.rint(r / 0.002), 1, 65535)
                    refl[b, 16 * f : 16 * f + 16] = np.clip(60 + 10 * np.arange(16) + 50 * np.sin(np.radians(azimuths[b] / 100.0)), 0, 255).astype(np.int64)
            dist[(m + p) % 12, (3 * p) % 32] = 0
            ns = m * 100000000 + p * PACKET_NS
            packets.append(((100, ns), vo.encode_packet(azimuths, dist, refl)))
        out.append(((100, m * 100000000), packets))
    return out


def _oracle_records(packets):
    """What the vendor driver would publish for the message: the oracle's records, packet times relative to the first packet's stamp"""
    _, view = vo.place_packets([data for _, data in packets], 1206)
    s0, n0 = packets[0][0]
    times = [float((s - s0) * 1000000000 + (n - n0)) * 1e-9 for (s, n), _ in packets]
    rec, _ = vo.decode(view, 1206, times, *vo.model("vlp16"))
    return rec.tobytes()


def _livox_messages():
    """Per message ``(header stamp, CUSTOM_POINT array)``: a non-repetitive pattern in the same room, from a sensor at rest"""
    out = []
    for m in range(MESSAGES):
        rng = np.random.default_rng(40 + m)
        n = 3000
        az, el = rng.uniform(-35.0, 35.0, n), rng.uniform(-30.0, 35.0, n)
        d = _rays(az * 100.0, el)
        r = cast(np.zeros((n, 3)), d)
        pts = np.zeros(n, dtype=lfx.CUSTOM_POINT)
        pts["t"] = (np.arange(n) * (100000000 // n)).astype(np.uint32)
        pts["x"], pts["y"], pts["z"] = (d * r[:, None]).T
        pts["reflectivity"], pts["tag"], pts["line"] = rng.integers(0, 256, n), rng.integers(0, 64, n), rng.integers(0, 6, n)
        pts["x"][5 + m] = np.nan
        out.append(((100, m * 100000000), pts))
    return out


def _write(root, kind, name, points_type, point_messages, extra=None):
    """One bag ``name`` of storage ``kind`` under ``root / kind``: the image on /camera/image and the serialised point messages ``(stamp,
    payload)`` on /points; ``extra``: a second points topic ``(topic, type, messages)``"""
    os.makedirs(root / kind, exist_ok=True)
    ros1 = kind == "ros1"
    image = (fx1 if ros1 else fx2).image((50, 0), IMAGE, "mono8")
    topics = [("/camera/image", "sensor_msgs/Image" if ros1 else fx2.IMG), ("/points", points_type)] + ([extra[:2]] if extra else [])
    msgs = [(0, (50, 0), image)] + [(1, stamp, payload) for stamp, payload in point_messages] + ([(2, stamp, payload) for stamp, payload in extra[2]] if extra else [])
    msgs.sort(key=lambda m: m[1])
    if ros1:
        fx1.write_bag(root / kind / (name + ".bag"), [(k, t, ty) for k, (t, ty) in enumerate(topics)], msgs, chunk_size=3, index=True)
    elif kind == "sqlite3":
        fx2.write_sqlite3_dir(root / kind / name, [(k + 1, t, ty) for k, (t, ty) in enumerate(topics)], [(c + 1, fx2.nanoseconds(s), p) for c, s, p in msgs])
    else:
        fx2.write_mcap(root / kind / (name + ".mcap"), [(k + 1, t, ty) for k, (t, ty) in enumerate(topics)], [(c + 1, fx2.nanoseconds(s), p) for c, s, p in msgs], chunk_size=2)
    return {"ros1": name + ".bag", "sqlite3": name, "mcap": name + ".mcap"}[kind]


def _assert_same_directory(got_dir, want_dir, bag_name):
    for suffix in SUFFIXES:
        assert filecmp.cmp(os.path.join(got_dir, bag_name + suffix), os.path.join(want_dir, bag_name + suffix), shallow=False), suffix
    with open(os.path.join(got_dir, "calib.json")) as f, open(os.path.join(want_dir, "calib.json")) as g:
        got, ref = json.load(f), json.load(g)
    assert got["meta"].pop("data_path") != ref["meta"].pop("data_path")
    assert got == ref and got["meta"]["points_topic"] == "/points"
    assert sorted(os.listdir(got_dir)) == sorted(os.listdir(want_dir)) == sorted([bag_name + s for s in SUFFIXES] + ["calib.json"])
    return got


@pytest.fixture(scope="module")
def velodyne():
    messages = _velodyne_messages()
    return messages, [(stamp, _oracle_records(packets)) for stamp, packets in messages]


def _scan_payloads(messages, kind):
    if kind == "ros1":
        return lfx.SCAN1, [(stamp, lfx.velodyne_scan_ros1(stamp, packets)) for stamp, packets in messages]
    return lfx.SCAN2, [(stamp, lfx.velodyne_scan_cdr(stamp, packets, final_padding=k % 2 == 0)) for k, (stamp, packets) in enumerate(messages)]


def _cloud_payloads(records, kind, fields=VELODYNE_FIELDS, step=20):
    if kind == "ros1":
        return "sensor_msgs/PointCloud2", [(stamp, fx1.pointcloud2(stamp, fields, step, rec)) for stamp, rec in records]
    return fx2.PC2, [(stamp, fx2.pointcloud2(stamp, fields, step, rec)) for stamp, rec in records]


COMMANDS = {"ros1": preprocess_ros1, "sqlite3": preprocess_ros2, "mcap": preprocess_ros2}


@pytest.mark.parametrize("kind", ["ros1", "sqlite3", "mcap"])
def test_velodyne_scan_bag_equals_the_pointcloud2_bag_byte_for_byte(velodyne, tmp_path, capsys, kind):
    messages, records = velodyne
    name = _write(tmp_path / "packets", kind, "run", *_scan_payloads(messages, kind))
    assert _write(tmp_path / "clouds", kind, "run", *_cloud_payloads(records, kind)) == name
    got, want = str(tmp_path / "got"), str(tmp_path / "want")
    assert COMMANDS[kind].main([str(tmp_path / "packets" / kind), got, "--points_topic", "/points", "--image_topic", "/camera/image"] + CAMERA_ARGS) == 0
    out = capsys.readouterr().out
    assert "intensity_channel: intensity" in out and f"frames={MESSAGES} skipped_frames=0 skipped_points={MESSAGES * PACKETS}" in out
    assert COMMANDS[kind].main([str(tmp_path / "clouds" / kind), want, "--points_topic", "/points", "--image_topic", "/camera/image"] + CAMERA_ARGS) == 0
    assert f"frames={MESSAGES} skipped_frames=0 skipped_points={MESSAGES * PACKETS}" in capsys.readouterr().out
    _assert_same_directory(got, want, name)


@pytest.mark.parametrize("kind", ["ros1", "mcap"])
def test_velodyne_scan_bag_through_the_dynamic_integrator(velodyne, tmp_path, kind):
    messages, records = velodyne
    name = _write(tmp_path / "packets", kind, "run", *_scan_payloads(messages, kind))
    _write(tmp_path / "clouds", kind, "run", *_cloud_payloads(records, kind))
    command, flag = (preprocess_dynamic, []) if kind == "ros1" else (preprocess_ros2, ["-d"])
    got, want = str(tmp_path / "got"), str(tmp_path / "want")
    assert command.main([str(tmp_path / "packets" / kind), got, "-a", "--target_num_points", "1000", "--lidar_model", "vlp16"] + flag + CAMERA_ARGS) == 0
    assert command.main([str(tmp_path / "clouds" / kind), want, "-a", "--target_num_points", "1000"] + flag + CAMERA_ARGS) == 0
    _assert_same_directory(got, want, name)
    # the time field did deskew: the static route smears the same packets
    static = str(tmp_path / "static")
    assert COMMANDS[kind].main([str(tmp_path / "packets" / kind), static, "-a"] + CAMERA_ARGS) == 0
    assert not filecmp.cmp(os.path.join(static, name + ".ply"), os.path.join(got, name + ".ply"), shallow=False)


@pytest.mark.parametrize("kind", ["ros1", "sqlite3"])
def test_custom_msg_bag_equals_the_pointcloud2_bag_byte_for_byte(tmp_path, capsys, kind):
    messages = _livox_messages()
    fields = [("t", 0, 6, 1), ("x", 4, 7, 1), ("y", 8, 7, 1), ("z", 12, 7, 1), ("reflectivity", 16, 2, 1), ("tag", 17, 2, 1), ("line", 18, 2, 1)]
    if kind == "ros1":
        type_, payloads = lfx.LIVOX1, [(stamp, lfx.custom_msg_ros1(stamp, pts, timebase=1700000000000000000 + k)) for k, (stamp, pts) in enumerate(messages)]
    else:
        type_, payloads = lfx.LIVOX2, [(stamp, lfx.custom_msg_cdr(stamp, pts, timebase=1700000000000000000 + k, final_padding=k % 2 == 0)) for k, (stamp, pts) in enumerate(messages)]
    name = _write(tmp_path / "livox", kind, "run", type_, payloads)
    _write(tmp_path / "clouds", kind, "run", *_cloud_payloads([(stamp, pts.tobytes()) for stamp, pts in messages], kind, fields=fields, step=19))
    got, want = str(tmp_path / "got"), str(tmp_path / "want")
    assert COMMANDS[kind].main([str(tmp_path / "livox" / kind), got, "-a", "--lidar_model", "hdl32e"] + CAMERA_ARGS) == 0
    out = capsys.readouterr().out
    assert "intensity_channel: reflectivity" in out and f"frames={MESSAGES} skipped_frames=0 skipped_points={MESSAGES}" in out
    assert out.count("--lidar_model and --velodyne_calibration are ignored") == 1
    assert COMMANDS[kind].main([str(tmp_path / "clouds" / kind), want, "-a"] + CAMERA_ARGS) == 0
    _assert_same_directory(got, want, name)


def test_a_bag_with_both_topics_takes_the_pointcloud2_route_under_auto(velodyne, tmp_path, capsys):
    """/points (PointCloud2) next to /velodyne_packets (VelodyneScan, of OTHER packets: its cloud would differ): the output of -a is
    what the bag gives without the packets topic, i.e. what it gave before VelodyneScan topics were read"""
    messages, records = velodyne
    other = [(stamp, [(t, vo.encode_packet([0] * 12, np.full((12, 32), 2500), np.full((12, 32), 9))) for t, _ in packets]) for stamp, packets in messages]
    type_, clouds = _cloud_payloads(records, "ros1")
    name = _write(tmp_path / "both", "ros1", "run", type_, clouds, extra=("/velodyne_packets", lfx.SCAN1, _scan_payloads(other, "ros1")[1]))
    _write(tmp_path / "clouds", "ros1", "run", type_, clouds)
    got, want = str(tmp_path / "got"), str(tmp_path / "want")
    assert preprocess_ros1.main([str(tmp_path / "both" / "ros1"), got, "-a"] + CAMERA_ARGS) == 0
    captured = capsys.readouterr()
    assert "- points     : /points" in captured.out and "multiple points topics" not in captured.err
    assert preprocess_ros1.main([str(tmp_path / "clouds" / "ros1"), want, "-a"] + CAMERA_ARGS) == 0
    _assert_same_directory(got, want, name)
