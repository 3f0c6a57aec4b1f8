"""End-to-end GPU tests of the Ouster PacketMsg route: a bag recorded as raw lidar packets with the sensor's metadata topic (and the IMU
packets, which have the same type) must come out of preprocess_ros1, preprocess_ros2 and preprocess_dynamic as the SAME BYTES as a bag
that holds, on the same topic name, one PointCloud2 message per scan with the 32-byte records of tests/ouster_oracle.py.  The PointCloud2
route is held to its oracle by tests/test_preprocess_ros1_gpu.py, tests/test_preprocess_ros2_gpu.py and tests/test_odometry_gpu.py, whose
room and trajectory this scene is."""
import filecmp
import json
import os

import numpy as np
import pytest

import ouster_fixture as ofx
import ouster_oracle as oo
import rosbag1_fixture as fx1
import rosbag2_fixture as fx2
from direct_visual_lidar_calibration_amd import preprocess_dynamic, preprocess_ros1, preprocess_ros2
from test_odometry_gpu import ARGS, cast, true_pose
from test_preprocess_ros2_gpu import SUFFIXES

pytestmark = pytest.mark.gpu

PROFILE, H, W, C = ofx.RNG19, 16, 512, 16
SCANS, SCAN_NS, COLUMN_NS = 4, 100000000, 195312
EPOCH = 100  # seconds
TOPIC = "/ouster/lidar_packets"
ALT, AZ = ofx.os_angles(H)
N_MM = 15.806
LOST = [(40, 3), (200, 0), (333, 15)]  # per scan: pixels without a return
FIELDS = [("x", 0, 7, 1), ("y", 4, 7, 1), ("z", 8, 7, 1), ("intensity", 12, 7, 1), ("t", 16, 6, 1), ("reflectivity", 20, 4, 1), ("ring", 22, 4, 1), ("ambient", 24, 4, 1), ("range", 28, 6, 1)]
IMAGE = np.random.default_rng(3).integers(0, 256, size=(48, 64)).astype(np.uint8)
CAMERA_ARGS = [a for a in ARGS if a not in ("--image_topic", "/camera/image", "--points_topic", "/points")]
COMMANDS = {"ros1": preprocess_ros1, "sqlite3": preprocess_ros2, "mcap": preprocess_ros2}
R_SENSOR = np.array(ofx.OS1_TRANSFORM).reshape(4, 4)[:3, :3]


def _stamp(ns):
    return (EPOCH + ns // 1000000000, ns % 1000000000)


def _scene():
    """Per scan ``(first column's time [ns behind the epoch], packets)``: an OS1-16 carried through the room of tests/test_odometry_gpu.py,
    every column cast from where the sensor is at its time; the first scan starts half way round"""
    scans = []
    for s in range(SCANS):
        def range_mm(m, t_ns):
            T = true_pose((t_ns - EPOCH * 1000000000) * 1e-9)
            d = ofx.beam_directions(m, W, ALT, AZ) @ R_SENSOR.T
            return np.rint(cast(np.tile(T[:3, 3], (H, 1)), d @ T[:3, :3].T) * 1000.0)

        first = W // 2 if s == 0 else 0
        packets = ofx.scan_packets(PROFILE, H, W, C, 700 + s, EPOCH * 1000000000 + s * SCAN_NS, COLUMN_NS, range_mm, first_column=first, lost=LOST)
        scans.append((s * SCAN_NS + first * COLUMN_NS, packets))
    return scans


def _oracle_cloud(packets):
    """What the decode makes of the scan: ``(stamp, record bytes)``"""
    size = oo.packet_size(PROFILE, H, C)
    _, view = ofx.place_packets(packets, size)
    ts0 = oo.first_valid_timestamp(view, size, len(packets), PROFILE, H, C)
    rec, _ = oo.decode(view, size, len(packets), PROFILE, H, W, C, oo.column_table(W), oo.beam_table(AZ, ALT), N_MM, ofx.OS1_TRANSFORM[:12], ts0)
    return (ts0 // 1000000000, ts0 % 1000000000), rec.tobytes()


@pytest.fixture(scope="module")
def scene():
    scans = _scene()
    return scans, [_oracle_cloud(packets) for _, packets in scans]


def _write(root, kind, name, topics, messages):
    """One bag ``name`` of storage ``kind`` under ``root / kind``: ``topics`` [(topic, type)], ``messages`` [(topic index, stamp, payload)]"""
    os.makedirs(root / kind, exist_ok=True)
    messages = sorted(messages, key=lambda m: m[1])
    if kind == "ros1":
        fx1.write_bag(root / kind / (name + ".bag"), [(k, t, ty) for k, (t, ty) in enumerate(topics)], messages, chunk_size=5, index=True)
    elif kind == "sqlite3":
        fx2.write_sqlite3_dir(root / kind / name, [(k + 1, t, ty) for k, (t, ty) in enumerate(topics)], [(c + 1, fx2.nanoseconds(s), p) for c, s, p in messages])
    else:
        fx2.write_mcap(root / kind / (name + ".mcap"), [(k + 1, t, ty) for k, (t, ty) in enumerate(topics)], [(c + 1, fx2.nanoseconds(s), p) for c, s, p in messages], chunk_size=7)
    return {"ros1": name + ".bag", "sqlite3": name, "mcap": name + ".mcap"}[kind]


def _image(kind):
    return ("/camera/image", "sensor_msgs/Image" if kind == "ros1" else fx2.IMG), (fx1 if kind == "ros1" else fx2).image((50, 0), IMAGE, "mono8")


def _packets_bag(root, kind, scans, metadata=True):
    """/camera/image, the lidar packets, the IMU packets (48 bytes, between the lidar packets) and, latched before them, the metadata"""
    ros1 = kind == "ros1"
    packet_type = ofx.PACKET1 if ros1 else ofx.PACKET2 if kind == "sqlite3" else ofx.PACKET2_SENSOR
    pack, string = (ofx.packet_msg_ros1, ofx.string_ros1) if ros1 else (ofx.packet_msg_cdr, ofx.string_cdr)
    image_topic, image = _image(kind)
    topics = [image_topic, ("/ouster/imu_packets", packet_type), (TOPIC, packet_type)] + ([("/ouster/metadata", ofx.STRING1 if ros1 else ofx.STRING2)] if metadata else [])
    messages = [(0, (50, 0), image)]
    if metadata:
        messages.append((3, (60, 0), string(ofx.metadata(PROFILE, H, W, C, ALT, AZ, N_MM, shape="flat" if ros1 else "nested"))))
    for start, packets in scans:
        for k, p in enumerate(packets):
            messages.append((2, _stamp(start + k * C * COLUMN_NS), pack(p)))
            messages.append((1, _stamp(start + k * C * COLUMN_NS + 1000), pack(bytes(48))))
    return _write(root, kind, "run", topics, messages)


def _clouds_bag(root, kind, clouds):
    ros1 = kind == "ros1"
    image_topic, image = _image(kind)
    make = fx1.pointcloud2 if ros1 else fx2.pointcloud2
    messages = [(0, (50, 0), image)] + [(1, stamp, make(stamp, FIELDS, 32, rec)) for stamp, rec in clouds]
    return _write(root, kind, "run", [image_topic, (TOPIC, "sensor_msgs/PointCloud2" if ros1 else fx2.PC2)], messages)


def _assert_same_directory(got_dir, want_dir, bag_name):
    for suffix in SUFFIXES:
        assert filecmp.cmp(os.path.join(got_dir, bag_name + suffix), os.path.join(want_dir, bag_name + suffix), shallow=False), suffix
    with open(os.path.join(got_dir, "calib.json")) as f, open(os.path.join(want_dir, "calib.json")) as g:
        got, ref = json.load(f), json.load(g)
    got["meta"].pop("data_path"), ref["meta"].pop("data_path")
    assert got == ref and got["meta"]["points_topic"] == TOPIC and got["meta"]["intensity_channel"] == "reflectivity"
    assert sorted(os.listdir(got_dir)) == sorted(os.listdir(want_dir)) == sorted([bag_name + s for s in SUFFIXES] + ["calib.json"])


@pytest.mark.parametrize("kind", ["ros1", "sqlite3", "mcap"])
def test_packet_bag_equals_the_pointcloud2_bag_byte_for_byte(scene, tmp_path, capsys, kind):
    scans, clouds = scene
    name = _packets_bag(tmp_path / "packets", kind, scans)
    assert _clouds_bag(tmp_path / "clouds", kind, clouds) == name
    got, want = str(tmp_path / "got"), str(tmp_path / "want")
    assert COMMANDS[kind].main([str(tmp_path / "packets" / kind), got, "-a"] + CAMERA_ARGS) == 0
    out = capsys.readouterr().out
    assert f"- points     : {TOPIC}" in out and "intensity_channel: reflectivity" in out
    assert f"frames={SCANS} skipped_frames=0 skipped_points={SCANS * len(LOST) - 2}" in out  # (columns 40 and 200 are not in the first, partial scan)
    assert COMMANDS[kind].main([str(tmp_path / "clouds" / kind), want, "-a"] + CAMERA_ARGS) == 0
    assert f"frames={SCANS} skipped_frames=0 skipped_points={SCANS * len(LOST) - 2}" in capsys.readouterr().out
    _assert_same_directory(got, want, name)


def test_packet_bag_through_the_dynamic_integrator(scene, tmp_path):
    scans, clouds = scene
    name = _packets_bag(tmp_path / "packets", "ros1", scans)
    _clouds_bag(tmp_path / "clouds", "ros1", clouds)
    got, want = str(tmp_path / "got"), str(tmp_path / "want")
    assert preprocess_dynamic.main([str(tmp_path / "packets" / "ros1"), got, "-a", "--target_num_points", "1000"] + CAMERA_ARGS) == 0
    assert preprocess_dynamic.main([str(tmp_path / "clouds" / "ros1"), want, "-a", "--target_num_points", "1000"] + CAMERA_ARGS) == 0
    _assert_same_directory(got, want, name)
    # the t field did deskew: the static route smears the same packets
    static = str(tmp_path / "static")
    assert preprocess_ros1.main([str(tmp_path / "packets" / "ros1"), static, "-a"] + CAMERA_ARGS) == 0
    assert not filecmp.cmp(os.path.join(static, name + ".ply"), os.path.join(got, name + ".ply"), shallow=False)


def test_the_metadata_file_equals_auto_and_its_absence_names_the_option(scene, tmp_path, capsys):
    scans, _ = scene
    name = _packets_bag(tmp_path / "with", "ros1", scans)
    assert _packets_bag(tmp_path / "without", "ros1", scans, metadata=False) == name
    path = tmp_path / "os1.json"
    path.write_text(ofx.metadata(PROFILE, H, W, C, ALT, AZ, N_MM, shape="nested"))
    auto, named, lidar_frame = str(tmp_path / "auto"), str(tmp_path / "named"), str(tmp_path / "lidar_frame")
    assert preprocess_ros1.main([str(tmp_path / "with" / "ros1"), auto, "-a"] + CAMERA_ARGS) == 0
    assert preprocess_ros1.main([str(tmp_path / "without" / "ros1"), named, "--points_topic", TOPIC, "--image_topic", "/camera/image", "--ouster_metadata", str(path)] + CAMERA_ARGS) == 0
    _assert_same_directory(named, auto, name)
    capsys.readouterr()
    assert preprocess_ros1.main([str(tmp_path / "without" / "ros1"), str(tmp_path / "none"), "-a"] + CAMERA_ARGS) == 1
    err = capsys.readouterr().err
    assert "--ouster_metadata" in err and TOPIC in err and not os.path.exists(tmp_path / "none" / "calib.json")
    # the IMU topic, named as the points topic, is refused with both lengths
    assert preprocess_ros1.main([str(tmp_path / "with" / "ros1"), str(tmp_path / "imu"), "--points_topic", "/ouster/imu_packets", "--image_topic", "/camera/image"] + CAMERA_ARGS) == 1
    err = capsys.readouterr().err
    assert "48 bytes" in err and str(oo.packet_size(PROFILE, H, C)) in err and "/ouster/imu_packets" in err
    # --ouster_frame lidar is another cloud: x and y turned around, z lower by 36.18 mm
    assert preprocess_ros1.main([str(tmp_path / "with" / "ros1"), lidar_frame, "-a", "--ouster_frame", "lidar"] + CAMERA_ARGS) == 0
    assert not filecmp.cmp(os.path.join(lidar_frame, name + ".ply"), os.path.join(auto, name + ".ply"), shallow=False)
