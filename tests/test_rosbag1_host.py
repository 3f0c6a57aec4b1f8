"""CPU tests of the ROS1 bag reader (rosbag1.py), of the time keeper and of the host logic of the preprocess_ros1 command line.  The
bags come from tests/rosbag1_fixture.py, a writer that shares no code with the reader, and from bytes spelled out below."""
import struct
import types

import numpy as np
import pytest

import rosbag1_fixture as fx
from direct_visual_lidar_calibration_amd import dataset, preprocess, preprocess_ros1, rosbag1

PC2, IMG, CIMG, INFO = "sensor_msgs/PointCloud2", "sensor_msgs/Image", "sensor_msgs/CompressedImage", "sensor_msgs/CameraInfo"


def _payloads(bag, topic=None):
    return [(m.conn, m.time, bytes(m.data)) for m in bag.messages(topic)]


def test_a_hand_packed_minimal_bag(tmp_path):
    """Every byte of the bag is written out here: the magic, a bag header record padded to 4096 bytes, one connection and one
    message record outside any chunk."""
    bag_header = (
        b"\x45\x00\x00\x00"  # header_len = 69
        b"\x04\x00\x00\x00op=\x03"
        b"\x12\x00\x00\x00index_pos=\x00\x00\x00\x00\x00\x00\x00\x00"
        b"\x0f\x00\x00\x00conn_count=\x01\x00\x00\x00"
        b"\x10\x00\x00\x00chunk_count=\x00\x00\x00\x00"
    )
    assert len(bag_header) == 4 + 69
    pad = 4096 - len(bag_header) - 4
    bag_header += struct.pack("<I", pad) + b" " * pad
    conn_data = b"\x0b\x00\x00\x00topic=/chat" b"\x14\x00\x00\x00type=std_msgs/String" b"\x0b\x00\x00\x00md5sum=992c" b"\x17\x00\x00\x00message_definition=data"
    conn = b"\x24\x00\x00\x00" b"\x04\x00\x00\x00op=\x07" b"\x09\x00\x00\x00conn=\x05\x00\x00\x00" b"\x0b\x00\x00\x00topic=/chat" + struct.pack("<I", len(conn_data)) + conn_data
    payload = b"\x02\x00\x00\x00hi"
    msg = b"\x26\x00\x00\x00" b"\x04\x00\x00\x00op=\x02" b"\x09\x00\x00\x00conn=\x05\x00\x00\x00" b"\x0d\x00\x00\x00time=\x0a\x00\x00\x00\x07\x00\x00\x00" + b"\x06\x00\x00\x00" + payload
    path = tmp_path / "hand.bag"
    path.write_bytes(b"#ROSBAG V2.0\n" + bag_header + conn + msg)
    assert len(b"#ROSBAG V2.0\n" + bag_header) == 4096 + 13
    bag = rosbag1.Bag(path)
    assert (bag.index_pos, bag.conn_count, bag.chunk_count) == (0, 1, 0)
    assert bag.connections == {5: rosbag1.Connection(5, "/chat", "std_msgs/String", "992c", "data")}
    assert _payloads(bag) == [(5, (10, 7), payload)]
    assert rosbag1.topics_and_types(path) == [("/chat", "std_msgs/String")]


def _three_topic_bag(path, **kw):
    conns = [(0, "/points", PC2), (1, "/image", IMG), (2, "/info", INFO)]
    msgs = [(k % 3, (100 + k, 5 * k), bytes([k]) * (k + 1)) for k in range(8)]
    return conns, msgs, fx.write_bag(path, conns, msgs, **kw)


@pytest.mark.parametrize("kw", [dict(compression="none"), dict(compression="bz2"), dict(outside=True), dict(compression="none", index=True), dict(compression="bz2", index=True, chunk_size=1)],
                         ids=["none", "bz2", "outside_chunks", "indexed", "bz2_indexed"])
def test_chunked_compressed_indexed_and_bare_bags_parse_alike(tmp_path, kw):
    path = tmp_path / "a.bag"
    conns, msgs, _ = _three_topic_bag(path, **kw)
    bag = rosbag1.Bag(path)
    assert bag.topics_and_types() == [(c[1], c[2]) for c in conns]
    assert _payloads(bag) == msgs
    assert _payloads(bag, "/image") == [m for m in msgs if m[0] == 1]
    assert (bag.index_pos > 0) == bool(kw.get("index"))


def test_an_lz4_chunk_decodes_or_names_the_compression(tmp_path):
    inner = fx.connection_record(0, "/points", PC2) + fx.message_record(0, (1, 2), b"abc")
    try:
        import lz4.frame
    except ImportError:
        lz4 = None
    else:
        import lz4
    data = inner if lz4 is None else lz4.frame.compress(inner)
    path = tmp_path / "lz4.bag"
    path.write_bytes(fx.MAGIC + fx.bag_header_record(0, 1, 1) + fx.chunk_record(inner, "lz4", compressed=data))
    if lz4 is None:
        with pytest.raises(ValueError, match="lz4"):
            rosbag1.Bag(path)
    else:
        assert _payloads(rosbag1.Bag(path)) == [(0, (1, 2), b"abc")]
    path.write_bytes(fx.MAGIC + fx.bag_header_record(0, 1, 1) + fx.chunk_record(inner, "zstd", compressed=inner))
    with pytest.raises(ValueError, match="zstd"):
        rosbag1.Bag(path)


def test_messages_come_by_time_then_file_order(tmp_path):
    conns = [(0, "/points", PC2)]
    times = [(5, 0), (3, 9), (3, 9), (4, 0), (3, 8), (5, 0), (2, 999999999), (3, 9)]
    msgs = [(0, t, bytes([k])) for k, t in enumerate(times)]
    want = [msgs[k] for k in sorted(range(len(msgs)), key=lambda k: (times[k], k))]
    assert [m[2][0] for m in want] == [6, 4, 1, 2, 7, 3, 0, 5]
    for kw in (dict(chunk_size=3), dict(outside=True), dict(compression="bz2", chunk_size=2)):
        path = tmp_path / "t.bag"
        fx.write_bag(path, conns, msgs, **kw)
        assert _payloads(rosbag1.Bag(path), "/points") == want


def test_two_connections_on_one_topic(tmp_path):
    conns = [(0, "/points", PC2), (3, "/points", PC2), (1, "/image", IMG)]
    msgs = [(3, (9, 0), b"c"), (0, (7, 0), b"a"), (1, (7, 5), b"i"), (3, (8, 0), b"b")]
    path = tmp_path / "two.bag"
    fx.write_bag(path, conns, msgs)
    bag = rosbag1.Bag(path)
    assert bag.topics_and_types() == [("/points", PC2), ("/image", IMG), ("/points", PC2)]  # connection-id order
    assert _payloads(bag, "/points") == [(0, (7, 0), b"a"), (3, (8, 0), b"b"), (3, (9, 0), b"c")]


@pytest.mark.parametrize("kw", [dict(outside=True), dict(compression="none", index=True, chunk_size=3)], ids=["outside_chunks", "indexed"])
def test_truncation_next_to_every_record_boundary_is_refused_with_the_offset(tmp_path, kw):
    path = tmp_path / "full.bag"
    _, _, bounds = _three_topic_bag(path, **kw)
    raw = path.read_bytes()
    assert bounds[-1] == len(raw) and bounds[0] == 13 and bounds[1] == 13 + 4096 and len(bounds) > 8
    cut = tmp_path / "cut.bag"
    for b in bounds[1:]:
        for end in (b - 1, b + 1):
            if end > len(raw):
                continue
            cut.write_bytes(raw[:end])
            with pytest.raises(ValueError, match=r"truncated.*byte offset \d+"):
                rosbag1.Bag(cut)
        cut.write_bytes(raw[:b])  # a cut AT a boundary leaves a shorter, well-formed bag
        rosbag1.Bag(cut)
    # a chunk whose inner records are cut short
    inner = fx.connection_record(0, "/points", PC2) + fx.message_record(0, (1, 2), b"abc")
    cut.write_bytes(fx.MAGIC + fx.bag_header_record() + fx.chunk_record(inner[:-1]))
    with pytest.raises(ValueError, match="truncated.*byte offset"):
        rosbag1.Bag(cut)


def test_valid_bag(tmp_path):
    good, bad, short = tmp_path / "g.bag", tmp_path / "b.bag", tmp_path / "s.bag"
    fx.write_bag(good, [(0, "/points", PC2)], [])
    bad.write_bytes(b"#ROSBAG V1.2\n" + b" " * 100)
    short.write_bytes(b"#ROSBAG V2.0")
    assert rosbag1.valid_bag(good) and not rosbag1.valid_bag(bad) and not rosbag1.valid_bag(short)
    assert not rosbag1.valid_bag(tmp_path / "missing.bag") and not rosbag1.valid_bag(tmp_path)
    with pytest.raises(ValueError, match="not a ROS1 bag"):
        rosbag1.Bag(bad)


def test_to_mono8_for_the_five_encodings():
    rng = np.random.default_rng(3)
    h, w = 7, 13
    gray = rng.integers(0, 256, (h, w), dtype=np.uint8)
    assert np.array_equal(rosbag1.to_mono8(rosbag1.decode_image(fx.image((1, 2), gray, "mono8", step=16))), gray)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    rgb[0, 0], rgb[0, 1], rgb[0, 2] = (255, 255, 255), (0, 0, 0), (255, 0, 255)
    r, g, b = (rgb[:, :, k].astype(np.int64) for k in range(3))
    want = ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)
    assert want[0, 0] == 255 and want[0, 1] == 0
    alpha = rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
    for enc, arr in (("rgb8", rgb), ("bgr8", rgb[:, :, ::-1]), ("rgba8", np.concatenate([rgb, alpha], axis=2)), ("bgra8", np.concatenate([rgb[:, :, ::-1], alpha], axis=2))):
        msg = rosbag1.decode_image(fx.image((1, 2), arr, enc, step=arr.shape[1] * arr.shape[2] + 3))
        assert (msg.height, msg.width, msg.encoding, msg.stamp) == (h, w, enc, (1, 2))
        out = rosbag1.to_mono8(msg)
        assert out.dtype == np.uint8 and out.flags.c_contiguous and np.array_equal(out, want), enc
    for enc in ("mono16", "bayer_rggb8", "16UC1"):
        with pytest.raises(ValueError, match=enc):
            rosbag1.to_mono8(rosbag1.decode_image(fx.image((1, 2), gray, enc)))


def test_compressed_image_png_decodes_and_jpeg_is_refused(tmp_path):
    gray = np.random.default_rng(4).integers(0, 256, (9, 11), dtype=np.uint8)
    png = tmp_path / "g.png"
    dataset.write_png_gray(png, gray)
    msg = rosbag1.decode_compressed_image(fx.compressed_image((3, 4), "png", png.read_bytes()))
    assert (msg.format, msg.stamp) == ("png", (3, 4))
    assert np.array_equal(rosbag1.compressed_to_mono8(msg), gray)
    rgb = np.random.default_rng(5).integers(0, 256, (9, 11, 3), dtype=np.uint8)
    dataset.write_png(png, rgb)
    msg = rosbag1.decode_compressed_image(fx.compressed_image((3, 4), "rgb8; png compressed bgr8", png.read_bytes()))
    assert np.array_equal(rosbag1.compressed_to_mono8(msg), dataset.read_png_gray(png))
    jpeg = rosbag1.decode_compressed_image(fx.compressed_image((3, 4), "jpeg", b"\xff\xd8\xff\xe0" + b"\x00" * 20))
    with pytest.raises(ValueError, match="JPEG images are not decoded here"):
        rosbag1.compressed_to_mono8(jpeg)
    with pytest.raises(ValueError, match="tiff"):
        rosbag1.compressed_to_mono8(rosbag1.decode_compressed_image(fx.compressed_image((3, 4), "tiff", b"II*\x00" + b"\x00" * 20)))


def test_camera_info_decodes_to_intrinsics_and_distortion():
    K = [610.5, 0.0, 322.25, 0.0, 611.75, 241.5, 0.0, 0.0, 1.0]
    D = [-0.04, 0.08, 1e-4, -3e-4, -0.04]
    info = rosbag1.decode_camera_info(fx.camera_info((8, 9), 640, 480, "plumb_bob", D, K))
    assert (info.width, info.height, info.stamp, info.frame_id) == (640, 480, (8, 9), "camera")
    assert rosbag1.camera_from_info(info) == ("plumb_bob", [610.5, 611.75, 322.25, 241.5], D)
    assert info.K == K and info.R == [1, 0, 0, 0, 1, 0, 0, 0, 1] and len(info.P) == 12
    info = rosbag1.decode_camera_info(fx.camera_info((8, 9), 640, 480, "equidistant", [], K))
    assert rosbag1.camera_from_info(info) == ("equidistant", [610.5, 611.75, 322.25, 241.5], [])
    with pytest.raises(ValueError, match="truncated"):
        rosbag1.decode_camera_info(fx.camera_info((8, 9), 640, 480, "plumb_bob", D, K)[:-1])


OUSTER = np.dtype({"names": ["x", "y", "z", "intensity", "t", "reflectivity", "ring", "ambient", "range"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u4", "<u2", "<u2", "<u2", "<u4"],
                   "offsets": [0, 4, 8, 16, 20, 24, 26, 28, 32], "itemsize": 48})


def test_pointcloud2_field_table_and_zero_copy_data():
    rec = np.zeros(5, dtype=OUSTER)
    rec["x"], rec["t"], rec["reflectivity"] = np.arange(5), np.arange(5) * 1000, np.arange(5) + 7
    raw = fx.cloud_from_struct((12, 500000000), rec, frame_id="os_sensor")
    cloud = rosbag1.decode_pointcloud2(memoryview(raw))
    assert cloud.fields == [rosbag1.PointField("x", 0, 7, 1), rosbag1.PointField("y", 4, 7, 1), rosbag1.PointField("z", 8, 7, 1), rosbag1.PointField("intensity", 16, 7, 1),
                            rosbag1.PointField("t", 20, 6, 1), rosbag1.PointField("reflectivity", 24, 4, 1), rosbag1.PointField("ring", 26, 4, 1),
                            rosbag1.PointField("ambient", 28, 4, 1), rosbag1.PointField("range", 32, 6, 1)]
    assert (cloud.height, cloud.width, cloud.point_step, cloud.row_step, cloud.is_bigendian, cloud.is_dense, cloud.frame_id) == (1, 5, 48, 240, 0, 1, "os_sensor")
    assert rosbag1.stamp_to_sec(cloud.stamp) == 12.5 and rosbag1.num_points(cloud) == 5
    assert isinstance(cloud.data, np.ndarray) and cloud.data.dtype == np.uint8 and cloud.data.tobytes() == rec.tobytes()
    assert not cloud.data.flags.owndata and np.shares_memory(cloud.data, np.frombuffer(raw, dtype=np.uint8))  # a view, not a copy
    table = rosbag1.field_table(cloud)
    assert np.array_equal(rosbag1.read_field_all(cloud, table["reflectivity"]), np.arange(5) + 7.0)
    assert np.array_equal(rosbag1.read_field(cloud, table["t"], [0, 4]), [0.0, 4000.0])
    with pytest.raises(ValueError, match="truncated"):
        rosbag1.decode_pointcloud2(raw[:-2])


# ---------------------------------------------------------------------------------------------- TimeKeeper
def _keeper():
    log = []
    return preprocess.TimeKeeper(log=log.append), log


def test_time_keeper_skips_a_rewinding_frame():
    k, log = _keeper()
    assert k.process(100.0, 0.0, 0.09, 0.0) and k.process(100.1, 0.0, 0.09, 0.0)
    assert not k.process(100.05, 0.0, 0.09, 0.0)
    assert log[-2] == "warning: point timestamp rewind detected!!" and log[-1] == "       : current:100.050000 last:100.100000 diff:-0.050000"
    assert k.last_points_stamp == 100.1  # the skipped frame does not move the clock
    assert k.process(100.1, 0.0, 0.09, 0.0) and k.process(100.7, 0.0, 0.09, 0.0)
    assert log[-2] == "warning: large time gap between consecutive LiDAR frames!!"


def test_time_keeper_absolute_point_times():
    # point times near the frame stamp: the first point's time becomes the stamp
    k, log = _keeper()
    assert k.process(1000.0, 1000.02, 1000.12, 1000.02) and k.stamp == 1000.02 and k.point_time_offset == 0.0
    assert "warning: use first point timestamp as frame timestamp" in log
    n = len(log)
    assert k.process(1000.1, 1000.12, 1000.22, 1000.12) and k.stamp == 1000.12 and len(log) == n  # warnings once
    assert not k.process(1000.2, 1000.05, 1000.15, 1000.05)  # the point clock rewinds although the frame stamp does not
    # point times on another clock: the offset of the first frame is kept
    k, log = _keeper()
    assert k.process(5000.0, 20.0, 20.1, 20.0) and k.stamp == 5000.0 and k.point_time_offset == 4980.0
    assert "warning: point timestamp is too apart from frame timestamp!!" in log
    assert k.process(5000.3, 20.1, 20.2, 20.1) and k.stamp == 20.1 + 4980.0
    # relative times (first < 1): the stamp stays
    k, log = _keeper()
    assert k.process(77.0, 0.0, 0.1, 0.0) and k.stamp == 77.0 and log == []


def test_time_keeper_nanosecond_times_above_1e16():
    k, log = _keeper()
    t0 = 1.7e18
    assert k.process(1.7e9 + 0.25, t0, t0 + 1e8, t0)
    assert k.stamp == t0 * 1e-9 and any("1e16" in line for line in log) and any("nanosec to sec" in line for line in log)
    assert k.process(1.7e9 + 0.35, t0 + 1e8, t0 + 2e8, t0 + 1e8) and k.stamp == (t0 + 1e8) * 1e-9
    assert not k.process(1.7e9 + 0.45, t0 - 1e8, t0, t0 - 1e8)


def test_time_keeper_negative_times():
    k, log = _keeper()
    calls = []

    def min_time():
        calls.append(1)
        return -0.05

    assert k.process(50.0, -0.05, 0.05, min_time) and calls == [1]
    assert k.stamp == 50.05 and log[0] == "warning: negative per-point timestamp (-0.050000 or 0.050000) found!!" and log[1] == "       : min_stamp=-0.050000"
    assert k.process(50.1, 0.0, 0.1, min_time) and calls == [1]  # the minimum is read only when a time is negative
    assert k.process(50.12, -0.05, 0.05, -0.05) and k.stamp == 50.12 - (-0.05)  # the stamp moves with the times
    assert not k.process(50.2, -0.05, 0.05, -0.1 + 0.2)  # a minimum of +0.1 pulls the stamp back to 50.1 < 50.17
    k, _ = _keeper()
    assert k.process(50.0, 0.01, -0.02, -0.03) and k.stamp == 50.03  # the LAST time negative, the minimum elsewhere


def test_time_keeper_without_a_time_field():
    k, log = _keeper()
    assert k.process(10.0) and k.process(10.1) and not k.process(10.05) and k.process(10.1)
    assert log[:2] == ["warning: per-point timestamps are not given!!", "       : use pseudo per-point timestamps based on the order of points"]
    assert sum("per-point timestamps are not given" in line for line in log) == 1


def test_frame_times_from_raw_bytes():
    rec = np.zeros(4, dtype=OUSTER)
    rec["t"] = [250, 5, 1000000000, 3000000000]
    cloud = rosbag1.decode_pointcloud2(fx.cloud_from_struct((12, 500000000), rec))
    stamp, first, last, min_time = preprocess_ros1.frame_times(cloud, "(here)")
    assert (stamp, first, last, min_time()) == (12.5, 250 / 1e9, 3.0, 5 / 1e9)
    for code, values in (("<f8", [-0.5, 0.25, 1.5]), ("<f4", [0.5, -0.25, 1.5])):
        dt = np.dtype({"names": ["x", "y", "z", "intensity", "timestamp"], "formats": ["<f4", "<f4", "<f4", "<u1", code], "offsets": [0, 4, 8, 12, 13], "itemsize": 22})
        rec = np.zeros(3, dtype=dt)
        rec["timestamp"] = values
        _, first, last, min_time = preprocess_ros1.frame_times(rosbag1.decode_pointcloud2(fx.cloud_from_struct((1, 0), rec)), "(here)")
        assert (first, last, min_time()) == (values[0], values[2], min(values))
    no_time = np.zeros(3, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")])
    assert preprocess_ros1.frame_times(rosbag1.decode_pointcloud2(fx.cloud_from_struct((1, 0), no_time)), "(here)") == (1.0, None, None, None)
    assert preprocess_ros1.frame_times(rosbag1.decode_pointcloud2(fx.cloud_from_struct((1, 0), np.zeros(0, dtype=OUSTER))), "(here)") == (1.0, None, None, None)
    bad = np.zeros(3, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("t", "<u2")])
    with pytest.raises(ValueError, match="unsupported time type 4"):
        preprocess_ros1.frame_times(rosbag1.decode_pointcloud2(fx.cloud_from_struct((1, 0), bad)), "(here)")


# ---------------------------------------------------------------------------------------------- the command line's host logic
XYZI = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")])


def _args(*argv):
    return preprocess_ros1.build_parser().parse_args(preprocess_ros1._attach_values(list(argv)))


def _bag(tmp_path, conns, msgs, name="a.bag", **kw):
    path = tmp_path / name
    fx.write_bag(path, conns, msgs, **kw)
    return rosbag1.Bag(path)


def test_defaults_are_the_references():
    a = _args("src", "dst")
    assert (a.data_path, a.dst_path, a.intensity_channel, a.camera_model, a.voxel_resolution, a.min_distance, a.k_neighbors) == ("src", "dst", "auto", "auto", 0.002, 1.0, 20)
    assert not a.auto_topic and not a.dynamic_lidar_integration and not a.verbose and a.bag_id is None and a.first_n_bags is None and a.device == 0
    a = _args("src", "dst", "-a", "-i", "reflectivity", "--camera_distortion_coeffs", "-0.04,0.08", "--first_n_bags", "2", "--verbose", "--k_neighbors", "10")
    assert a.auto_topic and a.intensity_channel == "reflectivity" and a.camera_distortion_coeffs == "-0.04,0.08" and a.first_n_bags == 2 and a.verbose


def test_topic_selection(tmp_path):
    conns = [(0, "/cam/info", INFO), (1, "/cam/image", IMG), (2, "/lidar/points", PC2), (3, "/cam2/image/compressed", CIMG), (4, "/imu", "sensor_msgs/Imu"), (5, "/lidar2/points", PC2)]
    bag = _bag(tmp_path, conns, [(4, (1, 0), b"x")], index=True)  # (connections without messages: only the index section lists them)
    warn, log = [], []
    assert preprocess_ros1.get_topics(_args("s", "d", "-a"), bag, log=log.append, warn=warn.append) == ("/cam/info", "/cam2/image/compressed", "/lidar2/points")  # the last wins
    assert warn == ["warning: bag constains multiple image topics!!", "warning: bag constains multiple points topics!!"]
    assert "- /imu : sensor_msgs/Imu" in log
    # without -a: the named topics; what is missing is warned about
    warn = []
    assert preprocess_ros1.get_topics(_args("s", "d", "--image_topic", "/i", "--points_topic", "/p"), bag, log=log.append, warn=warn.append) == ("", "/i", "/p")
    assert warn == ["warning: failed to get camera_info topic!!"]
    # -a fills what it finds, the options the rest
    bag = _bag(tmp_path, [(0, "/lidar/points", PC2)], [], name="b.bag", outside=True)
    warn = []
    assert preprocess_ros1.get_topics(_args("s", "d", "-a", "--image_topic", "/i", "--points_topic", "/ignored"), bag, log=log.append, warn=warn.append) == ("", "/i", "/lidar/points")


def test_intensity_channel_priority(tmp_path):
    def bag_with(names, name):
        dt = np.dtype([(n, "<f4") for n in names])
        return _bag(tmp_path, [(0, "/p", PC2)], [(0, (1, 0), fx.cloud_from_struct((1, 0), np.zeros(2, dtype=dt)))], name=name)

    auto = _args("s", "d")
    assert preprocess_ros1.get_intensity_channel(auto, bag_with(["x", "y", "z", "intensity", "reflectivity"], "1.bag"), "/p") == "reflectivity"
    assert preprocess_ros1.get_intensity_channel(auto, bag_with(["x", "y", "z", "reflectivity", "intensity"], "2.bag"), "/p") == "reflectivity"
    assert preprocess_ros1.get_intensity_channel(auto, bag_with(["x", "y", "z", "intensity"], "3.bag"), "/p") == "intensity"
    assert preprocess_ros1.get_intensity_channel(_args("s", "d", "-i", "ambient"), bag_with(["x", "y", "z", "intensity"], "4.bag"), "/p") == "ambient"
    with pytest.raises(ValueError, match="failed to determine point intensity channel automatically.*'/p'.*5.bag"):
        preprocess_ros1.get_intensity_channel(auto, bag_with(["x", "y", "z", "ring"], "5.bag"), "/p")
    with pytest.raises(ValueError, match="'/q'.*5.bag"):
        preprocess_ros1.get_intensity_channel(auto, bag_with(["x", "y", "z", "ring"], "5.bag"), "/q")


def test_camera_parameters(tmp_path):
    K = [610.5, 0.0, 322.25, 0.0, 611.75, 241.5, 0.0, 0.0, 1.0]
    D = [-0.04, 0.08, 1e-4, -3e-4, -0.04]
    gray = np.zeros((6, 10), dtype=np.uint8)
    bag = _bag(tmp_path, [(0, "/info", INFO), (1, "/image", IMG)], [(0, (1, 0), fx.camera_info((1, 0), 10, 6, "plumb_bob", D, K)), (1, (1, 0), fx.image((1, 0), gray, "mono8"))])
    quiet = dict(log=lambda m: None)
    assert preprocess_ros1.get_camera_params(_args("s", "d"), bag, "/info", "/image", **quiet) == ("plumb_bob", (10, 6), [610.5, 611.75, 322.25, 241.5], D)
    manual = _args("s", "d", "--camera_model", "fisheye", "--camera_intrinsics", "1,2,3,4", "--camera_distortion_coeffs", "-0.1,0.2,0,0")
    assert preprocess_ros1.get_camera_params(manual, bag, "/info", "/image", **quiet) == ("fisheye", (10, 6), [1.0, 2.0, 3.0, 4.0], [-0.1, 0.2, 0.0, 0.0])
    assert preprocess_ros1.get_camera_params(_args("s", "d", "--camera_model", "equirectangular"), bag, "", "/image", **quiet) == ("equirectangular", (10, 6), [10.0, 6.0], [])
    assert preprocess_ros1.VALID_CAMERA_MODELS == ("plumb_bob", "fisheye", "equidistant", "omnidir", "equirectangular")
    with pytest.raises(ValueError, match="invalid camera model atan"):  # (the reference's list has no atan, preprocess.cpp:362)
        preprocess_ros1.get_camera_params(_args("s", "d", "--camera_model", "atan", "--camera_intrinsics", "1,2,3,4", "--camera_distortion_coeffs", "0"), bag, "", "/image", **quiet)
    with pytest.raises(ValueError, match="camera_intrinsics has not been set"):
        preprocess_ros1.get_camera_params(_args("s", "d", "--camera_model", "omnidir"), bag, "", "/image", **quiet)
    with pytest.raises(ValueError, match="CameraInfo.*'/nope'.*a.bag"):
        preprocess_ros1.get_camera_params(_args("s", "d"), bag, "/nope", "/image", **quiet)
    with pytest.raises(ValueError, match="image_topic='/nope'.*a.bag"):
        preprocess_ros1.get_camera_params(_args("s", "d"), bag, "/info", "/nope", **quiet)
    # a compressed image topic gives the size of the decoded image
    png = tmp_path / "g.png"
    dataset.write_png_gray(png, gray)
    bag = _bag(tmp_path, [(1, "/image/compressed", CIMG)], [(1, (1, 0), fx.compressed_image((1, 0), "png", png.read_bytes()))], name="c.bag")
    assert preprocess_ros1.get_camera_params(_args("s", "d", "--camera_model", "equirectangular"), bag, "", "/image/compressed", **quiet)[1] == (10, 6)


class StubIntegrator:
    """Records what the command line hands the integrator"""

    def __init__(self):
        self.frames = []

    def insert_cloud2(self, cloud, channel):
        self.frames.append((rosbag1.stamp_to_sec(cloud.stamp), rosbag1.num_points(cloud), channel))
        return 1


def test_frames_reach_the_integrator_in_time_order_without_the_rewound_one(tmp_path):
    def cloud(stamp, n):
        return fx.cloud_from_struct(stamp, np.zeros(n, dtype=XYZI))

    msgs = [(0, (10, 0), cloud((100, 0), 3)), (0, (12, 0), cloud((100, 50000000), 5)), (0, (11, 0), cloud((100, 100000000), 4)), (1, (10, 5), b"not a cloud"),
            (0, (13, 0), cloud((100, 200000000), 0))]
    bag = _bag(tmp_path, [(0, "/p", PC2), (1, "/image", IMG)], msgs)
    stub, warn = StubIntegrator(), []
    assert preprocess_ros1.integrate_bag(_args("s", "d"), bag, "/p", "intensity", stub, warn=warn.append) == (3, 1, 3)
    assert stub.frames == [(100.0, 3, "intensity"), (100.1, 4, "intensity"), (100.2, 0, "intensity")]  # record-time order; 100.05 after 100.1 rewinds
    assert "warning: skip frame with an invalid timestamp!!" in warn and "warning: point timestamp rewind detected!!" in warn


def test_clouds_the_reference_would_crash_on_are_refused_with_topic_and_bag(tmp_path):
    cases = [
        (fx.cloud_from_struct((1, 0), np.zeros(2, dtype=[("x", "<f4"), ("y", "<f4"), ("intensity", "<f4")])), "missing point coordinate fields"),
        (fx.cloud_from_struct((1, 0), np.zeros(2, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("ring", "<u2")])), "no intensity channel 'intensity'"),
        (fx.cloud_from_struct((1, 0), np.zeros(2, dtype=XYZI), is_bigendian=1), "big-endian"),
        (fx.cloud_from_struct((1, 0), np.zeros(2, dtype=XYZI), width=3), "32 data bytes for 3 x 1 points of 16 bytes"),
    ]
    for k, (payload, what) in enumerate(cases):
        bag = _bag(tmp_path, [(0, "/p", PC2)], [(0, (1, 0), payload)], name=f"{k}.bag")
        with pytest.raises(ValueError, match=f"{what}.*'/p'.*{k}.bag"):
            preprocess_ros1.integrate_bag(_args("s", "d"), bag, "/p", "intensity", StubIntegrator())


def test_dynamic_integration_and_empty_directories_exit_with_status_1(tmp_path, capsys):
    assert preprocess_ros1.main([str(tmp_path), str(tmp_path / "dst"), "-d"]) == 1
    assert "dynamic LiDAR integration" in capsys.readouterr().err and not (tmp_path / "dst").exists()
    (tmp_path / "notes.txt").write_text("not a bag")
    (tmp_path / "ros2.db3").write_bytes(b"SQLite format 3\x00" + b"\x00" * 100)
    assert preprocess_ros1.find_bags(str(tmp_path)) == []
    assert preprocess_ros1.main([str(tmp_path), str(tmp_path / "dst")]) == 1
    assert "error: no input bags!!" in capsys.readouterr().err
    assert preprocess_ros1.main([]) == 0  # the usage (preprocess.cpp:73-76)
    assert "data_path" in capsys.readouterr().out
    # a bag without the image topic: status 1, the topic and the bag named, before any GPU work
    fx.write_bag(tmp_path / "b.bag", [(0, "/p", PC2)], [(0, (1, 0), fx.cloud_from_struct((1, 0), np.zeros(2, dtype=XYZI)))])
    fx.write_bag(tmp_path / "a.bag", [(0, "/p", PC2)], [(0, (1, 0), fx.cloud_from_struct((1, 0), np.zeros(2, dtype=XYZI)))])
    assert [p.rsplit("/", 1)[1] for p in preprocess_ros1.find_bags(str(tmp_path))] == ["a.bag", "b.bag"]
    assert preprocess_ros1.main([str(tmp_path), str(tmp_path / "dst"), "--points_topic", "/p", "--image_topic", "/image", "--camera_model", "equirectangular"]) == 1
    err = capsys.readouterr().err
    assert "image_topic='/image'" in err and "a.bag" in err
