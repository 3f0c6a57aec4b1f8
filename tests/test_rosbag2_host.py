"""CPU tests of the ROS2 bag reader (rosbag2.py: CDR, sqlite3 and MCAP storage) and of the host logic of the preprocess_ros2 command
line.  The bags come from tests/rosbag2_fixture.py, a writer that shares no code with the reader; because a reader and a writer by one
author can agree on a wrong layout, each format is also read from bytes spelled out below, field by field, from the public format
descriptions.  Nothing here is pinned against rosbag2_cpp, Fast-CDR or libmcap: none of them is available to these tests."""
import functools
import sqlite3
import struct
import zlib

import numpy as np
import pytest

import rosbag1_fixture as fx1
import rosbag2_fixture as fx
from direct_visual_lidar_calibration_amd import dataset, odometry, preprocess_ros1, preprocess_ros2, rosbag1, rosbag2

PC2, IMG, CIMG, INFO = fx.PC2, fx.IMG, fx.CIMG, fx.INFO

# ---------------------------------------------------------------------------------------------- CDR
# A sensor_msgs/msg/PointCloud2 with two float32 fields and three 8-byte records; the left column is the byte offset in the blob.
CLOUD_LITERAL = (
    b"\x00\x01\x00\x00"  # 0   encapsulation header: 00 01 = little-endian plain CDR, two option bytes.  Alignment counts from byte 4
    b"\x0c\x00\x00\x00"  # 4   header.stamp.sec = 12 (int32)
    b"\x00\x65\xcd\x1d"  # 8   header.stamp.nanosec = 500 000 000 (uint32)
    b"\x06\x00\x00\x00"  # 12  header.frame_id: length 6, the NUL included
    b"lidar\x00"  # 16
    b"\x00\x00"  # 22  padding to a multiple of 4 after byte 4
    b"\x01\x00\x00\x00"  # 24  height = 1
    b"\x03\x00\x00\x00"  # 28  width = 3
    b"\x02\x00\x00\x00"  # 32  fields: 2 elements
    b"\x02\x00\x00\x00" b"x\x00"  # 36  fields[0].name = "x"
    b"\x00\x00"  # 42  padding
    b"\x00\x00\x00\x00"  # 44  fields[0].offset = 0
    b"\x07"  # 48  fields[0].datatype = FLOAT32 (unaligned)
    b"\x00\x00\x00"  # 49  padding
    b"\x01\x00\x00\x00"  # 52  fields[0].count = 1
    b"\x0a\x00\x00\x00" b"intensity\x00"  # 56  fields[1].name = "intensity"
    b"\x00\x00"  # 70  padding
    b"\x04\x00\x00\x00"  # 72  fields[1].offset = 4
    b"\x07"  # 76  fields[1].datatype = FLOAT32
    b"\x00\x00\x00"  # 77  padding
    b"\x01\x00\x00\x00"  # 80  fields[1].count = 1
    b"\x00"  # 84  is_bigendian = false
    b"\x00\x00\x00"  # 85  padding
    b"\x08\x00\x00\x00"  # 88  point_step = 8
    b"\x18\x00\x00\x00"  # 92  row_step = 24
    b"\x18\x00\x00\x00"  # 96  data: 24 bytes
    b"\x00\x00\x80\x3f\x00\x00\x00\x3f"  # 100 record 0: x = 1.0, intensity = 0.5
    b"\x00\x00\x00\x40\x00\x00\x80\xbf"  # 108 record 1: x = 2.0, intensity = -1.0
    b"\x00\x00\x40\x40\x00\x00\x80\x40"  # 116 record 2: x = 3.0, intensity = 4.0
    b"\x01"  # 124 is_dense = true
)
CLOUD_FIELDS = [rosbag1.PointField("x", 0, 7, 1), rosbag1.PointField("intensity", 4, 7, 1)]
CLOUD_DATA = struct.pack("<6f", 1.0, 0.5, 2.0, -1.0, 3.0, 4.0)


def test_a_hand_packed_pointcloud2_blob():
    assert len(CLOUD_LITERAL) == 125 and CLOUD_LITERAL[100:124] == CLOUD_DATA
    cloud = rosbag2.decode_pointcloud2(memoryview(CLOUD_LITERAL))
    assert cloud == rosbag1.PointCloud2((12, 500000000), "lidar", 1, 3, CLOUD_FIELDS, 0, 8, 24, cloud.data, 1) and type(cloud) is rosbag1.PointCloud2
    assert cloud.data.dtype == np.uint8 and cloud.data.tobytes() == CLOUD_DATA
    assert not cloud.data.flags.owndata and np.shares_memory(cloud.data, np.frombuffer(CLOUD_LITERAL, dtype=np.uint8))  # a view, not a copy
    assert rosbag2.stamp_to_sec(cloud.stamp) == 12.5 and rosbag2.num_points(cloud) == 3
    assert np.array_equal(rosbag2.read_field_all(cloud, rosbag2.field_table(cloud)["intensity"]), [0.5, -1.0, 4.0])
    assert fx.pointcloud2((12, 500000000), [("x", 0, 7, 1), ("intensity", 4, 7, 1)], 8, CLOUD_DATA) == CLOUD_LITERAL  # the fixture writes these very bytes


def test_the_alignment_sweep():
    """frame_id lengths 0..8 and field names of lengths 1..5 put every padding 0..3 before a u32.  ``data`` follows its u32 count, so in the
    blob it starts at a multiple of 4 -- both residues mod 8 that leaves occur; the blob itself lies anywhere in a storage file, so the
    decode is repeated on views that start at every residue mod 8 of their buffer."""
    residues, paddings, addresses = set(), set(), set()
    for frame_len in range(9):
        for name_len in range(1, 6):
            frame_id, name = "f" * frame_len, "abcde"[:name_len]
            fields = [("x", 0, 7, 1), (name, 4, 7, 1)]
            blob = fx.pointcloud2((3, 4), fields, 8, CLOUD_DATA, frame_id=frame_id)
            paddings.add((4 - (16 + frame_len + 1)) % 4)  # before height: after the frame_id's bytes, which start at byte 16
            residues.add(fx.data_offset(blob, CLOUD_DATA) % 8)
            for shift in range(8):
                buffer = b"\xaa" * shift + blob + b"\xaa"
                cloud = rosbag2.decode_pointcloud2(memoryview(buffer)[shift : shift + len(blob)])
                assert (cloud.stamp, cloud.frame_id, cloud.height, cloud.width, cloud.point_step, cloud.row_step, cloud.is_bigendian, cloud.is_dense) == ((3, 4), frame_id, 1, 3, 8, 24, 0, 1)
                assert cloud.fields == [rosbag1.PointField(*f) for f in fields] and cloud.data.tobytes() == CLOUD_DATA
                base = np.frombuffer(buffer, dtype=np.uint8)
                assert np.shares_memory(cloud.data, base)
                addresses.add((cloud.data.ctypes.data - base.ctypes.data) % 8)
    assert paddings == {0, 1, 2, 3} and residues == {0, 4} and addresses == set(range(8))


K = [610.5, 0.0, 322.25, 0.0, 611.75, 241.5, 0.0, 0.0, 1.0]


@pytest.mark.parametrize("num_d", [0, 5, 8])
def test_camera_info_with_d_of_length_0_5_and_8(num_d):
    """After the u32 count of ``d`` the float64 elements align to 8 counted from byte 4 of the blob: with "plumb_bob" the count ends at blob
    offset 52 = 4 + 48 and no padding follows -- counted from byte 0 there would be four bytes of it; with "fisheye" it ends at 48 = 4 + 44
    and four bytes of padding do follow"""
    D = [-0.04, 0.08, 1e-4, -3e-4, -0.04, 0.5, 0.25, 0.125][:num_d]
    for model in ("plumb_bob", "rational_polynomial", "equidistant", "fisheye"):
        blob = fx.camera_info((8, 9), 640, 480, model, D, K)
        info = rosbag2.decode_camera_info(blob)
        want = rosbag1.decode_camera_info(fx1.camera_info((8, 9), 640, 480, model, D, K))
        assert info == want and type(info) is rosbag1.CameraInfo
        assert rosbag2.camera_from_info(info) == rosbag1.camera_from_info(want) == (model, [610.5, 611.75, 322.25, 241.5], D)
    # the position of d[0], spelled out for "plumb_bob" (10 bytes with its NUL): 4 header, 8 stamp, 4 + 7 frame_id "camera", 1 pad, 8 size, 4 + 10 model, 2 pad, 4 count
    blob = fx.camera_info((8, 9), 640, 480, "plumb_bob", D, K)
    count_at = 4 + 8 + 4 + 7 + 1 + 8 + 4 + 10 + 2
    assert struct.unpack_from("<I", blob, count_at)[0] == num_d
    assert count_at == 48 and struct.unpack_from("<d", blob, 52)[0] == (D + K)[0] and len(blob) == 52 + 8 * (num_d + 30) + 8 + 17
    # "fisheye" (8 bytes with its NUL): the count at 44, four bytes of padding, d[0] at 52 as well
    blob = fx.camera_info((8, 9), 640, 480, "fisheye", D, K)
    assert struct.unpack_from("<I", blob, 44)[0] == num_d and blob[48:52] == b"\x00" * 4 and struct.unpack_from("<d", blob, 52)[0] == (D + K)[0]


def test_image_in_the_five_encodings():
    rng = np.random.default_rng(3)
    h, w = 7, 13
    gray = rng.integers(0, 256, (h, w), dtype=np.uint8)
    assert np.array_equal(rosbag2.to_mono8(rosbag2.decode_image(fx.image((1, 2), gray, "mono8", step=16))), gray)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    r, g, b = (rgb[:, :, k].astype(np.int64) for k in range(3))
    want = ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)
    alpha = rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
    for enc, arr in (("rgb8", rgb), ("bgr8", rgb[:, :, ::-1]), ("rgba8", np.concatenate([rgb, alpha], axis=2)), ("bgra8", np.concatenate([rgb[:, :, ::-1], alpha], axis=2))):
        step = arr.shape[1] * arr.shape[2] + 3
        blob = fx.image((1, 2), arr, enc, step=step, frame_id="cam" + enc)  # (frame_ids of four lengths)
        msg = rosbag2.decode_image(blob)
        assert msg == rosbag1.decode_image(fx1.image((1, 2), arr, enc, step=step, frame_id="cam" + enc))._replace(data=msg.data) and type(msg) is rosbag1.Image
        assert np.shares_memory(msg.data, np.frombuffer(blob, dtype=np.uint8)) and np.array_equal(rosbag2.to_mono8(msg), want), enc
    with pytest.raises(ValueError, match="mono16"):
        rosbag2.to_mono8(rosbag2.decode_image(fx.image((1, 2), gray, "mono16")))


def test_compressed_image_with_a_png(tmp_path):
    gray = np.random.default_rng(4).integers(0, 256, (9, 11), dtype=np.uint8)
    png = tmp_path / "g.png"
    dataset.write_png_gray(png, gray)
    msg = rosbag2.decode_compressed_image(fx.compressed_image((3, 4), "png", png.read_bytes()))
    assert (msg.format, msg.stamp, msg.frame_id) == ("png", (3, 4), "camera") and bytes(msg.data) == png.read_bytes() and type(msg) is rosbag1.CompressedImage
    assert np.array_equal(rosbag2.compressed_to_mono8(msg), gray)


def test_big_endian_and_parameter_list_encapsulations_are_refused_by_name():
    for kind, name in ((b"\x00\x00", "big-endian"), (b"\x00\x02", "PL_CDR_BE"), (b"\x00\x03", "PL_CDR_LE"), (b"\x00\x07", "CDR2_LE"), (b"\x00\x0b", "PL_CDR2_LE"), (b"\x12\x34", "unknown")):
        for decode in (rosbag2.decode_pointcloud2, rosbag2.decode_image, rosbag2.decode_compressed_image, rosbag2.decode_camera_info):
            with pytest.raises(ValueError, match=name):
                decode(kind + CLOUD_LITERAL[2:])


def test_every_proper_prefix_of_a_blob_is_refused_with_an_offset():
    blobs = [(rosbag2.decode_pointcloud2, CLOUD_LITERAL), (rosbag2.decode_image, fx.image((1, 2), np.zeros((2, 3), dtype=np.uint8), "mono8")),
             (rosbag2.decode_compressed_image, fx.compressed_image((1, 2), "png", b"\x89PNG....")), (rosbag2.decode_camera_info, fx.camera_info((8, 9), 640, 480, "plumb_bob", [0.1, 0.2, 0.3], K))]
    for decode, blob in blobs:
        decode(blob)
        for cut in range(len(blob)):
            with pytest.raises(ValueError, match=r"truncated message \(\d+ bytes wanted at byte offset \d+ of \d+\)"):
                decode(blob[:cut])
    # a count that promises more than the blob holds: refused, not guessed
    huge = bytearray(CLOUD_LITERAL)
    huge[96:100] = b"\xff\xff\xff\x7f"
    with pytest.raises(ValueError, match="byte offset 100 of 125"):
        rosbag2.decode_pointcloud2(bytes(huge))
    huge = bytearray(CLOUD_LITERAL)
    huge[32:36] = b"\xff\xff\xff\xff"
    with pytest.raises(ValueError, match="truncated"):
        rosbag2.decode_pointcloud2(bytes(huge))


# ---------------------------------------------------------------------------------------------- sqlite3
def _payloads(bag, topic=None):
    return [(m.topic, m.type, m.time, bytes(m.data)) for m in bag.messages(topic)]


TOPICS = [(1, "/points", PC2), (2, "/image", IMG), (3, "/info", INFO)]


def _eight():
    """(topic id, timestamp [ns], payload) x 8 in ascending time, and what ``messages()`` must give for them"""
    msgs = [(k % 3 + 1, (100 + k) * 1000000000 + 5 * k, bytes([k]) * (k + 1)) for k in range(8)]
    return msgs, [(TOPICS[k % 3][1], TOPICS[k % 3][2], (100 + k, 5 * k), bytes([k]) * (k + 1)) for k in range(8)]


def test_a_split_directory_bag_reads_file_after_file_and_a_bare_file_reads(tmp_path):
    msgs, want = _eight()
    fx.write_sqlite3_dir(tmp_path / "run", TOPICS, msgs, split=3)
    assert sorted(p.name for p in (tmp_path / "run").iterdir()) == ["metadata.yaml", "run_0.db3", "run_1.db3"]
    assert rosbag2.valid_bag(tmp_path / "run") and rosbag2.valid_bag(str(tmp_path / "run" / "run_1.db3"))
    bag = rosbag2.Bag(tmp_path / "run")
    assert (bag.path, bag.storage) == (str(tmp_path / "run"), "sqlite3")
    assert bag.topics_and_types() == [(t[1], t[2]) for t in TOPICS] == rosbag2.topics_and_types(tmp_path / "run")
    assert _payloads(bag) == want and _payloads(bag, "/image") == [m for m in want if m[0] == "/image"] and _payloads(bag, "/nope") == []
    assert all(isinstance(m.data, memoryview) for m in bag.messages())
    assert bag.first_message("/image", "Image").data == b"\x01\x01" and bag.first_message("/image", "CompressedImage") is None and bag.first_message("/nope") is None
    # list order, not name or time order: the second file first
    fx.write_metadata(tmp_path / "run", "sqlite3", ["run_1.db3", "run_0.db3"])
    assert _payloads(rosbag2.Bag(tmp_path / "run")) == want[3:] + want[:3]
    assert _payloads(rosbag2.Bag(tmp_path / "run" / "run_1.db3")) == want[3:]  # a bare file
    # a listed file that is missing: not a bag
    fx.write_metadata(tmp_path / "run", "sqlite3", ["run_0.db3", "run_2.db3"])
    assert not rosbag2.valid_bag(tmp_path / "run")
    with pytest.raises(ValueError, match="run_2.db3"):
        rosbag2.Bag(tmp_path / "run")


def test_rows_inserted_out_of_order_come_by_timestamp_then_id(tmp_path):
    times = [5000000000, 3000000009, 3000000009, 4000000000, 3000000008, 5000000000, 2999999999, 3000000009]
    msgs = [(1, t, bytes([k])) for k, t in enumerate(times)]
    fx.write_sqlite3(tmp_path / "t.db3", TOPICS, msgs)
    got = [m.data[0] for m in rosbag2.Bag(tmp_path / "t.db3").messages("/points")]
    assert got == [6, 4, 1, 2, 7, 3, 0, 5] == sorted(range(8), key=lambda k: (times[k], k))
    assert [m.time for m in rosbag2.Bag(tmp_path / "t.db3").messages()][:2] == [(2, 999999999), (3, 8)]


def test_the_old_and_the_new_topics_schema_both_read(tmp_path):
    msgs, want = _eight()
    for schema in ("old", "new"):
        fx.write_sqlite3(tmp_path / f"{schema}.db3", TOPICS, msgs, schema=schema)
        tables = {r[0] for r in sqlite3.connect(tmp_path / f"{schema}.db3").execute("SELECT name FROM sqlite_master WHERE type = 'table'")}
        assert ("schema" in tables) == (schema == "new")
        assert _payloads(rosbag2.Bag(tmp_path / f"{schema}.db3")) == want
    # the schema spelled out here, columns in another order and one more: they are selected by name
    db = sqlite3.connect(tmp_path / "hand.db3")
    db.execute("CREATE TABLE topics(type TEXT, extra INTEGER, serialization_format TEXT, name TEXT, id INTEGER PRIMARY KEY)")
    db.execute("CREATE TABLE messages(data BLOB, timestamp INTEGER, topic_id INTEGER, id INTEGER PRIMARY KEY)")
    db.execute("INSERT INTO topics VALUES ('sensor_msgs/msg/Image', 0, 'cdr', '/image', 7)")
    db.execute("INSERT INTO topics VALUES ('sensor_msgs/msg/Image', 0, 'cdr', '/image', 9)")  # the name a second time: read over both ids
    db.execute("INSERT INTO messages VALUES (x'0102', 20, 9, 1)")
    db.execute("INSERT INTO messages VALUES (x'03', 10, 7, 2)")
    db.commit()
    db.close()
    bag = rosbag2.Bag(tmp_path / "hand.db3")
    assert bag.topics_and_types() == [("/image", IMG), ("/image", IMG)]
    assert [(m.conn, m.time, bytes(m.data)) for m in bag.messages("/image")] == [(7, (0, 10), b"\x03"), (9, (0, 20), b"\x01\x02")]


def test_what_is_not_a_ros2_bag(tmp_path):
    fake = tmp_path / "ros2.db3"
    fake.write_bytes(b"SQLite format 3\x00" + b"\x00" * 100)  # the 116 bytes of tests/test_rosbag1_host.py
    ros1 = tmp_path / "a.bag"
    fx1.write_bag(ros1, [(0, "/points", "sensor_msgs/PointCloud2")], [(0, (1, 0), b"abc")])
    text = tmp_path / "notes.txt"
    text.write_text("not a bag")
    other = tmp_path / "other.db3"  # a real database, but not a bag's
    db = sqlite3.connect(other)
    db.execute("CREATE TABLE topics(id INTEGER PRIMARY KEY)")
    db.commit()
    db.close()
    empty_dir = tmp_path / "dir"
    empty_dir.mkdir()
    bad_yaml = tmp_path / "bad"
    bad_yaml.mkdir()
    (bad_yaml / "metadata.yaml").write_text("rosbag2_bagfile_information: [1, 2\n")
    (tmp_path / "empty.mcap").write_bytes(b"")
    assert len(fake.read_bytes()) == 116 and rosbag1.valid_bag(ros1)
    for p in (fake, ros1, text, other, empty_dir, bad_yaml, tmp_path / "missing", tmp_path / "empty.mcap"):
        assert rosbag2.valid_bag(p) is False and rosbag2.valid_bag(str(p)) is False
        with pytest.raises(ValueError, match=p.name):
            rosbag2.Bag(p)
    assert preprocess_ros1.find_bags(str(tmp_path), rosbag2) == [] and preprocess_ros1.find_bags(str(tmp_path)) == [str(ros1)]


def test_a_topic_that_is_not_cdr_is_refused_when_it_is_asked_for(tmp_path):
    fx.write_sqlite3(tmp_path / "p.db3", [(1, "/points", PC2, "protobuf"), (2, "/image", IMG)], [(1, 5, b"a"), (2, 6, b"b")])
    bag = rosbag2.Bag(tmp_path / "p.db3")
    assert _payloads(bag, "/image") == [("/image", IMG, (0, 6), b"b")]
    for topic in ("/points", None):
        with pytest.raises(ValueError, match="'/points' is serialised as 'protobuf'.*cdr"):
            list(bag.messages(topic))
    fx.write_mcap(tmp_path / "p.mcap", [(1, "/points", PC2, "protobuf"), (2, "/image", IMG)], [(1, 5, b"a"), (2, 6, b"b")])
    bag = rosbag2.Bag(tmp_path / "p.mcap")
    assert _payloads(bag, "/image") == [("/image", IMG, (0, 6), b"b")]
    with pytest.raises(ValueError, match="'/points' is serialised as 'protobuf'.*cdr"):
        list(bag.messages("/points"))


def _zstd_compress():
    try:
        from compression import zstd

        return zstd.compress
    except ImportError:
        pass
    try:
        import zstandard

        return zstandard.ZstdCompressor().compress
    except ImportError:
        pass
    try:
        import zstd

        return zstd.compress
    except ImportError:
        return None


@pytest.mark.parametrize("mode", ["FILE", "MESSAGE"])
def test_a_compression_mode_is_refused_with_its_name_or_decoded(tmp_path, mode):
    compress = _zstd_compress()
    msgs, want = _eight()
    run = tmp_path / "run"
    run.mkdir()
    if mode == "MESSAGE":
        fx.write_sqlite3(run / "run_0.db3", TOPICS, [(i, t, (compress or bytes)(p)) for i, t, p in msgs])
        fx.write_metadata(run, "sqlite3", ["run_0.db3"], "zstd", mode)
    else:
        fx.write_sqlite3(run / "plain.db3", TOPICS, msgs)
        (run / "run_0.db3.zstd").write_bytes((compress or bytes)((run / "plain.db3").read_bytes()))
        fx.write_metadata(run, "sqlite3", ["run_0.db3.zstd"], "zstd", mode)
    assert rosbag2.valid_bag(run)  # it opens; what it needs to be read is said when it is read
    if compress is None:
        with pytest.raises(ValueError, match=f"{run}.*'{mode}'.*'zstd'"):
            rosbag2.Bag(run)
    else:
        assert _payloads(rosbag2.Bag(run)) == want
    fx.write_metadata(run, "sqlite3", ["run_0.db3.zstd" if mode == "FILE" else "run_0.db3"], "fancy", mode)
    with pytest.raises(ValueError, match=f"'{mode}'.*'fancy'"):
        rosbag2.Bag(run)


# ---------------------------------------------------------------------------------------------- MCAP
CHAT = b"\x00\x01\x00\x00" b"\x03\x00\x00\x00" b"hi\x00"  # a CDR std_msgs/msg/String: the header, length 3 with the NUL, "hi"
MCAP_LITERAL = (
    b"\x89MCAP0\r\n"  # 0   magic
    b"\x01" b"\x0c\x00\x00\x00\x00\x00\x00\x00"  # 8   Header, 12 bytes
    b"\x04\x00\x00\x00ros2"  # 17  profile
    b"\x00\x00\x00\x00"  # 25  library = ""
    b"\x03" b"\x33\x00\x00\x00\x00\x00\x00\x00"  # 29  Schema, 51 bytes
    b"\x01\x00"  # 38  id = 1
    b"\x13\x00\x00\x00std_msgs/msg/String"  # 40  name: the message type
    b"\x07\x00\x00\x00ros2msg"  # 63  encoding
    b"\x0b\x00\x00\x00string data"  # 74  data
    b"\x04" b"\x18\x00\x00\x00\x00\x00\x00\x00"  # 89  Channel, 24 bytes
    b"\x07\x00"  # 98  id = 7
    b"\x01\x00"  # 100 schema_id = 1
    b"\x05\x00\x00\x00/chat"  # 102 topic
    b"\x03\x00\x00\x00cdr"  # 111 message_encoding
    b"\x00\x00\x00\x00"  # 118 metadata: a map of 0 bytes
    b"\x05" b"\x21\x00\x00\x00\x00\x00\x00\x00"  # 122 Message, 33 bytes
    b"\x07\x00"  # 131 channel_id = 7
    b"\x00\x00\x00\x00"  # 133 sequence = 0
    b"\x07\xe4\x0b\x54\x02\x00\x00\x00"  # 137 log_time = 10 000 000 007 ns
    b"\x08\xe4\x0b\x54\x02\x00\x00\x00"  # 145 publish_time (not used)
    + CHAT  # 153 the payload, to the end of the record
    + b"\x0f" b"\x04\x00\x00\x00\x00\x00\x00\x00" b"\x00\x00\x00\x00"  # 164 DataEnd: data_section_crc = 0 (not computed)
    b"\x02" b"\x14\x00\x00\x00\x00\x00\x00\x00" + b"\x00" * 20  # 177 Footer: no summary
    + b"\x89MCAP0\r\n"  # 206 magic
)


def test_a_hand_packed_minimal_mcap_file(tmp_path):
    assert len(MCAP_LITERAL) == 214 and MCAP_LITERAL[153:164] == CHAT and MCAP_LITERAL[164] == 0x0F and MCAP_LITERAL[177] == 0x02
    path = tmp_path / "hand.mcap"
    path.write_bytes(MCAP_LITERAL)
    assert rosbag2.valid_bag(path)
    bag = rosbag2.Bag(path)
    assert (bag.storage, bag._stores[0].profile, bag._stores[0].library) == ("mcap", "ros2", "")
    assert bag.topics_and_types() == [("/chat", "std_msgs/msg/String")]
    (m,) = bag.messages("/chat")
    assert m == rosbag1.Message(7, "/chat", "std_msgs/msg/String", (10, 7), CHAT) and isinstance(m.data, memoryview)
    assert np.frombuffer(m.data, dtype=np.uint8).flags.owndata is False  # a view of the mapped file


@pytest.mark.parametrize("kw", [dict(), dict(chunk_size=3), dict(chunk_size=3, summary=True), dict(chunk_size=1, summary=True), dict(unknown=True), dict(chunk_size=2, unknown=True)],
                         ids=["unchunked", "chunked", "chunked_with_summary", "one_message_chunks", "unknown_opcodes", "unknown_opcodes_in_chunks"])
def test_chunked_unchunked_and_with_summary_files_parse_alike(tmp_path, kw):
    msgs, want = _eight()
    path = tmp_path / "a.mcap"
    fx.write_mcap(path, TOPICS, msgs, **kw)
    bag = rosbag2.Bag(path)
    assert bag.topics_and_types() == [(t[1], t[2]) for t in TOPICS]
    assert _payloads(bag) == want and _payloads(bag, "/info") == [m for m in want if m[0] == "/info"]
    base = np.frombuffer(bag._stores[0].buf, dtype=np.uint8)
    assert all(np.shares_memory(np.frombuffer(m.data, dtype=np.uint8), base) for m in bag.messages())  # zero-copy, chunked or not
    # the same file as the one storage file of a directory bag
    run = tmp_path / "run"
    run.mkdir(exist_ok=True)
    (run / "run_0.mcap").write_bytes(path.read_bytes())
    fx.write_metadata(run, "mcap", ["run_0.mcap"])
    assert rosbag2.valid_bag(run) and _payloads(rosbag2.Bag(run)) == want


def test_mcap_messages_come_by_log_time_then_file_order(tmp_path):
    times = [5000000000, 3000000009, 3000000009, 4000000000, 3000000008, 5000000000, 2999999999, 3000000009]
    msgs = [(1, t, bytes([k])) for k, t in enumerate(times)]
    for kw in (dict(), dict(chunk_size=3), dict(chunk_size=2, summary=True)):
        fx.write_mcap(tmp_path / "t.mcap", TOPICS, msgs, **kw)
        assert [m.data[0] for m in rosbag2.Bag(tmp_path / "t.mcap").messages("/points")] == [6, 4, 1, 2, 7, 3, 0, 5]


def _one_chunk_file(path, chunk):
    path.write_bytes(fx.MCAP_MAGIC + fx.header_record() + chunk + fx.data_end_record() + fx.footer_record() + fx.MCAP_MAGIC)
    return len(fx.MCAP_MAGIC + fx.header_record())  # the chunk's byte offset


def test_a_compressed_chunk_decodes_or_its_compression_is_named(tmp_path):
    inner = fx.schema_record(1, PC2) + fx.channel_record(1, 1, "/points") + fx.message_record(1, 0, 1000000002, b"abc")
    path = tmp_path / "c.mcap"
    try:
        import lz4.frame as lz4_frame
    except ImportError:
        lz4_frame = None
    for name, compress in (("lz4", None if lz4_frame is None else lz4_frame.compress), ("zstd", _zstd_compress())):
        offset = _one_chunk_file(path, fx.chunk_record(inner, compression=name, stored=inner if compress is None else compress(inner)))
        assert rosbag2.valid_bag(path)
        if compress is None:
            with pytest.raises(ValueError, match=f"byte offset {offset} is compressed with '{name}'.*uncompressed"):
                rosbag2.Bag(path)
        else:
            assert _payloads(rosbag2.Bag(path)) == [("/points", PC2, (1, 2), b"abc")]
    _one_chunk_file(path, fx.chunk_record(inner, compression="brotli", stored=inner))
    with pytest.raises(ValueError, match="'brotli'"):
        rosbag2.Bag(path)


def test_a_chunk_crc_mismatch_and_a_wrong_size_are_refused_with_the_offset(tmp_path):
    inner = fx.schema_record(1, PC2) + fx.channel_record(1, 1, "/points") + fx.message_record(1, 0, 1000000002, b"abc")
    path = tmp_path / "c.mcap"
    _one_chunk_file(path, fx.chunk_record(inner))
    assert _payloads(rosbag2.Bag(path)) == [("/points", PC2, (1, 2), b"abc")]  # the right CRC
    _one_chunk_file(path, fx.chunk_record(inner, crc=0))
    assert _payloads(rosbag2.Bag(path)) == [("/points", PC2, (1, 2), b"abc")]  # 0: not computed, not checked
    offset = _one_chunk_file(path, fx.chunk_record(inner, crc=zlib.crc32(inner) ^ 1))
    with pytest.raises(ValueError, match=f"chunk at byte offset {offset} has CRC"):
        rosbag2.Bag(path)
    offset = _one_chunk_file(path, fx.chunk_record(inner, size=len(inner) + 1))
    with pytest.raises(ValueError, match=f"chunk at byte offset {offset} holds {len(inner)} bytes, its header says {len(inner) + 1}"):
        rosbag2.Bag(path)


@pytest.mark.parametrize("kw", [dict(), dict(chunk_size=3, summary=True)], ids=["unchunked", "chunked_with_summary"])
def test_mcap_truncation_next_to_every_record_boundary_is_refused_with_the_offset(tmp_path, kw):
    msgs, _ = _eight()
    path = tmp_path / "full.mcap"
    bounds = fx.write_mcap(path, TOPICS, msgs, **kw)
    raw = path.read_bytes()
    assert bounds[0] == 8 and bounds[-1] == len(raw) - 8 and len(bounds) > 8
    cut = tmp_path / "cut.mcap"
    for b in bounds[1:]:  # (a cut in the opening magic leaves no MCAP file at all)
        for end in (b - 1, b, b + 1):
            cut.write_bytes(raw[:end])
            with pytest.raises(ValueError, match=r"cut.mcap.*truncated.*byte offset \d+"):
                rosbag2.Bag(cut)
    # a chunk whose inner records are cut short, and a chunk that promises more bytes than its record holds
    inner = fx.schema_record(1, PC2) + fx.channel_record(1, 1, "/points") + fx.message_record(1, 0, 1000000002, b"abc")
    offset = _one_chunk_file(cut, fx.chunk_record(inner[:-1]))
    at = offset + len(fx.chunk_record(b"")) + len(inner) - len(fx.message_record(1, 0, 1000000002, b"abc"))  # an uncompressed chunk's records are read where they lie in the file
    with pytest.raises(ValueError, match=f"cut.mcap: truncated record 0x05 at byte offset {at} "):
        rosbag2.Bag(cut)
    short = fx.chunk_record(inner)
    _one_chunk_file(cut, fx.record(0x06, short[9:-1]))
    with pytest.raises(ValueError, match=r"truncated chunk record \(records\).*byte offset \d+"):
        rosbag2.Bag(cut)
    # a record length that runs over the closing magic
    body = fx.MCAP_MAGIC + fx.header_record() + struct.pack("<BQ", 0x05, 1 << 40) + b"\x00" * 30 + fx.MCAP_MAGIC
    cut.write_bytes(body)
    with pytest.raises(ValueError, match=r"truncated record 0x05 at byte offset \d+"):
        rosbag2.Bag(cut)


def test_a_missing_trailing_magic_is_refused(tmp_path):
    path = tmp_path / "m.mcap"
    path.write_bytes(MCAP_LITERAL[:-8])
    assert rosbag2.valid_bag(path)  # by its first bytes, as the issue of what a bag is says; reading it is refused
    with pytest.raises(ValueError, match="does not end with the MCAP magic"):
        rosbag2.Bag(path)
    path.write_bytes(MCAP_LITERAL[:-8] + b"\x89MCAP1\r\n")
    with pytest.raises(ValueError):
        rosbag2.Bag(path)
    path.write_bytes(b"\x89MCAP0\r\n")  # the magic alone is the head, not also the tail
    with pytest.raises(ValueError, match="does not end with the MCAP magic"):
        rosbag2.Bag(path)


# ---------------------------------------------------------------------------------------------- the command line's host logic
XYZI = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")])


def _args(*argv):
    return preprocess_ros2.build_parser().parse_args(preprocess_ros1._attach_values(list(argv)))


def test_defaults_are_the_references():
    a = _args("src", "dst")
    assert (a.data_path, a.dst_path, a.intensity_channel, a.camera_model, a.voxel_resolution, a.min_distance, a.k_neighbors) == ("src", "dst", "auto", "auto", 0.002, 1.0, 20)
    assert not a.auto_topic and not a.dynamic_lidar_integration and not a.verbose and a.bag_id is None and a.first_n_bags is None and a.device == 0
    assert (a.target_num_points, a.seed, a.lru_thresh) == (10000, 0, 100)  # preprocess_dynamic's
    a = _args("src", "dst", "-a", "-d", "-i", "reflectivity", "--target_num_points", "2000", "--seed", "7", "--lru_thresh", "0")
    assert a.auto_topic and a.dynamic_lidar_integration and (a.intensity_channel, a.target_num_points, a.seed, a.lru_thresh) == ("reflectivity", 2000, 7, 0)
    assert "refused" not in preprocess_ros2.build_parser().format_help() and "refused" in preprocess_ros1.build_parser().format_help()


def test_auto_topic_selection_by_ros2_type_names(tmp_path):
    channels = [(0, "/cam/info", INFO), (1, "/cam/image", IMG), (2, "/lidar/points", PC2), (3, "/cam2/image/compressed", CIMG), (4, "/imu", "sensor_msgs/msg/Imu"), (5, "/lidar2/points", PC2)]
    msgs = [(c[0], 10 + c[0], b"x") for c in channels]
    fx.write_mcap(tmp_path / "a.mcap", channels, msgs, chunk_size=4)
    fx.write_sqlite3(tmp_path / "a.db3", [(c[0] + 1,) + c[1:] for c in channels], [])
    for name in ("a.mcap", "a.db3"):
        bag = rosbag2.Bag(tmp_path / name)
        warn, log = [], []
        assert preprocess_ros1.get_topics(_args("s", "d", "-a"), bag, log=log.append, warn=warn.append) == ("/cam/info", "/cam2/image/compressed", "/lidar2/points")  # the last wins
        assert warn == ["warning: bag constains multiple image topics!!", "warning: bag constains multiple points topics!!"]
        assert "- /imu : sensor_msgs/msg/Imu" in log and log[0] == f"topics in {tmp_path / name}:"


def test_intensity_channel_priority(tmp_path):
    def bag_with(names, name):
        dt = np.dtype([(n, "<f4") for n in names])
        fx.write_mcap(tmp_path / name, [(0, "/p", PC2)], [(0, 1, fx.cloud_from_struct((1, 0), np.zeros(2, dtype=dt)))])
        return rosbag2.Bag(tmp_path / name)

    auto = _args("s", "d")
    assert preprocess_ros1.get_intensity_channel(auto, bag_with(["x", "y", "z", "intensity", "reflectivity"], "1.mcap"), "/p", reader=rosbag2) == "reflectivity"
    assert preprocess_ros1.get_intensity_channel(auto, bag_with(["x", "y", "z", "reflectivity", "intensity"], "2.mcap"), "/p", reader=rosbag2) == "reflectivity"
    assert preprocess_ros1.get_intensity_channel(auto, bag_with(["x", "y", "z", "intensity"], "3.mcap"), "/p", reader=rosbag2) == "intensity"
    assert preprocess_ros1.get_intensity_channel(_args("s", "d", "-i", "ambient"), bag_with(["x", "y", "z", "intensity"], "4.mcap"), "/p", reader=rosbag2) == "ambient"
    with pytest.raises(ValueError, match="failed to determine point intensity channel automatically.*'/p'.*5.mcap"):
        preprocess_ros1.get_intensity_channel(auto, bag_with(["x", "y", "z", "ring"], "5.mcap"), "/p", reader=rosbag2)


def test_image_or_compressed_image_is_chosen_by_the_recorded_type(tmp_path):
    """The reference looks for "compressed" in the topic NAME; here a raw image on a topic named .../compressed and a compressed one on a
    topic named otherwise both decode"""
    gray = np.arange(60, dtype=np.uint8).reshape(6, 10)
    png = tmp_path / "g.png"
    dataset.write_png_gray(png, gray)
    fx.write_mcap(tmp_path / "a.mcap", [(0, "/raw/compressed", IMG), (1, "/packed", CIMG)], [(0, 1, fx.image((1, 0), gray, "mono8")), (1, 2, fx.compressed_image((1, 0), "png", png.read_bytes()))])
    bag = rosbag2.Bag(tmp_path / "a.mcap")
    assert np.array_equal(preprocess_ros1.get_image(bag, "/raw/compressed", reader=rosbag2), gray) and np.array_equal(preprocess_ros1.get_image(bag, "/packed", reader=rosbag2), gray)
    args = _args("s", "d", "--camera_model", "equirectangular")
    assert preprocess_ros1.get_camera_params(args, bag, "", "/packed", log=lambda m: None, reader=rosbag2) == ("equirectangular", (10, 6), [10.0, 6.0], [])


def test_statuses_usage_and_what_a_directory_entry_counts_as(tmp_path, capsys, monkeypatch):
    assert preprocess_ros2.main([str(tmp_path), str(tmp_path / "dst")]) == 1
    assert "error: no input bags!!" in capsys.readouterr().err
    assert preprocess_ros2.main([]) == 0  # the usage (preprocess.cpp:73-76)
    out = capsys.readouterr().out
    assert "data_path" in out and "preprocess_ros2" in out
    # a ROS1 bag, a text file and a fake .db3 are ignored: still no input bags
    cloud = np.zeros(2, dtype=XYZI)
    fx1.write_bag(tmp_path / "c.bag", [(0, "/p", "sensor_msgs/PointCloud2")], [(0, (1, 0), fx1.cloud_from_struct((1, 0), cloud))])
    (tmp_path / "notes.txt").write_text("not a bag")
    (tmp_path / "ros2.db3").write_bytes(b"SQLite format 3\x00" + b"\x00" * 100)
    assert preprocess_ros1.find_bags(str(tmp_path), rosbag2) == []
    assert preprocess_ros2.main([str(tmp_path), str(tmp_path / "dst"), "-d"]) == 1
    assert "error: no input bags!!" in capsys.readouterr().err
    # a directory bag, a bare .mcap and a bare .db3 are bags, sorted by name
    fx.write_sqlite3_dir(tmp_path / "b_dir", [(1, "/p", PC2)], [(1, 1000000000, fx.cloud_from_struct((1, 0), cloud))])
    fx.write_mcap(tmp_path / "a.mcap", [(0, "/p", PC2)], [(0, 1000000000, fx.cloud_from_struct((1, 0), cloud))])
    fx.write_sqlite3(tmp_path / "d.db3", [(1, "/p", PC2)], [(1, 1000000000, fx.cloud_from_struct((1, 0), cloud))])
    assert [p.rsplit("/", 1)[1] for p in preprocess_ros1.find_bags(str(tmp_path), rosbag2)] == ["a.mcap", "b_dir", "d.db3"]
    assert [p.rsplit("/", 1)[1] for p in preprocess_ros1.find_bags(str(tmp_path))] == ["c.bag"]
    # a bag without the image topic: status 1, the topic and the bag named, before any GPU work
    assert preprocess_ros2.main([str(tmp_path), str(tmp_path / "dst"), "--points_topic", "/p", "--image_topic", "/image", "--camera_model", "equirectangular"]) == 1
    err = capsys.readouterr().err
    assert "image_topic='/image'" in err and "a.mcap" in err and not (tmp_path / "dst").exists()
    # -d reaches the dynamic factory, with preprocess_dynamic's checks; without -d the static one stays
    calls = []
    monkeypatch.setattr(preprocess_ros1, "run", lambda args, **kw: calls.append(kw))
    assert preprocess_ros2.main([str(tmp_path), "dst", "-d", "--target_num_points", "2000", "--seed", "7", "--k_neighbors", "10"]) == 0
    assert preprocess_ros2.main([str(tmp_path), "dst"]) == 0
    factory = calls[0]["integrator_factory"]
    assert isinstance(factory, functools.partial) and factory.func is odometry.DynamicPointCloudIntegrator
    assert factory.keywords == {"k_neighbors": 10, "target_num_points": 2000, "seed": 7, "lru_thresh": 100}
    assert calls[0]["reader"] is rosbag2 and calls[1] == {"reader": rosbag2}
    assert preprocess_ros2.main([str(tmp_path), "dst", "-d", "--k_neighbors", "40"]) == 1 and len(calls) == 2
    assert "2..32 neighbours" in capsys.readouterr().err
    assert preprocess_ros2.main([str(tmp_path), "dst", "--k_neighbors", "40"]) == 0  # unused without -d, as in preprocess_ros1


def test_clouds_the_reference_would_crash_on_are_refused_with_the_ros1_wording(tmp_path):
    cases = [
        (fx.cloud_from_struct((1, 0), np.zeros(2, dtype=[("x", "<f4"), ("y", "<f4"), ("intensity", "<f4")])), "missing point coordinate fields"),
        (fx.cloud_from_struct((1, 0), np.zeros(2, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("ring", "<u2")])), "no intensity channel 'intensity'"),
        (fx.cloud_from_struct((1, 0), np.zeros(2, dtype=XYZI), is_bigendian=1), "big-endian"),
        (fx.cloud_from_struct((1, 0), np.zeros(2, dtype=XYZI), width=3), "32 data bytes for 3 x 1 points of 16 bytes"),
    ]
    for k, (payload, what) in enumerate(cases):
        fx.write_sqlite3(tmp_path / f"{k}.db3", [(1, "/p", PC2)], [(1, 1, payload)])
        with pytest.raises(ValueError, match=f"{what}.*'/p'.*{k}.db3"):
            preprocess_ros1.integrate_bag(_args("s", "d"), rosbag2.Bag(tmp_path / f"{k}.db3"), "/p", "intensity", RecordingIntegrator(), reader=rosbag2)


# ---------------------------------------------------------------------------------------------- route identity on the host
class RecordingIntegrator:
    """Records what the command line hands the integrator"""

    def __init__(self):
        self.frames = []

    def insert_cloud2(self, cloud, channel):
        self.frames.append((tuple(cloud.fields), cloud.point_step, bytes(cloud.data), channel, cloud.width, cloud.height, cloud.stamp))
        return 1


def test_the_three_routes_hand_the_integrator_the_same_frames(tmp_path):
    """Three frames and one whose stamp rewinds, written as a ROS1 bag, a sqlite3 bag and an MCAP file"""
    rng = np.random.default_rng(5)
    dt = np.dtype({"names": ["x", "y", "z", "intensity", "tag", "timestamp"], "formats": ["<f4", "<f4", "<f4", "<f4", "u1", "<f8"], "offsets": [0, 4, 8, 12, 16, 18], "itemsize": 26})
    stamps = [(100, 0), (100, 100000000), (100, 50000000), (100, 200000000)]  # the third rewinds
    records = []
    for n in (7, 5, 3, 4):
        rec = np.zeros(n, dtype=dt)
        rec["x"], rec["intensity"], rec["timestamp"] = rng.normal(size=n), rng.uniform(0, 255, n), np.linspace(0.0, 0.09, n)
        records.append(rec)
    times = [(10, 0), (11, 0), (12, 0), (13, 0)]
    gray = np.zeros((4, 4), dtype=np.uint8)
    fx1.write_bag(tmp_path / "a.bag", [(0, "/p", "sensor_msgs/PointCloud2"), (1, "/image", "sensor_msgs/Image")],
                  [(1, (9, 0), fx1.image((9, 0), gray, "mono8"))] + [(0, t, fx1.cloud_from_struct(s, r, frame_id="livox_frame")) for t, s, r in zip(times, stamps, records)])
    blobs = [(fx.nanoseconds(t), fx.cloud_from_struct(s, r, frame_id="livox_frame")) for t, s, r in zip(times, stamps, records)]
    fx.write_sqlite3_dir(tmp_path / "a_dir", [(1, "/p", PC2), (2, "/image", IMG)], [(2, 9000000000, fx.image((9, 0), gray, "mono8"))] + [(1, t, b) for t, b in blobs], split=2)
    fx.write_mcap(tmp_path / "a.mcap", [(1, "/p", PC2), (2, "/image", IMG)], [(2, 9000000000, fx.image((9, 0), gray, "mono8"))] + [(1, t, b) for t, b in blobs], chunk_size=2, summary=True)
    got = {}
    for name, reader in (("a.bag", rosbag1), ("a_dir", rosbag2), ("a.mcap", rosbag2)):
        stub, warn = RecordingIntegrator(), []
        counts = preprocess_ros1.integrate_bag(_args("s", "d"), reader.Bag(tmp_path / name), "/p", "intensity", stub, warn=warn.append, reader=reader)
        got[name] = (counts, stub.frames, warn)
    counts, frames, warn = got["a.bag"]
    assert counts == (3, 1, 3) and [f[6] for f in frames] == [stamps[0], stamps[1], stamps[3]] and [f[2] for f in frames] == [records[k].tobytes() for k in (0, 1, 3)]
    assert "warning: skip frame with an invalid timestamp!!" in warn
    assert got["a_dir"] == got["a.bag"] and got["a.mcap"] == got["a.bag"]
