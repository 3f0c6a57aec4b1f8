"""GPU tests of the ROS2 route: the same frames written as ROS1 bags and as ROS2 bags (sqlite3 directories, bare MCAP files, both by
tests/rosbag2_fixture.py) must come out of preprocess_ros2 exactly as they come out of preprocess_ros1 / preprocess_dynamic -- the ROS2
reader hands the device the very bytes the ROS1 reader does.  preprocess_ros1 itself is held to the oracle by
tests/test_preprocess_ros1_gpu.py, whose scene and frames these are.  No kernel is under test that the ROS1 route does not run; what is
new is where the records lie in host memory (anywhere in a mapped file) and the layouts ROS2 drivers publish."""
import filecmp
import json
import os

import numpy as np
import pytest

import preprocess_oracle
import rosbag1_fixture as fx1
import rosbag2_fixture as fx
from direct_visual_lidar_calibration_amd import dataset, odometry, preprocess, preprocess_dynamic, preprocess_ros1, preprocess_ros2, rosbag2, synth
from test_odometry_gpu import SPINNER, spinner_frames
from test_odometry_gpu import ARGS as DYNAMIC_ARGS
from test_preprocess_ros1_gpu import MIN_D, RES, _frame

pytestmark = pytest.mark.gpu
SUFFIXES = (".ply", ".png", "_lidar_intensities.png", "_lidar_indices.png")


# ---------------------------------------------------------------------------------------------- 1. static, end to end, three ways
def _content(scene, lo, hi, image, encoding, rng):
    """What one bag of tests/test_preprocess_ros1_gpu.py holds, not yet serialised: ``(camera_info arguments, image, encoding, [(record
    time, header stamp, records)])`` with three frames of 9 non-finite records each and one frame whose header stamp rewinds"""
    cuts = [lo, lo + (hi - lo) // 3, lo + 2 * (hi - lo) // 3 + 7, hi]
    frames = [_frame(scene.points[a:b, :3], scene.intensities[a:b], rng, nan_rows=9) for a, b in zip(cuts[:-1], cuts[1:])]
    ghost = _frame(scene.points[lo:lo + 500, :3] + [100.0, 0.0, 0.0], scene.intensities[lo:lo + 500], rng, nan_rows=0)
    K = [scene.intrinsics[0], 0.0, scene.intrinsics[2], 0.0, scene.intrinsics[1], scene.intrinsics[3], 0.0, 0.0, 1.0]
    clouds = [((100, 0), (100, 0), frames[0]), ((100, 100000000), (100, 100000000), frames[1]), ((100, 150000000), (100, 50000000), ghost), ((100, 200000000), (100, 200000000), frames[2])]
    return (scene.width, scene.height, scene.model, list(scene.distortion), K), image, encoding, clouds


TOPIC_NAMES = ("/camera/camera_info", "/camera/image", "/os_cloud_node/points")


def _write_ros1(path, content):
    info, image, encoding, clouds = content
    msgs = [(0, (50, 0), fx1.camera_info((50, 0), *info)), (1, (50, 1), fx1.image((50, 1), image, encoding))] + [(2, t, fx1.cloud_from_struct(s, rec)) for t, s, rec in clouds]
    fx1.write_bag(path, list(zip(range(3), TOPIC_NAMES, ("sensor_msgs/CameraInfo", "sensor_msgs/Image", "sensor_msgs/PointCloud2"))), msgs, compression="bz2", chunk_size=2, index=True)


def _ros2_messages(content):
    info, image, encoding, clouds = content
    return [(1, fx.nanoseconds((50, 0)), fx.camera_info((50, 0), *info)), (2, fx.nanoseconds((50, 1)), fx.image((50, 1), image, encoding))] + \
           [(3, fx.nanoseconds(t), fx.cloud_from_struct(s, rec, frame_id="os_sensor")) for t, s, rec in clouds]


ROS2_TOPICS = list(zip((1, 2, 3), TOPIC_NAMES, (fx.INFO, fx.IMG, fx.PC2)))


@pytest.fixture(scope="module")
def three_ways(tmp_path_factory):
    """The two bags as ROS1 files, sqlite3 directories (split over two .db3 files) and bare .mcap files, and preprocess_ros1's output"""
    root = tmp_path_factory.mktemp("three_ways")
    scene = synth.make_scene("pinhole_vga", 20000)
    rng = np.random.default_rng(17)
    raw = (scene.image_u8 // 2 + 40).astype(np.uint8)
    bgr = np.stack([255 - raw, raw // 2 + 10, raw], axis=2)
    contents = {"a": _content(scene, 0, 10000, raw, "mono8", rng), "b": _content(scene, 10000, 20000, bgr, "bgr8", rng)}
    for kind in ("ros1", "sqlite3", "mcap"):
        (root / kind).mkdir()
        (root / kind / "README.txt").write_text("not a bag")
    for name, content in contents.items():
        _write_ros1(root / "ros1" / (name + ".bag"), content)
        fx.write_sqlite3_dir(root / "sqlite3" / name, ROS2_TOPICS, _ros2_messages(content), split=3)
        fx.write_mcap(root / "mcap" / (name + ".mcap"), ROS2_TOPICS, _ros2_messages(content), chunk_size=2, summary=True)
        _write_ros1(root / "mcap" / (name + ".bag"), content)  # a ROS1 bag among the ROS2 ones is ignored
    want = str(root / "want")
    assert preprocess_ros1.main([str(root / "ros1"), want, "--voxel_resolution", str(RES), "--min_distance", str(MIN_D), "-a"]) == 0
    return root, want


@pytest.mark.parametrize("kind,names", [("sqlite3", ["a", "b"]), ("mcap", ["a.mcap", "b.mcap"])])
def test_static_end_to_end_equals_the_ros1_route_byte_for_byte(three_ways, tmp_path, capsys, kind, names):
    root, want = three_ways
    dst = str(tmp_path / "data")
    assert preprocess_ros2.main([str(root / kind), dst, "--voxel_resolution", str(RES), "--min_distance", str(MIN_D), "-a"]) == 0
    captured = capsys.readouterr()
    assert captured.err.count("warning: skip frame with an invalid timestamp!!") == 2 and "intensity_channel: reflectivity" in captured.out
    assert captured.out.count("frames=3 skipped_frames=1 skipped_points=27") == 2
    for name, ros1_name in zip(names, ["a.bag", "b.bag"]):
        for suffix in SUFFIXES:
            assert filecmp.cmp(os.path.join(dst, name + suffix), os.path.join(want, ros1_name + suffix), shallow=False), (name, suffix)
    assert sorted(os.listdir(dst)) == sorted([n + s for n in names for s in SUFFIXES] + ["calib.json"])
    with open(os.path.join(dst, "calib.json")) as f, open(os.path.join(want, "calib.json")) as g:
        got, ref = json.load(f), json.load(g)
    assert got["meta"].pop("data_path") == str(root / kind) and ref["meta"].pop("data_path") == str(root / "ros1")
    assert got["meta"].pop("bag_names") == names and ref["meta"].pop("bag_names") == ["a.bag", "b.bag"]
    assert got == ref and got["meta"]["points_topic"] == "/os_cloud_node/points"
    config, bags = dataset.load_dataset(dst)
    assert [b.bag_name for b in bags] == names and all(5000 < b.num_points <= 10000 for b in bags)


# ---------------------------------------------------------------------------------------------- 2. layouts ROS1 fixtures never had
LIVOX = np.dtype({"names": ["x", "y", "z", "intensity", "tag", "line", "timestamp"], "formats": ["<f4", "<f4", "<f4", "<f4", "u1", "u1", "<f8"], "offsets": [0, 4, 8, 12, 16, 17, 18], "itemsize": 26})
XYZ64 = np.dtype({"names": ["x", "y", "z", "intensity"], "formats": ["<f8", "<f8", "<f8", "u1"], "offsets": [0, 8, 16, 24], "itemsize": 25})


def _records(dtype, n, seed):
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, dtype=dtype)
    xyz = rng.uniform(-8.0, 8.0, size=(n, 3))
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    rec["intensity"] = rng.integers(0, 256, n)
    if "timestamp" in dtype.names:
        rec["timestamp"] = rng.permutation(n) * (0.1 / (n - 1))  # 0 and 0.1 both occur
        rec["tag"], rec["line"] = rng.integers(0, 256, n), rng.integers(0, 6, n)
    rec["x"][17], rec["y"][n // 2], rec["z"][n - 1] = np.nan, np.inf, -np.inf
    return rec


def _cloud_at_an_odd_address(tmp_path, rec):
    """The records as a decoded message whose ``data`` view starts at an ODD byte offset of the mapped MCAP file it was read from.
    Inside a CDR blob ``data`` follows its u32 count and so starts at a multiple of 4 -- no frame_id makes that odd; it is the blob that
    lies anywhere in a storage file.  A topic name one byte longer moves it by one byte: one of two names gives an odd offset."""
    for topic in ("/livox/lidar", "/livox/lidar2"):
        blob = fx.cloud_from_struct((100, 0), rec, frame_id="livox_frame")
        assert fx.data_offset(blob, rec.tobytes()) % 4 == 0
        path = tmp_path / f"{len(topic)}.mcap"
        fx.write_mcap(path, [(1, topic, fx.PC2)], [(1, fx.nanoseconds((100, 0)), blob)])
        bag = rosbag2.Bag(path)
        cloud = rosbag2.decode_pointcloud2(bag.first_message(topic, "PointCloud2").data)
        mapped = np.frombuffer(bag._stores[0].buf, dtype=np.uint8)
        assert np.shares_memory(cloud.data, mapped) and cloud.data.tobytes() == rec.tobytes()
        if (cloud.data.ctypes.data - mapped.ctypes.data) % 2 == 1:
            assert cloud.data.ctypes.data % 2 == 1  # (a mapping starts on a page)
            return cloud
    raise AssertionError("neither topic name put the records at an odd offset")


def _oracle(rec):
    pts = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float64)
    ok = np.isfinite(pts).all(axis=1)
    assert (~ok).sum() == 3
    rec_o, _, _, _ = preprocess_oracle.winners_numpy([(pts[ok], rec["intensity"].astype(np.float64)[ok])], 0.05, 2.0)
    return rec_o


@pytest.mark.parametrize("dtype", [LIVOX, XYZ64], ids=["livox_26_bytes", "float64_xyz_25_bytes"])
def test_unaligned_ros2_layouts_from_an_odd_address_equal_the_oracle_bit_for_bit(tmp_path, dtype):
    rec = _records(dtype, 3000, 31)
    cloud = _cloud_at_an_odd_address(tmp_path, rec)
    assert cloud.point_step == dtype.itemsize and [(f.name, f.offset) for f in cloud.fields] == [(n, dtype.fields[n][1]) for n in dtype.names]
    rec_o = _oracle(rec)
    assert 2000 < len(rec_o) < 3000
    static = preprocess.StaticPointCloudIntegrator(0.05, 2.0)
    try:
        assert static.insert_cloud2(cloud, "intensity") == 3
        got = static.get_records()
        seq = static.last_seq
        assert np.array_equal(got.view(np.uint32), rec_o.view(np.uint32))
    finally:
        static.close()
    if dtype is not LIVOX:
        return
    # the unaligned float64 time column, at identity poses: the deskewing insert is insert_cloud2, bit for bit
    field = (18, rosbag2.FLOAT64)
    grid = preprocess.StaticPointCloudIntegrator(0.05, 2.0)
    try:
        assert odometry.deskew_insert(grid, preprocess.cloud2_layout(cloud, "intensity"), "intensity", field, 1.0, 0.0, float(rec["timestamp"].max()), np.eye(4), np.eye(4)) == 3
        assert np.array_equal(grid.get_records().view(np.uint32), got.view(np.uint32)) and np.array_equal(grid.last_seq, seq)
    finally:
        grid.close()
    dynamic = odometry.DynamicPointCloudIntegrator(0.05, 2.0, 0, target_num_points=1000)
    try:
        assert dynamic.insert_cloud2_timed(cloud, "intensity", field, 1.0, 0.0) == 3
        assert all(np.array_equal(T, np.eye(4)) for T in dynamic.poses()[0])  # the first frame is not registered
        assert np.array_equal(dynamic.get_records().view(np.uint32), got.view(np.uint32)) and np.array_equal(dynamic.last_seq, seq)
    finally:
        dynamic.close()


# ---------------------------------------------------------------------------------------------- 3. dynamic, end to end
def test_dynamic_end_to_end_equals_preprocess_dynamic_byte_for_byte(tmp_path):
    frames = spinner_frames()[:4]
    image = np.random.default_rng(3).integers(0, 256, size=(48, 64)).astype(np.uint8)
    stamps = [(100, f * 100000000) for f in range(4)]
    (tmp_path / "ros1").mkdir(), (tmp_path / "ros2").mkdir()
    fx1.write_bag(tmp_path / "ros1" / "run.bag", [(0, "/camera/image", "sensor_msgs/Image"), (1, "/points", "sensor_msgs/PointCloud2")],
                  [(0, (50, 0), fx1.image((50, 0), image, "mono8"))] + [(1, s, fx1.cloud_from_struct(s, rec)) for s, rec in zip(stamps, frames)], chunk_size=4, index=True)
    fx.write_mcap(tmp_path / "ros2" / "run.mcap", [(1, "/camera/image", fx.IMG), (2, "/points", fx.PC2)],
                  [(1, fx.nanoseconds((50, 0)), fx.image((50, 0), image, "mono8"))] + [(2, fx.nanoseconds(s), fx.cloud_from_struct(s, rec)) for s, rec in zip(stamps, frames)], chunk_size=2)
    assert frames[0].dtype == SPINNER
    want, dst = str(tmp_path / "want"), str(tmp_path / "data")
    assert preprocess_dynamic.main([str(tmp_path / "ros1"), want, "--target_num_points", "2000"] + DYNAMIC_ARGS) == 0
    assert preprocess_ros2.main([str(tmp_path / "ros2"), dst, "-d", "--target_num_points", "2000"] + DYNAMIC_ARGS) == 0
    for suffix in SUFFIXES:
        assert filecmp.cmp(os.path.join(dst, "run.mcap" + suffix), os.path.join(want, "run.bag" + suffix), shallow=False), suffix
    with open(os.path.join(dst, "calib.json")) as f, open(os.path.join(want, "calib.json")) as g:
        got, ref = json.load(f), json.load(g)
    assert got["meta"].pop("data_path") != ref["meta"].pop("data_path") and (got["meta"].pop("bag_names"), ref["meta"].pop("bag_names")) == (["run.mcap"], ["run.bag"])
    assert got == ref and sorted(os.listdir(dst)) == sorted(["run.mcap" + s for s in SUFFIXES] + ["calib.json"])
    # -d did run the dynamic integrator: without it the same bag gives the smeared cloud of the static one
    static = str(tmp_path / "static")
    assert preprocess_ros2.main([str(tmp_path / "ros2"), static] + DYNAMIC_ARGS) == 0
    assert not filecmp.cmp(os.path.join(static, "run.mcap.ply"), os.path.join(dst, "run.mcap.ply"), shallow=False)
