"""End-to-end GPU tests of the raw image encodings: a bag whose image topic carries a bayer_rggb8 mosaic or a mono16 image goes through
preprocess_ros1 (ROS1 bag) and preprocess_ros2 (sqlite3 directory, MCAP file) to the very directory that the same bag gives with the
mono8 image of the oracle's conversion (tests/raw_image_oracle.py) in its place, byte for byte; an encoding outside the converted set
is still refused by name.  preprocess_dynamic takes its image through the same preprocess_ros1.get_image."""
import filecmp
import json
import os

import numpy as np
import pytest

import raw_image_oracle as ro
import rosbag1_fixture as fx1
import rosbag2_fixture as fx2
from direct_visual_lidar_calibration_amd import preprocess_dynamic, preprocess_ros1, preprocess_ros2, synth

pytestmark = pytest.mark.gpu
ARGS = ["--voxel_resolution", "0.05", "--min_distance", "0.5", "-a"]
TOPIC_NAMES = ("/camera/camera_info", "/camera/image_raw", "/points")
SUFFIXES = (".ply", ".png", "_lidar_intensities.png", "_lidar_indices.png")


class Material:
    """The scene's camera and two clouds, and its image as a bayer_rggb8 mosaic and as a mono16 image, each with the oracle's mono8"""

    def __init__(self):
        scene = synth.make_scene("pinhole_vga", num_points=6000, seed=30)
        self.rec = np.zeros(len(scene.points), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")])
        self.rec["x"], self.rec["y"], self.rec["z"], self.rec["intensity"] = scene.points[:, 0], scene.points[:, 1], scene.points[:, 2], scene.intensities
        K = [scene.intrinsics[0], 0.0, scene.intrinsics[2], 0.0, scene.intrinsics[1], scene.intrinsics[3], 0.0, 0.0, 1.0]
        self.info = (scene.width, scene.height, scene.model, list(scene.distortion), K)
        h, w = scene.image_u8.shape
        yy, xx = np.mgrid[0:h, 0:w]
        deep = (scene.image_u8.astype(np.int64) * 257 + (xx * 7 + yy * 3) % 257 - 128).clip(0, 65535).astype("<u2")
        self.images = {"bayer_rggb8": np.ascontiguousarray(scene.image_u8), "mono16": deep.view(np.uint8).reshape(h, w, 2)}
        self.mono8 = {enc: ro.to_mono8(a.tobytes(), w, h, a.size // h, enc) for enc, a in self.images.items()}
        assert not np.array_equal(self.mono8["bayer_rggb8"], scene.image_u8) and self.mono8["mono16"].std() > 10

    def clouds(self):
        return [((100, 0), self.rec[:3000]), ((100, 100000000), self.rec[3000:])]

    def write_ros1(self, path, image, encoding):
        msgs = [(0, (50, 0), fx1.camera_info((50, 0), *self.info)), (1, (50, 1), fx1.image((50, 1), image, encoding))] + [(2, t, fx1.cloud_from_struct(t, r)) for t, r in self.clouds()]
        fx1.write_bag(path, list(zip(range(3), TOPIC_NAMES, ("sensor_msgs/CameraInfo", "sensor_msgs/Image", "sensor_msgs/PointCloud2"))), msgs)

    def ros2(self, image, encoding):
        topics = list(zip((1, 2, 3), TOPIC_NAMES, (fx2.INFO, fx2.IMG, fx2.PC2)))
        msgs = [(1, fx2.nanoseconds((50, 0)), fx2.camera_info((50, 0), *self.info)), (2, fx2.nanoseconds((50, 1)), fx2.image((50, 1), image, encoding))]
        return topics, msgs + [(3, fx2.nanoseconds(t), fx2.cloud_from_struct(t, r)) for t, r in self.clouds()]


@pytest.fixture(scope="module")
def material(tmp_path_factory):
    """... and what preprocess_ros1 writes for the ROS1 bag ``bags/a.bag`` with each oracle image as mono8: ``want[encoding]``"""
    m = Material()
    m.root = tmp_path_factory.mktemp("raw_e2e")
    (m.root / "bags").mkdir()
    m.want = {}
    for enc in m.images:
        m.write_ros1(m.root / "bags" / "a.bag", m.mono8[enc], "mono8")
        m.want[enc] = str(m.root / ("want_" + enc))
        assert preprocess_ros1.main([str(m.root / "bags"), m.want[enc]] + ARGS) == 0
    return m


def _same_directories(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and len(names) >= 5
    match, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert sorted(match) == names and not mismatch and not errors, (mismatch, errors)


@pytest.mark.parametrize("encoding", ["bayer_rggb8", "mono16"])
def test_preprocess_ros1_on_a_raw_image_equals_preprocess_ros1_on_the_oracles_mono8(material, tmp_path, encoding):
    material.write_ros1(material.root / "bags" / "a.bag", material.images[encoding], encoding)  # the same path as the reference's: calib.json records it
    assert preprocess_ros1.main([str(material.root / "bags"), str(tmp_path / "got")] + ARGS) == 0
    _same_directories(str(tmp_path / "got"), material.want[encoding])


@pytest.mark.parametrize("kind", ["sqlite3", "mcap"])
@pytest.mark.parametrize("encoding", ["bayer_rggb8", "mono16"])
def test_preprocess_ros2_on_a_raw_image_equals_the_ros1_route_on_the_oracles_mono8(material, tmp_path, encoding, kind):
    src, dst = tmp_path / "ros2", str(tmp_path / "got")
    src.mkdir()
    topics, msgs = material.ros2(material.images[encoding], encoding)
    if kind == "sqlite3":
        fx2.write_sqlite3_dir(src / "a", topics, msgs, split=3)
        name = "a"
    else:
        fx2.write_mcap(src / "a.mcap", topics, msgs, chunk_size=2, summary=True)
        name = "a.mcap"
    assert preprocess_ros2.main([str(src), dst] + ARGS) == 0
    assert sorted(os.listdir(dst)) == sorted([name + s for s in SUFFIXES] + ["calib.json"])
    for suffix in SUFFIXES:
        assert filecmp.cmp(os.path.join(dst, name + suffix), os.path.join(material.want[encoding], "a.bag" + suffix), shallow=False), suffix
    with open(os.path.join(dst, "calib.json")) as f, open(os.path.join(material.want[encoding], "calib.json")) as g:
        got, ref = json.load(f), json.load(g)
    assert got["meta"].pop("data_path") == str(src) and got["meta"].pop("bag_names") == [name] and ref["meta"].pop("data_path") and ref["meta"].pop("bag_names") == ["a.bag"]
    assert got == ref


def test_an_encoding_outside_the_converted_set_is_still_refused_by_name(material, tmp_path, capsys):
    src = tmp_path / "bags"
    src.mkdir()
    material.write_ros1(src / "a.bag", material.images["mono16"], "16UC1")
    assert preprocess_ros1.main([str(src), str(tmp_path / "dst")] + ARGS) == 1
    err = capsys.readouterr().err
    assert "encoding '16UC1' is not converted here" in err and "/camera/image_raw" in err and "a.bag" in err


def test_preprocess_dynamic_takes_its_image_through_the_same_call():
    assert preprocess_dynamic.preprocess_ros1 is preprocess_ros1 and preprocess_ros2.preprocess_ros1 is preprocess_ros1
