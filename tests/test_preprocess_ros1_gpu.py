"""GPU test of the preprocess_ros1 command end to end: two ROS1 bags written by tests/rosbag1_fixture.py in, a preprocessed directory
out, checked against the oracle of tests/preprocess_oracle.py on a numpy decode of the same bytes and read back through
dataset.load_dataset."""
import os

import numpy as np
import pytest

import preprocess_oracle
import rosbag1_fixture as fx
from direct_visual_lidar_calibration_amd import dataset, nid, pose, preprocess, preprocess_ros1, render, synth

RES, MIN_D = 0.01, 0.5
OUSTER = np.dtype({"names": ["x", "y", "z", "intensity", "t", "reflectivity", "ring", "ambient", "range"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u4", "<u2", "<u2", "<u2", "<u4"],
                   "offsets": [0, 4, 8, 16, 20, 24, 26, 28, 32], "itemsize": 48})
PC2, IMG, INFO = "sensor_msgs/PointCloud2", "sensor_msgs/Image", "sensor_msgs/CameraInfo"


def _frame(points, intensities, rng, nan_rows):
    """An Ouster-like frame of the points with ``nan_rows`` extra records mixed in whose x, y or z is not finite"""
    n = len(points) + nan_rows
    rec = np.zeros(n, dtype=OUSTER)
    where = np.sort(rng.choice(n, nan_rows, replace=False))
    good = np.setdiff1d(np.arange(n), where)
    rec["x"][good], rec["y"][good], rec["z"][good] = points[:, 0], points[:, 1], points[:, 2]
    rec["reflectivity"][good] = np.rint(intensities * 65535.0)
    rec["intensity"] = rng.uniform(0, 1, n)  # the channel that must NOT be chosen
    rec["x"][where], rec["y"][where], rec["z"][where] = rng.uniform(2, 5, (3, nan_rows))
    for k, i in enumerate(where):
        rec["xyz"[k % 3]][i] = (np.nan, np.inf, -np.inf)[(k // 3) % 3]
    rec["t"] = np.linspace(0, 0.09e9, n).astype(np.uint32)  # relative per-point times [ns]
    return rec


def _write_bag(path, scene, lo, hi, image_msg, rng):
    cuts = [lo, lo + (hi - lo) // 3, lo + 2 * (hi - lo) // 3 + 7, hi]
    frames = [_frame(scene.points[a:b, :3], scene.intensities[a:b], rng, nan_rows=9) for a, b in zip(cuts[:-1], cuts[1:])]
    ghost = _frame(scene.points[lo:lo + 500, :3] + [100.0, 0.0, 0.0], scene.intensities[lo:lo + 500], rng, nan_rows=0)  # would show up 100 m away
    K = [scene.intrinsics[0], 0.0, scene.intrinsics[2], 0.0, scene.intrinsics[1], scene.intrinsics[3], 0.0, 0.0, 1.0]
    msgs = [(0, (50, 0), fx.camera_info((50, 0), scene.width, scene.height, scene.model, list(scene.distortion), K)), (1, (50, 1), image_msg),
            (2, (100, 0), fx.cloud_from_struct((100, 0), frames[0])), (2, (100, 100000000), fx.cloud_from_struct((100, 100000000), frames[1])),
            (2, (100, 150000000), fx.cloud_from_struct((100, 50000000), ghost)),  # its header stamp rewinds: skipped
            (2, (100, 200000000), fx.cloud_from_struct((100, 200000000), frames[2]))]
    fx.write_bag(path, [(0, "/camera/camera_info", INFO), (1, "/camera/image", IMG), (2, "/os_cloud_node/points", PC2)], msgs, compression="bz2", chunk_size=2, index=True)
    return frames


@pytest.mark.gpu
def test_two_bags_to_a_directory_calibrate_reads(tmp_path, capsys):
    scene = synth.make_scene("pinhole_vga", 20000)
    rng = np.random.default_rng(17)
    src, dst = tmp_path / "bags", str(tmp_path / "data")
    src.mkdir()
    (src / "README.txt").write_text("not a bag")
    raw = (scene.image_u8 // 2 + 40).astype(np.uint8)
    bgr = np.stack([255 - raw, raw // 2 + 10, raw], axis=2)
    b, g, r = (bgr[:, :, k].astype(np.int64) for k in range(3))
    gray_of_bgr = ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)
    frames = {"a.bag": _write_bag(src / "a.bag", scene, 0, 10000, fx.image((50, 1), raw, "mono8"), rng),
              "b.bag": _write_bag(src / "b.bag", scene, 10000, 20000, fx.image((50, 1), bgr, "bgr8"), rng)}
    images = {"a.bag": raw, "b.bag": gray_of_bgr}

    assert preprocess_ros1.main([str(src), dst, "--voxel_resolution", str(RES), "--min_distance", str(MIN_D), "-a"]) == 0
    captured = capsys.readouterr()
    assert captured.err.count("warning: skip frame with an invalid timestamp!!") == 2 and "intensity_channel: reflectivity" in captured.out
    assert captured.out.count("frames=3 skipped_frames=1 skipped_points=27") == 2

    config, bags = dataset.load_dataset(dst)
    assert config["meta"] == {"data_path": str(src), "camera_info_topic": "/camera/camera_info", "image_topic": "/camera/image", "points_topic": "/os_cloud_node/points",
                              "intensity_channel": "reflectivity", "bag_names": ["a.bag", "b.bag"]}
    assert config["camera"] == {"camera_model": scene.model, "intrinsics": [float(v) for v in scene.intrinsics], "distortion_coeffs": [float(v) for v in scene.distortion]}
    assert nid.create_camera(*dataset.camera_from_calib(config)) is not None and [b.bag_name for b in bags] == ["a.bag", "b.bag"]

    clouds = {}
    for bag in bags:
        name = bag.bag_name
        assert np.array_equal(bag.image, preprocess.equalize_hist(images[name]))
        # the oracle: decode, finite filter, gate, last insert wins, then the rank equalisation
        filtered = []
        for rec in frames[name]:
            pts = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float64)
            ok = np.isfinite(pts).all(axis=1)
            assert (~ok).sum() == 9
            filtered.append((pts[ok], rec["reflectivity"].astype(np.float64)[ok]))
        rec_o, _, _, _ = preprocess_oracle.winners_numpy(filtered, RES, MIN_D)
        assert 5000 < len(rec_o) <= 10000 and bag.num_points == len(rec_o)
        assert np.array_equal(np.asarray(bag.xyz_f32).view(np.uint32), rec_o[:, :3].view(np.uint32))
        assert (np.asarray(bag.xyz_f32)[:, 0] < 50.0).all()  # the rewound frame is absent
        want = render.equalize_intensities(rec_o[:, 3].astype(np.float64), device=0)
        assert np.array_equal(np.asarray(bag.intensities_f32), want.astype(np.float32))
        clouds[name] = (bag.points, want)

    # the LiDAR images: the camera the FIRST bag's field of view selects, for both bags
    fov = preprocess.estimate_lidar_fov(clouds["a.bag"][0], device=0)
    model, intr, size, T_lidar_camera = preprocess.lidar_camera(fov)
    proj = nid.create_camera(model, intr, [])
    for name, (points, intensities) in clouds.items():
        inten_img, idx_img = render.generate_lidar_image(proj, size, np.linalg.inv(T_lidar_camera), points, intensities, device=0)
        assert np.array_equal(dataset.read_png_gray(os.path.join(dst, name + "_lidar_intensities.png")), np.clip(np.rint(np.asarray(inten_img) * 255.0), 0, 255).astype(np.uint8))
        assert np.array_equal(pose.read_index_image(os.path.join(dst, name + "_lidar_indices.png")), idx_img) and (np.asarray(idx_img) >= 0).sum() > 1000
