"""GPU tests of the preprocess_map command end to end -- raw map + image in, a preprocessed directory out, read back through
dataset.VisualLiDARData -- and of estimate_lidar_fov on clouds of known extent."""
import math
import os

import numpy as np
import pytest

import oracle_lib
import preprocess_oracle
from direct_visual_lidar_calibration_amd import dataset, nid, pose, preprocess, preprocess_map, render, synth

RES = 0.05


def write_binary_pcd(path, xyz, intensities):
    rec = np.zeros(len(xyz), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")])
    rec["x"], rec["y"], rec["z"], rec["intensity"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], intensities
    with open(path, "wb") as f:
        f.write(f"VERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\nWIDTH {len(xyz)}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(xyz)}\nDATA binary\n".encode())
        f.write(rec.tobytes())


@pytest.mark.gpu
def test_map_and_image_to_a_directory_calibrate_reads(tmp_path, capsys):
    scene = synth.make_scene("pinhole_vga", num_points=60000, seed=30)
    raw_image = (scene.image_u8 // 2 + 40).astype(np.uint8)  # the scene's image with its equalisation undone: 128 grey levels in [40, 167]
    map_ply, map_pcd, image_png = str(tmp_path / "map.ply"), str(tmp_path / "map.pcd"), str(tmp_path / "image.png")
    dataset.write_ply(map_ply, scene.points, scene.intensities)
    xyz32, inten32 = dataset.read_ply_float32(map_ply)
    write_binary_pcd(map_pcd, xyz32, inten32)
    dataset.write_png_gray(image_png, raw_image)
    dst = str(tmp_path / "data")
    intr = ",".join(repr(float(v)) for v in scene.intrinsics)
    dist = ",".join(repr(float(v)) for v in scene.distortion)
    argv = ["--image_path", image_png, "--camera_model", scene.model, "--camera_intrinsics", intr, "--camera_distortion_coeffs", dist, "--voxel_resolution", str(RES)]
    assert preprocess_map.main(argv + ["--map_path", map_ply, "--dst_path", dst]) == 0
    out = capsys.readouterr().out

    # the oracle's side: the voxel winners of the float32 map (min_distance is not applied), then the rank equalisation
    o = preprocess_oracle.Integrator(RES, 0.0)
    o.insert(xyz32, inten32)
    rec_o, _, _ = o.winners()
    m = len(rec_o)
    assert f"map_points=60000 filtered={m}" in out and "LiDAR FoV: " in out and 1000 < m < 60000

    config = dataset.read_calib(dst)
    assert config["meta"] == {"data_path": map_ply, "camera_info_topic": "N/A", "image_topic": "N/A", "points_topic": "N/A", "intensity_channel": "N/A", "bag_names": ["000000"]}
    assert config["camera"] == {"camera_model": scene.model, "intrinsics": [float(v) for v in scene.intrinsics], "distortion_coeffs": [float(v) for v in scene.distortion]}
    assert np.array_equal(dataset.read_png_gray(os.path.join(dst, "000000.png")), preprocess.equalize_hist(raw_image))

    bag = dataset.VisualLiDARData(dst, "000000")
    assert bag.xyz_f32 is not None and bag.num_points == m
    assert np.array_equal(np.asarray(bag.xyz_f32).view(np.uint32), rec_o[:, :3].view(np.uint32))
    want_inten = render.equalize_intensities(rec_o[:, 3].astype(np.float64), device=0)
    assert np.array_equal(np.asarray(bag.intensities_f32), want_inten.astype(np.float32)) and np.array_equal(bag.intensities, want_inten)

    # the LiDAR images: the size the FoV rule gives, indices that name a point which projects into their pixel
    fov = preprocess.estimate_lidar_fov(bag.points, device=0)
    assert f"LiDAR FoV: {math.degrees(fov):g}[deg]" in out
    model, lidar_intr, size, T_lidar_camera = preprocess.lidar_camera(fov)
    inten_img = dataset.read_png_gray(os.path.join(dst, "000000_lidar_intensities.png"))
    idx = pose.read_index_image(os.path.join(dst, "000000_lidar_indices.png"))
    assert inten_img.shape == (size[1], size[0]) and idx.shape == (size[1], size[0])
    assert ((idx == -1) | ((idx >= 0) & (idx < m))).all()
    vs, us = np.nonzero(idx >= 0)
    assert len(vs) > 1000
    T = np.linalg.inv(T_lidar_camera)
    pc = bag.points[idx[vs, us], :3] @ T[:3, :3].T + T[:3, 3]
    uv = oracle_lib.project(model, lidar_intr, [], pc)
    assert np.array_equal(np.trunc(uv).astype(np.int64), np.stack([us, vs], axis=1))
    assert np.array_equal(inten_img[vs, us], np.clip(np.rint(bag.intensities[idx[vs, us]] * 255.0), 0, 255).astype(np.uint8)) and (inten_img[idx < 0] == 0).all()

    # what calibrate reads: the camera and the bag load through the same functions
    loaded_config, bags = dataset.load_dataset(dst)
    assert nid.create_camera(*dataset.camera_from_calib(loaded_config)) is not None and bags[0].num_points == m

    # the same map as a PCD file: byte-identical cloud
    dst2 = str(tmp_path / "data_pcd")
    assert preprocess_map.main(argv + ["--map_path", map_pcd, "--dst_path", dst2]) == 0
    with open(os.path.join(dst, "000000.ply"), "rb") as f, open(os.path.join(dst2, "000000.ply"), "rb") as g:
        assert f.read() == g.read()


def _cap(half_angle_deg, n, seed, radius=5.0):
    """n points on the spherical cap of the given half angle around +x (uniform in area), plus 2000 on its rim"""
    rng = np.random.default_rng(seed)
    a = math.radians(half_angle_deg)
    cos_t = np.concatenate([rng.uniform(math.cos(a), 1.0, n), np.full(2000, math.cos(a))])
    phi = rng.uniform(0, 2 * math.pi, n + 2000)
    sin_t = np.sqrt(1.0 - cos_t * cos_t)
    return radius * np.stack([cos_t, sin_t * np.cos(phi), sin_t * np.sin(phi)], axis=1)


@pytest.mark.gpu
def test_lidar_fov_of_a_cone_and_of_a_sphere():
    """A cap of half angle 40 degrees at 5 m: 80 degrees, within the angular size of a 0.2 m voxel at 5 m, atan(0.2 sqrt(3) / 5) --
    the furthest a voxel's representative can be from where the rim crosses the voxel (a derived bound, not a measured one)."""
    bound = math.atan(0.2 * math.sqrt(3.0) / 5.0)
    fov = preprocess.estimate_lidar_fov(_cap(40.0, 60000, 41), device=0)
    print(f"cap of 2 x 40 deg: {math.degrees(fov):.3f} deg (bound +-{math.degrees(bound):.3f})")
    assert abs(fov - math.radians(80.0)) <= bound
    assert preprocess.lidar_camera(fov)[0] == "plumb_bob"
    # float32 input takes the float32 route (a point that float32 rounding moves across a voxel face may change a representative)
    assert abs(preprocess.estimate_lidar_fov(_cap(40.0, 60000, 41).astype(np.float32), device=0) - math.radians(80.0)) <= bound
    shell = _cap(180.0, 60000, 42)
    fov = preprocess.estimate_lidar_fov(np.concatenate([shell, np.ones((len(shell), 1))], axis=1), device=0)
    print(f"full shell: {math.degrees(fov):.3f} deg")
    assert fov > math.radians(150.0) and preprocess.lidar_camera(fov)[0] == "equirectangular"
    with pytest.raises(ValueError):
        preprocess.estimate_lidar_fov(np.array([[2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 2.0]]), device=0)
    with pytest.raises(ValueError):  # coplanar
        preprocess.estimate_lidar_fov(np.array([[2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [2.0, 2.0, 0.0], [3.0, 1.0, 0.0], [1.0, 3.0, 0.0]]), device=0)
