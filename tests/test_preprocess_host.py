"""Host-side pieces of preprocess_map (no GPU): cv::equalizeHist in numpy, the PCD reader, the command line's parsing and the
choice of the virtual LiDAR camera."""
import math

import numpy as np
import pytest
import torch

from direct_visual_lidar_calibration_amd import dataset, preprocess, preprocess_map, synth


def _images():
    rng = np.random.default_rng(11)
    random = rng.integers(0, 256, (48, 64), dtype=np.uint8)
    three = rng.choice(np.array([17, 90, 201], dtype=np.uint8), size=(48, 64))
    constant = np.full((48, 64), 93, dtype=np.uint8)
    from_zero = rng.integers(0, 40, (48, 64), dtype=np.uint8)
    from_zero[0, 0] = 0
    return {"random": random, "three_levels": three, "constant": constant, "first_bin_zero": from_zero}


@pytest.mark.parametrize("name", ["random", "three_levels", "constant", "first_bin_zero"])
def test_equalize_hist_equals_the_torch_restatement_byte_for_byte(name):
    img = _images()[name]
    want = synth.equalize_hist_u8(torch.from_numpy(img)).numpy()
    got = preprocess.equalize_hist(img)
    assert got.dtype == np.uint8 and got.shape == img.shape and np.array_equal(got, want)
    if name == "constant":
        assert np.array_equal(got, img)
    else:
        assert got.min() == 0 and got.max() == 255


def _write_pcd(path, fields, sizes, types, counts, n, data, body):
    header = (f"# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS {' '.join(fields)}\nSIZE {' '.join(map(str, sizes))}\nTYPE {' '.join(types)}\n"
              f"COUNT {' '.join(map(str, counts))}\nWIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA {data}\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(body)


def _cloud(n=37):
    rng = np.random.default_rng(12)
    return rng.uniform(-20, 20, (n, 3)).astype(np.float32), rng.uniform(0, 255, n).astype(np.float32)


def test_read_pcd_binary_round_trip(tmp_path):
    xyz, inten = _cloud()
    rec = np.zeros(len(xyz), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")])
    rec["x"], rec["y"], rec["z"], rec["intensity"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], inten
    path = str(tmp_path / "a.pcd")
    _write_pcd(path, ["x", "y", "z", "intensity"], [4] * 4, ["F"] * 4, [1] * 4, len(xyz), "binary", rec.tobytes())
    got_xyz, got_inten = dataset.read_pcd(path)
    assert got_xyz.dtype == np.float32 and got_inten.dtype == np.float32 and got_xyz.shape == (37, 3) and got_inten.shape == (37,)
    assert np.array_equal(got_xyz, xyz) and np.array_equal(got_inten, inten)


def test_read_pcd_skips_an_rgb_field_and_wider_fields(tmp_path):
    """x y z, a packed rgb (U 4), a 3-count normal (F 4 x 3) and a double timestamp between z and intensity"""
    xyz, inten = _cloud()
    dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgb", "<u4"), ("normal", "<f4", (3,)), ("t", "<f8"), ("intensity", "<f4")])
    rec = np.zeros(len(xyz), dtype=dt)
    rec["x"], rec["y"], rec["z"], rec["intensity"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], inten
    rec["rgb"], rec["t"], rec["normal"] = 0xFFAA3311, 1.7e9, 0.5
    path = str(tmp_path / "b.pcd")
    _write_pcd(path, ["x", "y", "z", "rgb", "normal", "t", "intensity"], [4, 4, 4, 4, 4, 8, 4], ["F", "F", "F", "U", "F", "F", "F"], [1, 1, 1, 1, 3, 1, 1], len(xyz), "binary", rec.tobytes())
    got_xyz, got_inten = dataset.read_pcd(path)
    assert np.array_equal(got_xyz, xyz) and np.array_equal(got_inten, inten)
    # the same as text
    lines = "".join(f"{float(r['x'])!r} {float(r['y'])!r} {float(r['z'])!r} {int(r['rgb'])} 0.5 0.5 0.5 1700000000.0 {float(r['intensity'])!r}\n" for r in rec)
    path = str(tmp_path / "c.pcd")
    _write_pcd(path, ["x", "y", "z", "rgb", "normal", "t", "intensity"], [4, 4, 4, 4, 4, 8, 4], ["F", "F", "F", "U", "F", "F", "F"], [1, 1, 1, 1, 3, 1, 1], len(xyz), "ascii", lines.encode("ascii"))
    got_xyz, got_inten = dataset.read_pcd(path)
    assert np.array_equal(got_xyz, xyz) and np.array_equal(got_inten, inten)


def test_read_pcd_ascii_without_intensity_and_refusals(tmp_path):
    xyz, _ = _cloud(5)
    path = str(tmp_path / "d.pcd")
    _write_pcd(path, ["x", "y", "z"], [4] * 3, ["F"] * 3, [1] * 3, 5, "ascii", "".join(f"{float(a)!r} {float(b)!r} {float(c)!r}\n" for a, b, c in xyz).encode("ascii"))
    got_xyz, got_inten = dataset.read_pcd(path)
    assert np.array_equal(got_xyz, xyz) and np.array_equal(got_inten, np.zeros(5, dtype=np.float32))
    path = str(tmp_path / "e.pcd")
    _write_pcd(path, ["x", "y", "z"], [4] * 3, ["F"] * 3, [1] * 3, 5, "binary_compressed", b"\0" * 16)
    with pytest.raises(ValueError, match="binary_compressed"):
        dataset.read_pcd(path)
    path = str(tmp_path / "f.pcd")
    _write_pcd(path, ["x", "y", "z"], [8] * 3, ["F"] * 3, [1] * 3, 5, "binary", b"\0" * 120)
    with pytest.raises(ValueError, match="F 8"):
        dataset.read_pcd(path)
    path = str(tmp_path / "g.pcd")
    _write_pcd(path, ["x", "y", "z"], [4] * 3, ["F"] * 3, [1] * 3, 5, "binary", b"\0" * 59)
    with pytest.raises(ValueError, match="truncated"):
        dataset.read_pcd(path)


def test_command_line_parsing(capsys):
    assert preprocess_map.parse_values("1100,1100,960,540") == [1100.0, 1100.0, 960.0, 540.0]
    assert all(isinstance(v, float) for v in preprocess_map.parse_values("1100,1100,960,540"))
    assert preprocess_map.parse_values("-0.04,0.08,1e-4,-3e-4,-0.04") == [-0.04, 0.08, 1e-4, -3e-4, -0.04]
    assert preprocess_map.parse_values("") == []
    args = preprocess_map.build_parser().parse_args(preprocess_map._attach_values(["--map_path", "m.ply", "--camera_distortion_coeffs", "-0.04,0.08", "--camera_intrinsics", "1,2,3,4"]))
    assert args.camera_distortion_coeffs == "-0.04,0.08" and args.camera_intrinsics == "1,2,3,4"
    assert args.voxel_resolution == 0.002 and args.min_distance == 1.0 and args.device == 0
    # a missing required flag: the usage, and 0 (preprocess_map.cpp:56-61)
    assert preprocess_map.main(["--map_path", "m.ply", "--image_path", "i.png", "--dst_path", "d", "--camera_model", "plumb_bob", "--camera_intrinsics", "1,2,3,4"]) == 0
    out = capsys.readouterr().out
    assert "usage: preprocess_map" in out and "--camera_distortion_coeffs" in out and "NOT applied" in out


def test_jpeg_input_is_refused_with_a_message(tmp_path, capsys):
    path = str(tmp_path / "photo.jpg")
    with open(path, "wb") as f:
        f.write(b"\xff\xd8\xff\xe0" + b"\0" * 32)
    rc = preprocess_map.main(["--map_path", "m.ply", "--image_path", path, "--dst_path", str(tmp_path / "d"), "--camera_model", "plumb_bob", "--camera_intrinsics", "1,2,3,4",
                              "--camera_distortion_coeffs", ""])
    assert rc == 1 and "JPEG" in capsys.readouterr().err


@pytest.mark.parametrize("fov_deg", [149.0, 151.0])
def test_lidar_camera_choice(fov_deg):
    """preprocess_map.cpp:184-200 against the closed forms tests/test_pose_gpu.py::lidar_image_camera uses (restated here)"""
    model, intrinsics, size, T_lidar_camera = preprocess.lidar_camera(math.radians(fov_deg))
    want = np.eye(4)
    if fov_deg < 150.0:
        fx = 1024.0 / (2.0 * np.tan(np.radians(fov_deg) / 2.0))
        ry = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])  # AngleAxis(pi/2, Y)
        rz = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])  # AngleAxis(-pi/2, Z)
        want[:3, :3] = ry @ rz
        assert model == "plumb_bob" and size == (1024, 1024)
        assert intrinsics[2:] == [512.0, 512.0] and intrinsics[0] == intrinsics[1] and abs(intrinsics[0] - fx) <= 1e-12 * fx
        assert np.allclose(want[:3, :3] @ np.array([0.0, 0.0, 1.0]), [1.0, 0.0, 0.0])  # the optical axis is the LiDAR's x
    else:
        want[:3, :3] = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])  # AngleAxis(-pi/2, X)
        assert model == "equirectangular" and size == (1920, 960) and intrinsics == [1920.0, 960.0]
        c, s = math.cos(-math.pi / 2), math.sin(-math.pi / 2)
        assert np.allclose(want[:3, :3], [[1, 0, 0], [0, c, -s], [0, s, c]], atol=1e-15)
    assert np.array_equal(T_lidar_camera, want)
    assert abs(np.linalg.det(T_lidar_camera[:3, :3]) - 1.0) < 1e-15
