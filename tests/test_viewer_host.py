"""Host side of the headless viewer (direct_visual_lidar_calibration_amd/viewer.py, render.quantize_colors,
dataset.write_ply_colored): which transforms are found and in which order, TUM -> pose, the orbit pose, the coloured PLY, colour
quantisation, the command line.  No GPU: nothing here launches a kernel."""
import itertools
import json
import math
import os

import numpy as np
import pytest

from direct_visual_lidar_calibration_amd import dataset, render, viewer

KEYS = {"init_auto": "init_T_lidar_camera_auto", "init_manual": "init_T_lidar_camera", "result": "T_lidar_camera"}
ORDER = ["init_auto", "init_manual", "result"]  # viewer.cpp:49-74
TUM = {"init_auto": [0.1, -0.2, 0.3, 0.0, 0.0, 0.0, 1.0], "init_manual": [1.0, 2.0, 3.0, 1.0, 0.0, 0.0, 0.0], "result": [-1.0, 0.5, 0.25, 0.0, math.sqrt(0.5), 0.0, math.sqrt(0.5)]}


def config_with(labels):
    return {"camera": {}, "meta": {"bag_names": []}, "results": {KEYS[k]: TUM[k] for k in labels}}


@pytest.mark.parametrize("labels", [c for r in range(4) for c in itertools.combinations(ORDER, r)], ids=lambda c: "+".join(c) or "none")
def test_transforms_are_found_in_the_reference_order_and_selected_by_name(labels):
    """Every subset of the three keys, written into calib.json in REVERSE order: found in the reference's order whatever the file's;
    `last` = the last found (what the reference pre-selects), `all` = all of them, a present label = itself, an absent one refused."""
    cfg = config_with(labels[::-1])
    found = viewer.find_transforms(cfg)
    assert [f[0] for f in found] == [k for k in ORDER if k in labels]
    for label, T in found:
        assert np.array_equal(T, viewer.tum_to_pose(TUM[label]))
    if not labels:
        for which in ("last", "all", "result"):
            with pytest.raises(SystemExit, match="no transformation found"):
                viewer.select_transforms(found, which)
        return
    assert [f[0] for f in viewer.select_transforms(found, "last")] == [found[-1][0]]
    assert [f[0] for f in viewer.select_transforms(found, "all")] == [f[0] for f in found]
    for k in ORDER:
        if k in labels:
            assert [f[0] for f in viewer.select_transforms(found, k)] == [k]
        else:
            with pytest.raises(SystemExit, match=f"no '{k}' transformation"):
                viewer.select_transforms(found, k)


def test_tum_to_pose_against_closed_forms():
    """Identity; a half turn about x (q = (1, 0, 0, 0)): diag(1, -1, -1); a quarter turn about y: x -> -z, z -> x.  The translation is
    taken as given."""
    assert np.array_equal(viewer.tum_to_pose(TUM["init_auto"]), np.array([[1, 0, 0, 0.1], [0, 1, 0, -0.2], [0, 0, 1, 0.3], [0, 0, 0, 1.0]]))
    assert np.array_equal(viewer.tum_to_pose(TUM["init_manual"]), np.array([[1, 0, 0, 1.0], [0, -1, 0, 2.0], [0, 0, -1, 3.0], [0, 0, 0, 1.0]]))
    T = viewer.tum_to_pose(TUM["result"])
    assert np.allclose(T, np.array([[0, 0, 1, -1.0], [0, 1, 0, 0.5], [-1, 0, 0, 0.25], [0, 0, 0, 1.0]]), rtol=0, atol=4e-16)  # sqrt(0.5)^2 is 0.5 to an ulp
    assert np.array_equal(T[:3, 3], [-1.0, 0.5, 0.25])


def test_no_transform_prints_the_reference_line_and_writes_nothing(tmp_path, capsys):
    """calib.json without results (and with an empty `results`): status 1, the reference's line (viewer.cpp:78) on stderr, no output
    directory, nothing else touched -- before the dataset or the GPU is."""
    for results in (None, {}):
        d = tmp_path / ("none" if results is None else "empty")
        d.mkdir()
        cfg = {"camera": {"camera_model": "plumb_bob", "intrinsics": [1, 1, 1, 1], "distortion_coeffs": [0, 0, 0, 0, 0]}, "meta": {"bag_names": ["missing_bag"]}}
        if results is not None:
            cfg["results"] = results
        (d / "calib.json").write_text(json.dumps(cfg))
        assert viewer.main([str(d)]) == 1
        cap = capsys.readouterr()
        assert cap.err.strip() == "error: no transformation found in calib.json!!" and cap.out == ""
        assert sorted(os.listdir(d)) == ["calib.json"]


def test_orbit_pose_against_closed_forms():
    """Angle 0 is the camera pose bit for bit.  With the camera at the LiDAR origin and the pivot 2 m ahead, +90 deg puts the view's
    centre at (-2, 0, 2) looking along +x, -90 deg at (2, 0, 2) looking along -x: the pivot stays at (0, 0, 2) in every view and the y
    axis is untouched.  Under a general camera pose the same holds in the camera frame."""
    rng = np.random.default_rng(5)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    T = viewer.tum_to_pose([0.3, -0.1, 0.2, *q])
    assert np.array_equal(viewer.orbit_pose(T, 0.0, [1.0, 2.0, 3.0]), T)
    for angle, centre, forward in ((90.0, [-2.0, 0.0, 2.0], [1.0, 0.0, 0.0]), (-90.0, [2.0, 0.0, 2.0], [-1.0, 0.0, 0.0])):
        V = viewer.orbit_pose(np.eye(4), angle, [0.0, 0.0, 2.0])
        inv = np.linalg.inv(V)
        assert np.allclose(inv[:3, 3], centre, atol=1e-15)            # where the view camera sits
        assert np.allclose(inv[:3, 2], forward, atol=1e-15)            # where it looks
        assert np.allclose(inv[:3, 1], [0.0, 1.0, 0.0], atol=1e-15)    # the axis it turned about
        assert np.allclose(V @ [0.0, 0.0, 2.0, 1.0], [0.0, 0.0, 2.0, 1.0], atol=1e-15)  # the pivot: straight ahead, same distance
        # general camera pose: the view differs from the camera by the same motion, expressed in the camera frame
        pivot_lidar = np.linalg.inv(T) @ [0.0, 0.0, 2.0, 1.0]
        assert np.allclose(viewer.orbit_pose(T, angle, pivot_lidar[:3]), V @ T, atol=1e-14)
    V = viewer.orbit_pose(T, 37.0, [1.0, 2.0, 3.0])
    assert np.allclose(V[:3, :3] @ V[:3, :3].T, np.eye(3), atol=1e-15) and np.isclose(np.linalg.det(V[:3, :3]), 1.0)
    p = np.array([1.0, 2.0, 3.0, 1.0])
    assert np.allclose(V @ p, T @ p, atol=1e-14)


def test_view_camera_has_the_asked_horizontal_field_of_view():
    cam = viewer.view_camera((1280, 720), 60.0)
    assert cam.model == "plumb_bob" and not np.any(cam._dist8)
    fx, fy, cx, cy = cam._intr5[:4]
    assert fx == fy and (cx, cy) == (640.0, 360.0)
    assert np.isclose(2.0 * math.atan(640.0 / fx), math.radians(60.0), rtol=1e-15)


def test_colored_ply_is_read_back_byte_for_byte(tmp_path):
    """Header text, then 15 bytes a vertex: float32 x y z little endian, uchar red green blue.  read_ply gives the positions back."""
    rng = np.random.default_rng(2)
    for n in (0, 1, 257):
        pts = np.ones((n, 4))
        pts[:, :3] = rng.normal(size=(n, 3)) * 10.0
        rgb = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
        path = str(tmp_path / f"c{n}.ply")
        dataset.write_ply_colored(path, pts, rgb)
        data = open(path, "rb").read()
        header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {n}\nproperty float x\nproperty float y\nproperty float z\n"
                  "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n").encode()
        assert data[: len(header)] == header and len(data) == len(header) + 15 * n
        body = np.frombuffer(data, dtype=np.uint8, offset=len(header)).reshape(n, 15)
        assert body[:, :12].tobytes() == pts[:, :3].astype("<f4").tobytes()
        assert np.array_equal(body[:, 12:], rgb)
        back, inten = dataset.read_ply(path)
        assert inten is None and np.array_equal(back[:, :3], pts[:, :3].astype(np.float32).astype(np.float64))
    with pytest.raises(ValueError, match="one RGB colour per point"):
        dataset.write_ply_colored(str(tmp_path / "bad.ply"), np.ones((3, 4)), np.zeros((2, 3), dtype=np.uint8))


def test_quantize_colors():
    """floor(c * 255 + 0.5) clipped to 0..255: 0 -> 0, 1 -> 255, every k / 255 -> k, values outside [0, 1] saturate; at the half step
    0.5 / 255 the float32 input decides (the product is formed in float64, where it is exact)."""
    q = render.quantize_colors
    assert q(np.float32(0.0)) == 0 and q(np.float32(1.0)) == 255
    k = np.arange(256)
    assert np.array_equal(q((k / 255.0).astype(np.float32)), k)
    assert np.array_equal(q(np.array([-1.0, -1e-3, 1.001, 2.0, 1e30, -1e30], dtype=np.float32)), [0, 0, 255, 255, 255, 0])
    half = np.float32(0.5 / 255.0)
    below, above = np.nextafter(half, np.float32(0.0)), np.nextafter(half, np.float32(1.0))
    for v in (below, half, above):
        assert q(v) == (1 if float(v) * 255.0 >= 0.5 else 0)
    assert q(below) == 0 and q(above) == 1
    out = q(np.zeros((7, 4), dtype=np.float32))
    assert out.dtype == np.uint8 and out.shape == (7, 4)


def test_command_line_defaults_and_parsing():
    p = viewer.build_parser()
    a = p.parse_args(["some/dir"])
    assert (a.data_path, a.dst_path, a.transformation, a.blend_weight, a.point_radius, a.alpha) == ("some/dir", None, "last", 0.7, 1, 178)
    assert (a.orbit_deg, a.view_size, a.view_fov, a.first_n_bags, a.disable_culling, a.nid_bins, a.save_ply, a.device) == ([-30.0, -15.0, 15.0, 30.0], (1280, 720), 60.0, None, False, 16, False, 0)
    a = p.parse_args(["d", "--dst_path", "o", "--transformation", "init_auto", "--blend_weight", "0.25", "--point_radius", "2", "--alpha", "255", "--orbit_deg=-90,0,45.5",
                      "--view_size", "320x200", "--view_fov", "75", "--first_n_bags", "3", "--disable_culling", "--nid_bins", "64", "--save_ply", "--device", "1"])
    assert (a.dst_path, a.transformation, a.blend_weight, a.point_radius, a.alpha) == ("o", "init_auto", 0.25, 2, 255)
    assert (a.orbit_deg, a.view_size, a.view_fov, a.first_n_bags, a.disable_culling, a.nid_bins, a.save_ply, a.device) == ([-90.0, 0.0, 45.5], (320, 200), 75.0, 3, True, 64, True, 1)
    # the usage line's own spelling: a list that starts with a minus sign, as a separate argument (argparse alone refuses it)
    a = viewer.parse_args(["d", "--orbit_deg", "-30,-15,15,30", "--alpha", "10"])
    assert a.orbit_deg == [-30.0, -15.0, 15.0, 30.0] and a.alpha == 10 and a.data_path == "d"
    assert viewer.parse_args(["d", "--orbit_deg", "5"]).orbit_deg == [5.0] and viewer.parse_args(["--orbit_deg=-5,5", "d"]).orbit_deg == [-5.0, 5.0]
    for which in ("last", "all", "result", "init_manual", "init_auto"):
        assert p.parse_args(["d", "--transformation", which]).transformation == which
    with pytest.raises(SystemExit):
        p.parse_args(["d", "--transformation", "none"])
    with pytest.raises(SystemExit):
        p.parse_args([])
