"""The mask and range options of the command lines end to end on a small synthetic bag (64 x 48 pinhole, 4000 points):
``calibrate --mask``, ``viewer --mask`` and ``find_matches --mask``."""
import json
import math
import os
import shutil

import numpy as np
import pytest

import select_oracle as so
from direct_visual_lidar_calibration_amd import calibrate, dataset, find_matches, nid, se3, synth, viewer

pytestmark = pytest.mark.gpu

CAMERA = ("plumb_bob", [52.0, 51.0, 32.0, 24.0], [-0.04, 0.08, 1e-4, -3e-4, -0.04], 64, 48)
W, H = 64, 48
BAG = "bag0"

_cache = {}


def scene():
    if "s" not in _cache:
        _cache["s"] = synth.make_scene(CAMERA, num_points=4000, seed=13)
    return _cache["s"]


def write_dir(d, lidar_images=None, image=None):
    s = scene()
    dataset.write_preprocessed(d, CAMERA[:3], [(BAG, s.image_u8 if image is None else image, s.points, s.intensities)],
                               init_T_lidar_camera_tum=dataset.T_camera_lidar_to_tum(s.T_camera_lidar_init), lidar_images=lidar_images)


def bonnet_mask():
    """the lower part of the image and a strip on the left are ignored"""
    m = np.full((H, W), 255, dtype=np.uint8)
    m[36:, :] = 0
    m[:, :6] = 0
    return m


@pytest.mark.parametrize("reg", ["nid_bfgs", "nid_nelder_mead"])
def test_calibrate_with_an_all_valid_mask_and_no_margin_writes_the_same_transform_bit_for_bit(tmp_path, reg):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    write_dir(a)
    shutil.copytree(a, b)
    dataset.write_png_gray(os.path.join(b, "mask.png"), np.full((H, W), 255, dtype=np.uint8))
    calibrate.run(calibrate.build_parser().parse_args([a, "--registration_type", reg]), log=lambda *_: None)
    lines = []
    calibrate.run(calibrate.build_parser().parse_args([b, "--registration_type", reg, "--mask", os.path.join(b, "mask.png"), "--mask_margin", "0"]), log=lines.append)
    ra, rb = dataset.read_calib(a)["results"], dataset.read_calib(b)["results"]
    assert sorted(ra) == sorted(rb) == ["T_lidar_camera", "init_T_lidar_camera"]  # the keys of calib.json do not change
    assert ra["T_lidar_camera"] == rb["T_lidar_camera"] and ra["T_lidar_camera"] != ra["init_T_lidar_camera"]
    sel = [line for line in lines if line.startswith("select pair 0: the cull kept ")]
    assert sel and all("the mask removed 0, the range 0:" in line for line in sel)  # one line per outer iteration


def test_calibrate_with_a_mask_and_a_range_runs_and_logs_what_it_left_out(tmp_path):
    d = str(tmp_path / "d")
    write_dir(d)
    dataset.write_png_gray(os.path.join(d, BAG + "_mask.png"), bonnet_mask())
    lines = []
    _, _, x = calibrate.run(calibrate.build_parser().parse_args([d, "--mask", "auto", "--min_range", "2.5", "--max_range", "14"]), log=lines.append)
    sel = [line for line in lines if line.startswith("select pair 0")]
    removed = [(int(line.split("the mask removed ")[1].split(",")[0]), int(line.split("the range ")[1].split(":")[0])) for line in sel]
    assert sel and all(m > 0 and r > 0 for m, r in removed)
    dt, dr = se3.delta_trans_rot(x, scene().T_camera_lidar_true)
    dt0, dr0 = se3.delta_trans_rot(scene().T_camera_lidar_init, scene().T_camera_lidar_true)
    print(f"masked calibration: {dt:.4f} m / {math.degrees(dr):.3f} deg from the truth (initial guess: {dt0:.4f} m / {math.degrees(dr0):.3f} deg)")
    assert np.isfinite(x).all()


def test_viewer_halves_the_ignored_pixels_and_scores_the_selected_points(tmp_path):
    d = str(tmp_path / "d")
    write_dir(d)
    mask = bonnet_mask()
    mask_path = os.path.join(d, "mask.png")
    dataset.write_png_gray(mask_path, mask)
    argv = [d, "--transformation", "init_manual", "--mask", mask_path, "--mask_margin", "3", "--max_range", "14", "--view_size", "48x32", "--orbit_deg", "20", "--point_radius", "0"]
    assert viewer.main(argv) == 0
    with open(os.path.join(d, "viewer", "viewer.json")) as f:
        entry = json.load(f)["transformations"]["init_manual"]["bags"][BAG]

    s = scene()
    proj = nid.create_camera(*CAMERA[:3])
    T = np.linalg.inv(viewer.tum_to_pose(dataset.read_calib(d)["results"]["init_T_lidar_camera"]))
    eroded = so.erode(mask, 3)
    # the NID of viewer.json = a handle built by hand from the selection
    cloud = nid.Cloud(s.points, s.intensities)
    m = nid.Mask(mask, margin=3)
    assert np.array_equal(m.eroded(), eroded)
    min_z = math.cos(nid.estimate_camera_fov(proj, (W, H)))
    sub, idx = cloud.select(proj, (W, H), T, min_z, True, mask=m, max_range=14.0, return_indices=True)
    want = so.select(CAMERA[0], CAMERA[1], CAMERA[2], W, H, s.points, T, True, min_z, mask=mask, margin=3, max_range=14.0)
    assert np.array_equal(idx, want) and 0 < len(idx) < len(nid.ViewCulling(proj, (W, H)).cull(s.points, T))
    cost = nid.CostCalculatorNID.from_cloud(proj, s.image_u8, sub, nid.NIDCostParams(16), cull=None)
    assert entry["culled"] == len(idx) and entry["nid"] == cost.calculate(T)
    for x in (cost, sub, m, cloud):
        x.close()

    # the overlay: where no point is drawn, an ignored pixel of the ERODED mask shows half its grey value, every other pixel its own
    args = viewer.parse_args(argv)
    args.selection = {"masks": {BAG: mask}, "margin": 3, "min_range": 0.0, "max_range": 14.0}
    bag = dataset.load_dataset(d)[1][0]
    overlay, index, count, value = viewer.overlay_and_nid(args, proj, bag, T)
    assert count == len(idx) and value == entry["nid"]
    written, _ = dataset.read_png(os.path.join(d, "viewer", f"{BAG}_init_manual_overlay.png"))
    assert np.array_equal(written, overlay)
    free = index < 0
    ignored = eroded == 0
    expected = np.where(ignored, s.image_u8 >> 1, s.image_u8)
    assert (free & ignored).sum() > 200 and (free & ~ignored).sum() > 50 and (s.image_u8[free & ignored] > 1).any()
    assert np.array_equal(overlay[free], np.repeat(expected[free][:, None], 3, axis=1))
    assert ((mask != 0) & ignored).sum() > 0  # the margin grew the ignored region, and the overlay shows the grown one


def _blocks(seed):
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 40, dtype=np.uint8)
    for _ in range(25):
        y, x = rng.integers(12, H - 18), rng.integers(12, W - 18)
        img[y : y + rng.integers(3, 8), x : x + rng.integers(3, 8)] = rng.integers(90, 255)
    return img


@pytest.mark.parametrize("rotate", [0, 90])
def test_find_matches_reports_no_camera_keypoint_on_a_zero_pixel(tmp_path, rotate):
    d = str(tmp_path / "d")
    cam = _blocks(3)
    index = np.arange(H * W, dtype=np.int32).reshape(H, W) % 4000
    write_dir(d, lidar_images={BAG: (_blocks(4) / 255.0, index)}, image=cam)
    common = [d, "--rotate_camera", str(rotate), "--levels", "2"]
    find_matches.run(find_matches.build_parser().parse_args(common), log=lambda *_: None)
    with open(os.path.join(d, BAG + "_matches.json")) as f:
        free = json.load(f)
    k_free = np.array(free["kpts0"]).reshape(-1, 2)
    mask = np.full((H, W), 255, dtype=np.uint8)
    mask[:, :32] = 0
    assert (k_free[:, 0] < 32).sum() >= 2 and (k_free[:, 0] >= 32).sum() >= 2  # without the mask both halves hold keypoints
    dataset.write_png_gray(os.path.join(d, BAG + "_mask.png"), mask)
    find_matches.run(find_matches.build_parser().parse_args(common + ["--mask", "auto"]), log=lambda *_: None)
    with open(os.path.join(d, BAG + "_matches.json")) as f:
        got = json.load(f)
    k = np.array(got["kpts0"]).reshape(-1, 2)
    assert len(k) >= 2 and (mask[k[:, 1], k[:, 0]] != 0).all()
    assert got["kpts1"] == free["kpts1"] and sorted(got) == sorted(free)
