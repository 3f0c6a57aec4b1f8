"""Host-side tests of masks and range gates (no GPU): the numpy restatement of the selection (tests/select_oracle.py) against the
cull oracle and against erosions worked out by hand, the conditions the GPU tests' inputs have to satisfy, ``dataset.load_mask``,
the command lines' new options, and ``matching.find_matches`` with a camera mask on the matching oracle."""
import math
import os

import numpy as np
import pytest

import matching_oracle as mo
import oracle_lib
import select_cases as sc
import select_oracle as so
from direct_visual_lidar_calibration_amd import calibrate, dataset, find_matches, matching, synth, viewer
from test_image_edges import MODELS


@pytest.mark.parametrize("model", MODELS)
def test_with_an_all_valid_mask_and_the_default_range_the_oracle_is_the_cull_oracle(model):
    c = sc.pixel_cloud(model)
    cam = c["cam"]
    for depth in (True, False):
        ref = oracle_lib.view_culling(cam.model, cam.intr, cam.dist, sc.W, sc.H, c["pts"], c["T"], depth, min_z=c["min_z"])
        for mask in (None, sc.masks()["valid"]):
            idx, parts = so.select(cam.model, cam.intr, cam.dist, sc.W, sc.H, c["pts"], c["T"], depth, c["min_z"], mask=mask, margin=5, return_parts=True)
            assert idx.dtype == np.int32 and np.array_equal(idx, ref)
            assert parts == dict(kept=len(ref), mask_removed=0, range_removed=0, fractions=parts["fractions"])
        # the inputs do what they are for: some points are culled, some kept, and with the depth buffer fewer are kept
        assert 1000 < len(ref) < len(c["pts"]) or (model == "equirectangular" and not depth and len(ref) == len(c["pts"]))  # (that image holds every direction)
    assert len(oracle_lib.view_culling(cam.model, cam.intr, cam.dist, sc.W, sc.H, c["pts"], c["T"], True, min_z=c["min_z"])) < len(ref)


@pytest.mark.parametrize("model", MODELS)
def test_every_survivor_of_the_built_cloud_sits_well_inside_its_pixel(model):
    """the condition on the input of test_select_gpu's mask test: every fraction the oracle truncates away lies in [0.2, 0.8]"""
    c = sc.pixel_cloud(model)
    cam = c["cam"]
    _, parts = so.select(cam.model, cam.intr, cam.dist, sc.W, sc.H, c["pts"], c["T"], False, c["min_z"], return_parts=True)
    f = parts["fractions"]
    assert f.shape[0] > 2000 and f.min() >= 0.2 and f.max() <= 0.8


@pytest.mark.parametrize("R", [0, 1, 2, 64])
@pytest.mark.parametrize("where", [(0, 0), (0, 47), (63, 47), (63, 0), (17, 0), (0, 23), (63, 30), (40, 47), (31, 20)])
def test_erosion_of_a_single_zero_pixel_is_its_clipped_box(R, where):
    x0, y0 = where
    mask = np.full((sc.H, sc.W), 200, dtype=np.uint8)
    mask[y0, x0] = 0
    want = np.full((sc.H, sc.W), 200, dtype=np.uint8)
    want[max(y0 - R, 0) : y0 + R + 1, max(x0 - R, 0) : x0 + R + 1] = 0
    got = so.erode(mask, R)
    assert np.array_equal(got, want)
    assert (got == 0).sum() == (min(x0 + R, sc.W - 1) - max(x0 - R, 0) + 1) * (min(y0 + R, sc.H - 1) - max(y0 - R, 0) + 1)


def test_erosion_takes_the_minimum_of_the_bytes_and_an_all_valid_mask_stays():
    m = sc.masks()
    assert np.array_equal(so.erode(m["valid"], 5), m["valid"]) and not so.erode(m["zero"], 0).any()
    assert np.array_equal(so.erode(m["random"], 0), m["random"])
    two = np.full((5, 7), 9, dtype=np.uint8)
    two[2, 3] = 4
    assert so.erode(two, 1)[1:4, 2:5].tolist() == [[4] * 3] * 3 and so.erode(two, 1)[0, 0] == 9


def test_the_range_rule_on_the_host():
    p = np.array([[3.0, 0.0, 4.0, 1.0], [1.0, 2.0, 2.0, 1.0], [0.0, 0.0, 0.0, 1.0]])
    assert so.range_ok(p).tolist() == [True, True, True]
    assert so.range_ok(p, 3.0, 5.0).tolist() == [True, True, False]
    assert so.range_ok(p, 5.0, 5.0).tolist() == [True, False, False]
    assert so.range_ok(p, 0.0, np.nextafter(3.0, 0.0)).tolist() == [False, False, True]


# ---- dataset.load_mask
def _png(path, value, shape=(12, 16)):
    dataset.write_png_gray(str(path), np.full(shape, value, dtype=np.uint8))


def test_load_mask_precedence_and_refusals(tmp_path):
    d = str(tmp_path)
    lines = []
    assert dataset.load_mask(d, "bag0", None, (12, 16)) is None
    assert dataset.load_mask(d, "bag0", "auto", (12, 16), log=lines.append) is None  # neither file: the bag is used whole, and that is logged
    assert len(lines) == 1 and "bag0" in lines[0] and "whole" in lines[0]
    _png(tmp_path / "mask.png", 7)
    assert (dataset.load_mask(d, "bag0", "auto", (12, 16)) == 7).all()
    _png(tmp_path / "bag0_mask.png", 9)
    assert (dataset.load_mask(d, "bag0", "auto", (12, 16)) == 9).all()  # the bag's own file first
    assert (dataset.load_mask(d, "bag1", "auto", (12, 16)) == 7).all()  # ... and only for that bag
    _png(tmp_path / "other.png", 3)
    m = dataset.load_mask(d, "bag0", str(tmp_path / "other.png"), (12, 16))
    assert m.dtype == np.uint8 and m.shape == (12, 16) and (m == 3).all()  # a path: that file for every bag
    with pytest.raises(ValueError, match=r"other\.png: the mask is 16x12, the image of bag0 16x13"):
        dataset.load_mask(d, "bag0", str(tmp_path / "other.png"), (13, 16))
    with pytest.raises(ValueError, match=r"bag0_mask\.png"):
        dataset.load_mask(d, "bag0", "auto", (16, 12))
    with pytest.raises(FileNotFoundError, match=r"nowhere\.png"):
        dataset.load_mask(d, "bag0", str(tmp_path / "nowhere.png"), (12, 16))


# ---- the command lines
@pytest.mark.parametrize("module", [calibrate, viewer])
def test_selection_options_defaults_and_refusals(module):
    parse = module.build_parser().parse_args
    assert dataset.selection_options(parse(["d"])) is None  # none given: the caller keeps the path without them
    assert dataset.selection_options(parse(["d", "--mask", "auto"])) == {"mask": "auto", "margin": 2, "min_range": 0.0, "max_range": math.inf}
    assert dataset.selection_options(parse(["d", "--min_range", "1.5"])) == {"mask": None, "margin": 2, "min_range": 1.5, "max_range": math.inf}
    assert dataset.selection_options(parse(["d", "--max_range", "40", "--mask_margin", "0", "--mask", "m.png"])) == {"mask": "m.png", "margin": 0, "min_range": 0.0, "max_range": 40.0}
    assert dataset.selection_options(parse(["d", "--mask_margin", "64"]))["margin"] == 64
    for bad in (["--mask_margin", "-1"], ["--mask_margin", "65"], ["--min_range", "-0.5"], ["--min_range", "3", "--max_range", "2"], ["--min_range", "nan"], ["--max_range", "nan"]):
        with pytest.raises(SystemExit, match="error: "):
            dataset.selection_options(parse(["d"] + bad))
    with pytest.raises(SystemExit):
        parse(["d", "--mask_margin", "two"])


def test_find_matches_takes_a_mask_and_nothing_else_of_the_four():
    p = find_matches.build_parser()
    assert p.parse_args(["d"]).mask is None and p.parse_args(["d", "--mask", "auto"]).mask == "auto"
    with pytest.raises(SystemExit):
        p.parse_args(["d", "--mask_margin", "2"])


def test_calibrate_refuses_a_mask_of_the_wrong_size_before_any_device(tmp_path):
    d = str(tmp_path / "data")
    s = synth.make_scene(("plumb_bob", [50.0, 50.0, 32.0, 24.0], [0.0] * 5, 64, 48), num_points=500, seed=3)
    dataset.write_preprocessed(d, (s.model, s.intrinsics, s.distortion), [("bag0", s.image_u8, s.points, s.intensities)], init_T_lidar_camera_tum=dataset.T_camera_lidar_to_tum(s.T_camera_lidar_init))
    _png(os.path.join(d, "mask.png"), 255, shape=(48, 63))
    with pytest.raises(ValueError, match=r"mask\.png: the mask is 63x48, the image of bag0 64x48"):
        calibrate.run(calibrate.build_parser().parse_args([d, "--mask", "auto", "--dry_run"]), log=lambda *_: None)
    _png(os.path.join(d, "mask.png"), 255, shape=(48, 64))
    lines = []
    calibrate.run(calibrate.build_parser().parse_args([d, "--mask", "auto", "--min_range", "1", "--dry_run"]), log=lines.append)
    assert any(line.startswith("selection: mask auto, margin 2 px, range [1.0, inf] m") for line in lines)
    with pytest.raises(SystemExit, match="--mask_margin"):
        calibrate.run(calibrate.build_parser().parse_args([d, "--mask_margin", "70", "--dry_run"]), log=lambda *_: None)


# ---- matching.find_matches with a camera mask, on the matching oracle
def _blocks(seed, shape=(80, 96)):
    rng = np.random.default_rng(seed)
    img = np.full(shape, 40, dtype=np.uint8)
    for _ in range(40):
        y, x = rng.integers(0, shape[0] - 8), rng.integers(0, shape[1] - 8)
        img[y : y + rng.integers(4, 12), x : x + rng.integers(4, 12)] = rng.integers(90, 255)
    return img


@pytest.mark.parametrize("rotate", [0, 90])
def test_find_matches_on_the_oracle_reports_no_camera_keypoint_on_a_zero_pixel(rotate):
    cam, lid = _blocks(1), _blocks(2)
    run = lambda **kw: matching.find_matches(cam, lid, None, levels=2, rotate_camera=rotate, detect=mo.detect, match=mo.match, **kw)  # noqa: E731
    free = run()
    k_free = np.array(free["kpts0"]).reshape(-1, 2)
    mask = np.full(cam.shape, 255, dtype=np.uint8)
    mask[:, :48] = 0  # the left half of the UNROTATED image
    assert (k_free[:, 0] < 48).sum() >= 3 and (k_free[:, 0] >= 48).sum() >= 3  # without the mask both halves hold keypoints
    got = run(camera_valid_mask=mask)
    k = np.array(got["kpts0"]).reshape(-1, 2)
    assert len(k) >= 3 and (mask[k[:, 1], k[:, 0]] != 0).all()
    assert got["kpts1"] == free["kpts1"]  # the LiDAR side is untouched
    # an all-valid mask changes one thing only: nothing is filled on the camera side, and with no hole there is nothing to fill
    assert run(camera_valid_mask=np.ones(cam.shape, dtype=bool)) == free
    with pytest.raises(ValueError, match="camera_valid_mask"):
        run(camera_valid_mask=mask[:, :-1])
