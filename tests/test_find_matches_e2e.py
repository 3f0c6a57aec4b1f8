"""find_matches end to end on the GPU: preprocessed directory -> ``find_matches`` -> ``initial_guess_auto`` -> ``calibrate``, with no
file from outside this package (tests/find_matches_scene.py builds the scene: pinhole_vga camera, 1M points, a 512 x 512 LiDAR image).

A CORRECT match is one whose camera keypoint lies within 10 px (initial_guess_auto's --ransac_error_thresh default) of its 3D point
projected under the true pose.  The yardstick of the pose error is what initial_guess_auto reaches on the same directory from
GROUND-TRUTH matches of the same LiDAR keypoints (projected under the true pose, rounded to integer pixels): existing code only.

Measured on an MI355X and recorded in profiles/find_matches.json (the matches are bit-identical to the CPU oracle's, the RANSAC is
seeded): 2048 + 2048 keypoints, 300 accepted matches, 250 correct; every one of the RANSAC winner's 250 inliers correct (worst 7.9 px);
matcher's guess 2.33e-2 m / 1.90e-3 rad from the truth, yardstick 7.19e-4 m / 4.14e-5 rad: factors 32 and 46.
POSE_FACTOR = 100 is the bar: the yardstick's keypoints carry rounding noise (0.29 px rms per axis) over 2048 matches, the matcher's a
localisation noise s over 250; a least-squares pose error scales with noise / sqrt(count), so the factor is (s / 0.29) sqrt(2048 / 250) =
9.9 s -- 100 at s = 10 px, the largest noise a correct match can have by definition.  (s = 3 to 4.6 px explains what was measured.)
``calibrate`` chain: from the ground-truth-match guess and from the scene's own initial guess it ends 5.41e-4 m / 5.20e-5 rad apart,
so the bar is max(1e-3, 2 x that) = 1.08e-3 m / 1e-3 rad; from the matcher's guess it ended 5.38e-4 m / 4.63e-5 rad from the former."""
import json
import os

import numpy as np
import pytest

import find_matches_scene as fms
import matching_oracle as mo
from direct_visual_lidar_calibration_amd import find_matches, matching, se3

pytestmark = pytest.mark.gpu

POSE_FACTOR = 100.0  # the matcher's initial-guess error over the ground-truth-match yardstick's (module docstring)
DELTA_T_BAR = 1e-3   # the project's bar on a calibration result [m] and [rad]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """The pipeline, once: directory, find_matches CLI, initial_guess_auto from its file and from ground-truth matches, calibrate from
    three starts."""
    s = fms.scene()
    inten, idx = fms.render_lidar(s, device=0)
    d = str(tmp_path_factory.mktemp("find_matches") / "data")
    fms.write_directory(d, s, inten, idx)
    lines = []
    written = find_matches.run(find_matches.build_parser().parse_args([d]), log=lines.append)
    result = fms.read_matches(d)
    guess = fms.initial_guess(d, s)
    fms.write_matches(d, fms.ground_truth_matches(s, idx, np.array(result["kpts1"]).reshape(-1, 2)))
    yard = fms.initial_guess(d, s)
    x_gt = fms.run_calibrate(d)  # from results.init_T_lidar_camera_auto = the ground-truth-match guess
    fms.set_manual_guess(d, s.T_camera_lidar_init)
    x_init = fms.run_calibrate(d)
    fms.set_manual_guess(d, guess["x"])
    x_matcher = fms.run_calibrate(d)
    return dict(s=s, inten=inten, idx=idx, d=d, lines=lines, written=written, result=result, guess=guess, yard=yard, x_gt=x_gt, x_init=x_init, x_matcher=x_matcher)


def test_cli_writes_the_file_the_cpu_oracle_computes(run):
    s, result = run["s"], run["result"]
    assert run["written"] == [os.path.join(run["d"], "bag0_matches.json")] and "2048 camera keypoints" in run["lines"][0]
    assert sorted(result) == ["confidence", "kpts0", "kpts1", "matches"]
    n0, n1 = len(result["kpts0"]) // 2, len(result["kpts1"]) // 2
    assert len(result["matches"]) == len(result["confidence"]) == n0 and max(result["matches"]) < n1
    assert all(isinstance(v, int) for v in result["kpts0"] + result["kpts1"] + result["matches"])
    lid = fms.intensities_u8(run["inten"])
    assert result == matching.find_matches(s.image_u8, lid, run["idx"] >= 0, detect=mo.detect, match=mo.match)
    k1 = np.array(result["kpts1"]).reshape(-1, 2)
    assert (run["idx"][k1[:, 1], k1[:, 0]] >= 0).all()  # no LiDAR keypoint on a blank pixel
    for m, c in zip(result["matches"], result["confidence"]):
        assert (c == 0.0) if m < 0 else (0.75 <= c <= 1.0)  # 1 - d / 256 with d <= 64


def test_correct_matches_exist_and_the_ransac_winner_holds_nothing_else(run):
    g = run["guess"]
    correct = g["err"] < fms.RANSAC_THRESH
    print(f"{len(g['err'])} correspondences, {int(correct.sum())} correct, {int(g['inliers'].sum())} RANSAC inliers, worst inlier {g['err'][g['inliers']].max():.2f} px")
    assert correct.sum() >= 2, "void: fewer than two correct matches"
    assert g["inliers"].sum() >= 2 and correct[g["inliers"]].all(), np.flatnonzero(g["inliers"] & ~correct)


def test_initial_guess_stays_within_the_factor_of_the_ground_truth_match_yardstick(run):
    g, y = run["guess"], run["yard"]
    print(f"matcher: {g['dt']:.3e} m, {g['dr']:.3e} rad; ground-truth matches: {y['dt']:.3e} m, {y['dr']:.3e} rad; factors {g['dt'] / y['dt']:.1f}, {g['dr'] / y['dr']:.1f}")
    assert len(y["err"]) >= 1000 and y["inliers"].all() and y["err"].max() < 1.0  # the yardstick is what it claims: rounding only
    assert g["dt"] <= POSE_FACTOR * y["dt"] and g["dr"] <= POSE_FACTOR * y["dr"], (g["dt"], y["dt"], g["dr"], y["dr"])
    with open(os.path.join(ROOT, "profiles", "find_matches.json")) as f:
        assert json.load(f)["bars"]["pose_factor_over_yardstick"] == POSE_FACTOR  # the recorded bar is the one asserted here


def test_calibrate_from_the_matchers_guess_ends_where_it_ends_from_ground_truth(run):
    dt0, dr0 = se3.delta_trans_rot(run["x_gt"], run["x_init"])  # two runs of existing code
    bar_t, bar_r = max(DELTA_T_BAR, 2.0 * dt0), max(DELTA_T_BAR, 2.0 * dr0)
    dt, dr = se3.delta_trans_rot(run["x_gt"], run["x_matcher"])
    print(f"existing code: {dt0:.3e} m, {dr0:.3e} rad apart -> bars {bar_t:.3e} m, {bar_r:.3e} rad; matcher's start: {dt:.3e} m, {dr:.3e} rad")
    assert dt <= bar_t and dr <= bar_r, (dt, bar_t, dr, bar_r)


def test_rotate_lidar_undoes_a_lidar_image_stored_on_its_side(run, tmp_path):
    """The same scene with both LiDAR images stored turned 270 degrees clockwise; ``--rotate_lidar 90`` turns them upright for the
    matcher and maps the keypoints back into the STORED image.  Same keypoints, same matches, hence the same 3D points and pose."""
    s = run["s"]
    d = str(tmp_path / "data")
    _, idx_stored = fms.write_directory(d, s, run["inten"], run["idx"], stored_rotation=270)
    assert find_matches.main([d, "--rotate_lidar", "90"]) == 0
    turned, upright = fms.read_matches(d), run["result"]
    assert turned["kpts0"] == upright["kpts0"] and turned["matches"] == upright["matches"] and turned["confidence"] == upright["confidence"]
    k_t, k_u = np.array(turned["kpts1"]).reshape(-1, 2), np.array(upright["kpts1"]).reshape(-1, 2)
    assert np.array_equal(idx_stored[k_t[:, 1], k_t[:, 0]], run["idx"][k_u[:, 1], k_u[:, 0]])  # the same points of the cloud
    assert np.array_equal(k_t, np.stack([k_u[:, 1], fms.LIDAR_SIZE - 1 - k_u[:, 0]], axis=1))  # 270 clockwise: (x, y) -> (y, W - 1 - x)
    g = fms.initial_guess(d, s)
    assert (g["err"] < fms.RANSAC_THRESH)[g["inliers"]].all() and g["inliers"].sum() >= 2
    assert np.array_equal(g["T"], run["guess"]["T"])
    # left unrotated, the turned image does not match: upright BRIEF has no orientation
    assert find_matches.main([d]) == 0
    wrong = fms.read_matches(d)
    assert sum(1 for m in wrong["matches"] if m >= 0) < sum(1 for m in upright["matches"] if m >= 0) // 4
