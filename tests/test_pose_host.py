"""CPU tests of the initial guess (pose.py, initial_guess_auto.py, the host entry points of csrc/nidreg_pose.hip): bearings,
the hypothesis sampler, the reprojection least squares, the file logic and the command line.  No GPU: the RANSAC stage of the
command-line test is a numpy stand-in (tests/pose_oracle.py)."""
import json
import os

import numpy as np
import pytest

import oracle_lib
import pose_oracle
from direct_visual_lidar_calibration_amd import calibrate, dataset, initial_guess_auto, nid, pose, se3, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pixel_grid(W, H):
    us = np.unique(np.linspace(0, W - 1, 16).astype(int))
    vs = np.unique(np.linspace(0, H - 1, 13).astype(int))
    return np.array([(float(u), float(v)) for v in vs for u in us])


def test_bearings_equal_the_oracles_nelder_mead_on_all_six_models():
    """nidreg_estimate_directions against oracle_lib.nelder_mead over oracle_lib.project with the reference's to_dir, 16 x 13 =
    208 integer pixels spread over the image of each of the six camera models, 1e-9 per component.  A pixel may be excluded
    when the two Nelder-Mead runs take different branches (a comparison decided inside the ~1e-14 difference of the two
    projection codes' reciprocal seeds; it shows as a disagreement of 1e-6 or more), at most 2 % of a model's pixels.
    Excluded on this grid: 0 of 208 for every model."""
    from test_gpu_parity import CAMERAS

    for name, (model, intr, dist, W, H) in CAMERAS.items():
        proj = nid.create_camera(model, intr, dist)
        uv = _pixel_grid(W, H)
        got = pose.estimate_directions(proj, uv)
        ref = np.array([pose_oracle.estimate_direction(model, intr, dist, p) for p in uv])
        diff = np.abs(got - ref).max(axis=1)
        branch = diff > 1e-6
        print(f"{name}: {len(uv)} pixels, max |d| {diff[~branch].max():.3e}, excluded {int(branch.sum())}")
        assert branch.sum() <= 0.02 * len(uv), (name, int(branch.sum()))
        assert diff[~branch].max() <= 1e-9, (name, float(diff[~branch].max()))
        # a bearing found is a bearing that projects onto its pixel (Nelder-Mead stops at a simplex variance of 1e-5 rad^2)
        assert np.isfinite(got).all() and np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-12)
    # one pixel more or fewer than a multiple of the thread slices, and the empty call
    proj = nid.create_camera(*CAMERAS["plumb_bob"][:3])
    uv = _pixel_grid(320, 240)[:37]
    assert np.array_equal(pose.estimate_directions(proj, uv), np.concatenate([pose.estimate_directions(proj, uv[:5]), pose.estimate_directions(proj, uv[5:])]))
    assert pose.estimate_directions(proj, np.zeros((0, 2))).shape == (0, 3)


def test_sampler_gives_distinct_in_range_pairs_and_is_a_pure_function():
    for n in (2, 3, 1000):
        pairs = pose.sample_pairs(5, n, 20000)
        assert pairs.shape == (20000, 2) and pairs.min() >= 0 and pairs.max() < n
        assert (pairs[:, 0] != pairs[:, 1]).all()
        assert set(np.unique(pairs[:, 0])) == set(range(n)) and set(np.unique(pairs[:, 1])) == set(range(n))
        # pure in (seed, k, n): a prefix, a second call
        assert np.array_equal(pose.sample_pairs(5, n, 100), pairs[:100])
        assert np.array_equal(pose.sample_pairs(5, n, 20000), pairs)
    assert not np.array_equal(pose.sample_pairs(5, 1000, 256), pose.sample_pairs(6, 1000, 256))
    assert not np.array_equal(pose.sample_pairs(5, 1000, 256), pose.sample_pairs(5, 1001, 256))
    with pytest.raises(RuntimeError, match="nidreg_ransac_sample_pairs"):
        pose.sample_pairs(0, 1, 4)


def _perturbed_start(T_true, angle_deg, seed):
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    T = np.eye(4)
    T[:3, :3] = T_true[:3, :3] @ se3.quat_to_rot(se3.so3_exp_quat(axis * np.radians(angle_deg)))
    return T  # t = 0, as PoseEstimation::estimate starts the least squares


@pytest.mark.parametrize("camera", ["pinhole_vga", "fisheye_1080p"])
def test_lsq_recovers_the_pose_from_exact_correspondences(camera):
    """500 exact (real-valued) projections, start = the true rotation turned by 2 degrees with t = 0: a zero-residual problem,
    Levenberg-Marquardt converges quadratically -- 1e-6 m / 1e-6 rad, the project's figure for pose agreement."""
    scene, kpts, pts, _ = pose_oracle.make_correspondences(camera, 500, 0.0, seed=3)
    proj = nid.create_camera(scene.model, scene.intrinsics, scene.distortion)
    T_true = se3.to_matrix(scene.T_camera_lidar_true)
    T = pose.estimate_pose_lsq(proj, kpts, pts, _perturbed_start(T_true, 2.0, 1), robust_kernel_width=10.0)
    dt, dr = se3.delta_trans_rot(scene.T_camera_lidar_true, se3.from_matrix(T))
    print(f"{camera}: |dt| {dt:.3e} m, rot {dr:.3e} rad")
    assert dt <= 1e-6 and dr <= 1e-6, (dt, dr)


def test_lsq_with_rounded_keypoints_and_gross_outliers_reaches_a_stationary_point():
    """Integer-rounded keypoints, 30 % of them uniform in the image.  Conditions: the robust cost at the returned pose is not
    above the cost at the truth, and the manifold gradient J^T rho' r has fallen to 1e-4 of its norm at the start.  The distance to
    the truth is recorded in profiles/initial_guess_auto.json (tools/ransac_time.py writes it; no bar on it)."""
    scene, kpts, pts, _ = pose_oracle.make_correspondences("pinhole_vga", 500, 0.3, seed=4, integer=True)
    proj = nid.create_camera(scene.model, scene.intrinsics, scene.distortion)
    T_true = se3.to_matrix(scene.T_camera_lidar_true)
    T0 = _perturbed_start(T_true, 2.0, 2)
    T = pose.estimate_pose_lsq(proj, kpts, pts, T0, robust_kernel_width=10.0)
    c_true, _ = pose.robust_cost_and_gradient(proj, kpts, pts, scene.T_camera_lidar_true, 10.0)
    c0, g0 = pose.robust_cost_and_gradient(proj, kpts, pts, se3.from_matrix(T0), 10.0)
    c1, g1 = pose.robust_cost_and_gradient(proj, kpts, pts, se3.from_matrix(T), 10.0)
    dt, dr = se3.delta_trans_rot(scene.T_camera_lidar_true, se3.from_matrix(T))
    print(f"cost start {c0:.6f} truth {c_true:.6f} returned {c1:.6f}; |g| start {np.linalg.norm(g0):.3e} returned {np.linalg.norm(g1):.3e}; |dt| {dt:.3e} m rot {dr:.3e} rad")
    assert c1 <= c_true
    assert np.linalg.norm(g1) <= 1e-4 * np.linalg.norm(g0)


def test_the_jacobian_of_the_reprojection_terms_is_the_derivative_of_plus():
    scene, kpts, pts, _ = pose_oracle.make_correspondences("fisheye_1080p", 20, 0.0, seed=5)
    proj = nid.create_camera(scene.model, scene.intrinsics, scene.distortion)
    x = scene.T_camera_lidar_init
    r, J = pose.reprojection_terms(proj, kpts, pts, x)
    for k in range(6):
        d = np.zeros(6)
        d[k] = 1e-6
        rp, _ = pose.reprojection_terms(proj, kpts, pts, se3.plus(x, d))
        rm, _ = pose.reprojection_terms(proj, kpts, pts, se3.plus(x, -d))
        assert np.allclose((rp - rm) / 2e-6, J[:, :, k], rtol=1e-5, atol=1e-4), k


def _write_index_png(path, idx):
    idx4 = np.ascontiguousarray(idx, dtype="<i4").view(np.uint8).reshape(idx.shape[0], idx.shape[1], 4)
    dataset.write_png(path, idx4[:, :, [2, 1, 0, 3]])  # as dataset.write_preprocessed stores it


def test_read_correspondences_keeps_the_references_behaviour_on_blank_pixels(tmp_path):
    d = str(tmp_path)
    idx = np.full((6, 8), -1, dtype=np.int32)
    idx[2, 3] = 7        # a valid pixel ...
    idx[4, 6] = 70000    # (an index that needs more than two bytes)
    idx[0, 0] = 0
    _write_index_png(os.path.join(d, "bag_lidar_indices.png"), idx)
    assert np.array_equal(pose.read_index_image(os.path.join(d, "bag_lidar_indices.png")), idx)
    points = np.column_stack([np.arange(70001.0), np.arange(70001.0) * 2, np.arange(70001.0) * 3, np.ones(70001)])
    matches = {
        # kpts1: [0] the blank pixel (4, 2) NEXT TO the valid (3, 2); [1] the valid pixel; [2] far blank; [3] (6, 4); [4] (0, 0)
        "kpts1": [4, 2, 3, 2, 0, 5, 6, 4, 0, 0],
        "kpts0": [10, 11, 20, 21, 30, 31, 40, 41, 50, 51, 60, 61],
        # keypoint 0 -> blank next to valid (dropped, no warning), 1 -> unmatched, 2 -> (6, 4) out of order, 3 -> valid pixel,
        # 4 -> far blank (dropped with the warning), 5 -> (0, 0)
        "matches": [0, -1, 3, 1, 2, 4],
        "confidence": [1.0] * 6,
    }
    with open(os.path.join(d, "bag_matches.json"), "w") as f:
        json.dump(matches, f)
    warnings = []
    kp, pts = pose.read_correspondences(d, "bag", points, log=warnings.append)
    assert kp.tolist() == [[30.0, 31.0], [40.0, 41.0], [60.0, 61.0]]
    assert pts[:, 0].tolist() == [70000.0, 7.0, 0.0] and pts.shape == (3, 4)
    assert warnings == ["warning: ignore keypoint in a blank region!!"]
    with pytest.raises(FileNotFoundError, match=r"error: failed to open .*other_matches\.json"):
        pose.read_correspondences(d, "other", points)


def _numpy_ransac_stage(proj, kpts_2d, dirs_camera, dirs_lidar, iterations, error_thresh, device=0, seed=0, pairs=None):
    """Stand-in for pose.ransac_rotation (the GPU stage): the numpy restatement on the hypotheses of the host sampler."""
    cam = (proj.model, proj.intrinsics, proj.distortion)
    if pairs is None:
        pairs = pose.sample_pairs(seed, len(kpts_2d), iterations)
    r = pose_oracle.ransac(cam, np.asarray(kpts_2d), dirs_camera, dirs_lidar, pairs, error_thresh)
    return r["Rs"][r["best"]], r["best"], int(r["counts"][r["best"]]), r["flags"], r["counts"].astype(np.int32)


def test_command_line_round_trip_of_calib_json(tmp_path, monkeypatch, capsys):
    """initial_guess_auto.main on a directory written by dataset.write_preprocessed + a matches file: every other key of calib.json
    is preserved, results.init_T_lidar_camera_auto holds the INVERSE pose with a unit quaternion, and calibrate picks it up."""
    monkeypatch.setattr(pose, "ransac_rotation", _numpy_ransac_stage)
    scene = synth.make_scene("pinhole_vga", num_points=20000, seed=11)
    cam = (scene.model, scene.intrinsics, scene.distortion)
    T_true = se3.to_matrix(scene.T_camera_lidar_true)
    _, idx = oracle_lib.generate_lidar_image(scene.model, scene.intrinsics, scene.distortion, scene.width, scene.height, scene.points, scene.intensities, T_true)
    d = str(tmp_path / "data")
    dataset.write_preprocessed(d, cam, [("bag0", scene.image_u8, scene.points, scene.intensities)], meta={"note": "kept"}, lidar_images={"bag0": (np.zeros(idx.shape), idx)})
    config = dataset.read_calib(d)
    config["results"] = {"other_result": [1, 2, 3]}
    dataset.write_calib(d, config)

    rng = np.random.default_rng(0)
    vs, us = np.nonzero(idx >= 0)
    pick = rng.choice(len(us), size=200, replace=False)
    points_f32 = scene.points.astype(np.float32).astype(np.float64)
    pc = points_f32[idx[vs[pick], us[pick]], :3] @ T_true[:3, :3].T + T_true[:3, 3]
    uv = oracle_lib.project(scene.model, scene.intrinsics, scene.distortion, pc)
    kpts0 = np.trunc(uv).astype(int)
    kpts1 = np.stack([us[pick], vs[pick]], axis=1)
    with open(os.path.join(d, "bag0_matches.json"), "w") as f:
        json.dump({"kpts0": kpts0.reshape(-1).tolist(), "kpts1": kpts1.reshape(-1).tolist(), "matches": list(range(200)), "confidence": [1.0] * 200}, f)

    assert initial_guess_auto.main([d, "--ransac_iterations", "64", "--seed", "3"]) == 0
    text = capsys.readouterr().out
    assert "--- T_camera_lidar (RANSAC) ---" in text and "--- T_camera_lidar (LSQ) ---" in text and "num_inliers: " in text and "/ 200" in text

    after = dataset.read_calib(d)
    assert after["meta"] == config["meta"] and after["camera"] == config["camera"] and after["results"]["other_result"] == [1, 2, 3]
    values = after["results"]["init_T_lidar_camera_auto"]
    assert len(values) == 7 and abs(np.linalg.norm(values[3:]) - 1.0) < 1e-12
    got, key = dataset.init_T_lidar_camera(after)
    assert key == "init_T_lidar_camera_auto" and got == values
    # the stored pose is T_lidar_camera: its inverse is the camera-from-LiDAR pose, near the truth (truncated keypoints: ~1 px)
    dt, dr = se3.delta_trans_rot(scene.T_camera_lidar_true, dataset.tum_to_T_camera_lidar(values))
    assert dt < 0.05 and dr < 0.01, (dt, dr)
    lines = []
    args = calibrate.build_parser().parse_args([d, "--dry_run"])
    calibrate.run(args, log=lines.append)
    assert "use automatically estimated initial guess" in lines


def test_a_ransac_without_any_inlier_is_refused_before_the_least_squares(monkeypatch):
    """Keypoints a million pixels away from every projection: every hypothesis of the stand-in counts 0 inliers and the winner is
    iteration 0.  estimate_rotation_ransac raises instead of handing that rotation to the least squares; so does a stage that
    returns a rotation that is not finite (what the device returns when every hypothesis is degenerate)."""
    monkeypatch.setattr(pose, "ransac_rotation", _numpy_ransac_stage)
    scene, kpts, pts, _ = pose_oracle.make_correspondences("pinhole_vga", 50, 0.0, seed=6, num_points=5000)
    proj = nid.create_camera(scene.model, scene.intrinsics, scene.distortion)
    pe = pose.PoseEstimation(pose.PoseEstimationParams(ransac_iterations=16))
    R, flags = pe.estimate_rotation_ransac(proj, kpts, pts, seed=1)
    assert pe.last_ransac["best_inliers"] == int(flags.sum()) > 0 and np.isfinite(R).all()
    with pytest.raises(ValueError, match="no hypothesis with an inlier"):
        pe.estimate_rotation_ransac(proj, kpts + 1e6, pts, seed=1)
    assert pe.last_ransac["best_iteration"] == 0 and pe.last_ransac["best_inliers"] == 0 and not pe.last_ransac["counts"].any()
    with pytest.raises(ValueError, match="no hypothesis with an inlier"):
        pe.estimate(proj, kpts + 1e6, pts, seed=1)

    def all_degenerate(proj, kpts_2d, dirs_camera, dirs_lidar, iterations, error_thresh, device=0, seed=0, pairs=None):
        return np.full((3, 3), np.nan), 0, 0, np.zeros(len(kpts_2d), dtype=bool), np.zeros(iterations, dtype=np.int32)

    monkeypatch.setattr(pose, "ransac_rotation", all_degenerate)
    with pytest.raises(ValueError, match="no hypothesis with an inlier"):
        pe.estimate_rotation_ransac(proj, kpts, pts)


def test_command_line_errors(tmp_path, monkeypatch):
    monkeypatch.setattr(pose, "ransac_rotation", _numpy_ransac_stage)
    empty = str(tmp_path / "empty")
    os.makedirs(empty)
    with pytest.raises(FileNotFoundError, match=r"error: failed to open .*calib\.json"):
        initial_guess_auto.main([empty])
    scene = synth.make_scene("pinhole_vga", num_points=2000, seed=12)
    d = str(tmp_path / "data")
    idx = np.full((scene.height, scene.width), -1, dtype=np.int32)
    idx[5, 5] = 3
    dataset.write_preprocessed(d, (scene.model, scene.intrinsics, scene.distortion), [("bag0", scene.image_u8, scene.points, scene.intensities)],
                               lidar_images={"bag0": (np.zeros(idx.shape), idx)})
    with pytest.raises(FileNotFoundError, match=r"error: failed to open .*bag0_matches\.json"):
        initial_guess_auto.main([d])
    with open(os.path.join(d, "bag0_matches.json"), "w") as f:
        json.dump({"kpts0": [1, 2, 3, 4], "kpts1": [5, 5, 9, 9], "matches": [0, 1], "confidence": [1.0, 1.0]}, f)
    with pytest.raises(SystemExit, match="1 usable correspondences; the rotation needs at least two"):
        initial_guess_auto.main([d])
    assert "results" not in dataset.read_calib(d)


def test_ransac_entry_point_refuses_bad_arguments_before_any_device_call():
    proj = nid.create_camera("plumb_bob", [400.0, 400.0, 320.0, 240.0], [])
    kp, d3 = np.zeros((4, 2)), np.tile([0.0, 0.0, 1.0], (4, 1))
    for kwargs, n in (({"iterations": 0}, 4), ({"iterations": -1}, 4), ({"iterations": 8}, 1)):
        with pytest.raises(RuntimeError, match=r"nidreg_estimate_rotation_ransac failed \(-1\)"):
            pose.ransac_rotation(proj, kp[:n], d3[:n], d3[:n], kwargs["iterations"], 5.0)
    with pytest.raises(RuntimeError, match="sample_pairs index out of range"):
        pose.ransac_rotation(proj, kp, d3, d3, 2, 5.0, pairs=[[0, 1], [2, 4]])
    proj.model_id = 9
    with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
        pose.ransac_rotation(proj, kp, d3, d3, 8, 5.0)
