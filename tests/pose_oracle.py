"""numpy / oracle restatement of PoseEstimation::estimate_rotation_ransac (src/vlcal/common/estimate_pose.cpp:40-145) and the
scenes the pose tests share -- TEST INFRASTRUCTURE ONLY (tests/test_pose_host.py, tests/test_pose_gpu.py, tools/ransac_time.py).
The rotation is numpy's SVD with the reference's S = diag(1, 1, det U det V); the projection is the CPU oracle's."""
import math

import numpy as np

import oracle_lib

DELTA_PX = 1e-4  # the decision band: a count may differ from the oracle's only through errors within DELTA of the threshold


def to_dir(x):
    """estimate_fov.cpp:19-21: AngleAxis(x0, X) * AngleAxis(x1, Y) * UnitZ through quaternions, as Eigen evaluates it."""
    aw, ax = math.cos(0.5 * x[0]), math.sin(0.5 * x[0])
    bw, by = math.cos(0.5 * x[1]), math.sin(0.5 * x[1])
    qw, qx, qy, qz = aw * bw, ax * bw, aw * by, ax * by
    ux, uy, uz = 2.0 * qy, -2.0 * qx, 0.0
    return np.array([qw * ux + (qy * uz - qz * uy), qw * uy + (qz * ux - qx * uz), (1.0 + qw * uz) + (qx * uy - qy * ux)])


def estimate_direction(model, intr, dist, pt_2d):
    """estimate_fov.cpp:17-34 over the oracle's Nelder-Mead and the oracle's projection."""
    big = float(np.finfo(np.float64).max)

    def f(x):
        uv = oracle_lib.project(model, intr, dist, to_dir(x))[0]
        err = float((pt_2d[0] - uv[0]) ** 2 + (pt_2d[1] - uv[1]) ** 2)
        return err if math.isfinite(err) else big

    return to_dir(oracle_lib.nelder_mead(f, np.zeros(2))["x"])


def rotation_svd(a1, a2, b1, b2):
    """find_rotation (estimate_pose.cpp:55-83) for two correspondences: camera bearings a, LiDAR bearings b."""
    A = np.stack([a1, a2], axis=1)
    B = np.stack([b1, b2], axis=1)
    U, _, Vt = np.linalg.svd(A @ B.T)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0.0:
        S[2, 2] = -1.0
    return U @ S @ Vt


def errors(camera, kpts, dirs_lidar, R):
    """|kp - project(R d_lidar)| in pixels per correspondence (NaN where the projection is not finite)."""
    model, intr, dist = camera
    uv = oracle_lib.project(model, intr, dist, dirs_lidar @ R.T)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(((kpts - uv) ** 2).sum(axis=1))


def count_band(err, thresh, delta=DELTA_PX):
    """(#{err < t - delta}, #{err < t + delta}); NaN is an outlier in both."""
    with np.errstate(invalid="ignore"):
        return int((err < thresh - delta).sum()), int((err < thresh + delta).sum())


def ransac(camera, kpts, dirs_camera, dirs_lidar, pairs, thresh):
    """The whole loop on one host core: per-hypothesis rotations, errors' counts at the threshold, the winner (largest count,
    lowest index) and its flags.  Returns dict(Rs, counts, best, flags, err_best)."""
    Rs = np.empty((len(pairs), 3, 3))
    counts = np.empty(len(pairs), dtype=np.int64)
    for k, (i, j) in enumerate(pairs):
        Rs[k] = rotation_svd(dirs_camera[i], dirs_camera[j], dirs_lidar[i], dirs_lidar[j])
        with np.errstate(invalid="ignore"):
            counts[k] = int((errors(camera, kpts, dirs_lidar, Rs[k]) < thresh).sum())
    best = int(np.argmax(counts))  # first of the maxima
    err_best = errors(camera, kpts, dirs_lidar, Rs[best])
    with np.errstate(invalid="ignore"):
        flags = err_best < thresh
    return dict(Rs=Rs, counts=counts, best=best, flags=flags, err_best=err_best)


def angle_between(u, v):
    return float(np.arctan2(np.linalg.norm(np.cross(u, v)), float(np.dot(u, v))))


def make_correspondences(camera_name, n, outlier_fraction, seed, num_points=60000, noise_px=0.0, integer=False):
    """n synthetic 2D-3D correspondences of a synth scene: points of the cloud that project inside the image under the true pose,
    keypoints = their real-valued projections (+ uniform noise of +-noise_px, rounded when ``integer``), a fraction replaced by
    pixels uniform in the image.  Returns (scene, kpts (n, 2), points (n, 4), is_outlier (n,))."""
    from direct_visual_lidar_calibration_amd import se3, synth

    scene = synth.make_scene(camera_name, num_points=num_points, seed=seed)
    T = se3.to_matrix(scene.T_camera_lidar_true)
    pc = scene.points[:, :3] @ T[:3, :3].T + T[:3, 3]
    uv = oracle_lib.project(scene.model, scene.intrinsics, scene.distortion, pc)
    inside = np.isfinite(uv).all(axis=1) & (uv[:, 0] >= 0) & (uv[:, 0] < scene.width - 1) & (uv[:, 1] >= 0) & (uv[:, 1] < scene.height - 1)
    if scene.model != "equirectangular":
        inside &= pc[:, 2] > 0.1
    rng = np.random.default_rng(seed)
    pick = rng.choice(np.flatnonzero(inside), size=n, replace=False)
    kpts = uv[pick].copy()
    if noise_px > 0.0:
        kpts += rng.uniform(-noise_px, noise_px, size=kpts.shape)
    is_outlier = np.zeros(n, dtype=bool)
    is_outlier[rng.choice(n, size=int(round(outlier_fraction * n)), replace=False)] = True
    kpts[is_outlier] = rng.uniform([0.0, 0.0], [scene.width - 1.0, scene.height - 1.0], size=(int(is_outlier.sum()), 2))
    if integer:
        kpts = np.rint(kpts)
    return scene, np.ascontiguousarray(kpts), np.ascontiguousarray(scene.points[pick]), is_outlier


def make_correspondences_without_image(camera_name, n, outlier_fraction, seed, noise_px=0.0):
    """make_correspondences without synth.make_scene's image (rendering 2048 x 2048 rays takes ten seconds a scene): n pixels
    uniform in the image, 2.5 px off its border, unprojected and cast onto the walls of synth's room from the camera centre of the
    true pose, rounded to float32 like a stored cloud.  Keypoints = the oracle's projections of those points under the true pose
    (+ uniform noise of +-noise_px), a fraction replaced by pixels uniform in the image.  Returns (camera (model, intrinsics,
    distortion), kpts (n, 2), points (n, 4), is_outlier (n,))."""
    import torch

    from direct_visual_lidar_calibration_amd import camera_models, se3, synth

    model, intr, dist, W, H = synth.CONFIG_CAMERAS[camera_name]
    T = se3.to_matrix(synth.true_T_camera_lidar())
    R, t = T[:3, :3], T[:3, 3]
    rng = np.random.default_rng(seed)
    px = rng.uniform([2.5, 2.5], [W - 2.5, H - 2.5], size=(n, 2))
    bear = camera_models.unproject(model, intr, dist, torch.tensor(px, dtype=torch.float64))
    X = synth.ray_room(-(R.T @ t), bear @ torch.tensor(R, dtype=torch.float64)).numpy().astype(np.float32).astype(np.float64)
    kpts = oracle_lib.project(model, list(intr), list(dist), X @ R.T + t)
    assert np.isfinite(kpts).all() and np.abs(kpts - px).max() < 1e-2  # (float32 points: the pixel is met to ~1e-4 px)
    if noise_px > 0.0:
        kpts += rng.uniform(-noise_px, noise_px, size=kpts.shape)
    is_outlier = np.zeros(n, dtype=bool)
    is_outlier[rng.choice(n, size=int(round(outlier_fraction * n)), replace=False)] = True
    kpts[is_outlier] = rng.uniform([0.0, 0.0], [W - 1.0, H - 1.0], size=(int(is_outlier.sum()), 2))
    points = np.concatenate([X, np.ones((n, 1))], axis=1)
    return (model, list(intr), list(dist)), np.ascontiguousarray(kpts), points, is_outlier


def unit(p):
    p = np.asarray(p, dtype=np.float64)[:, :3]
    return p / np.linalg.norm(p, axis=1, keepdims=True)
