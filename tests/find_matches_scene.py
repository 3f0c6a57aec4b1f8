"""The end-to-end scene of find_matches (tests/test_find_matches_e2e.py, tools/match_time.py): one seeded synth scene seen by the
camera and, through a 512 x 512 virtual pinhole along the LiDAR's x axis, as a LiDAR intensity image; the preprocessed directory
written with the package's own writers; correct-match bookkeeping against the true pose; ground-truth matches as the yardstick."""
import json
import os

import numpy as np

import oracle_lib
from direct_visual_lidar_calibration_amd import calibrate, dataset, initial_guess_auto, nid, pose, preprocess, render, se3, synth

CAMERA = "pinhole_vga"
SEED = 41
NUM_POINTS = 1_000_000  # about 9 points per covered LiDAR pixel: the covered part of the image has next to no blanks
LIDAR_SIZE = 512
LIDAR_FOV_DEG = 100.0
RANSAC_THRESH = 10.0  # initial_guess_auto's --ransac_error_thresh default: what "a correct match" is measured with
BAG = "bag0"

_scene = {}


def scene():
    if "s" not in _scene:
        _scene["s"] = synth.make_scene(CAMERA, num_points=NUM_POINTS, seed=SEED)
    return _scene["s"]


def lidar_view():
    """(camera object, (w, h), T_camera_lidar 4x4) of the virtual pinhole: preprocess.lidar_camera's orientation at 512 x 512."""
    fov = np.radians(LIDAR_FOV_DEG)
    _, _, _, T_lidar_camera = preprocess.lidar_camera(fov)
    fx = LIDAR_SIZE / (2.0 * np.tan(fov / 2.0))
    return nid.create_camera("plumb_bob", [fx, fx, LIDAR_SIZE / 2.0, LIDAR_SIZE / 2.0], []), (LIDAR_SIZE, LIDAR_SIZE), np.linalg.inv(T_lidar_camera)


def render_lidar(s, device=0):
    """(intensity image float64, index image int32); ``device=None``: the CPU oracle's renderer."""
    proj, size, T = lidar_view()
    if device is None:
        return oracle_lib.generate_lidar_image(proj.model, proj.intrinsics, proj.distortion, size[0], size[1], s.points, s.intensities, T)
    return render.generate_lidar_image(proj, size, T, s.points, s.intensities, device=device)


def intensities_u8(inten):
    return np.clip(np.rint(np.asarray(inten) * 255.0), 0, 255).astype(np.uint8)  # what dataset.write_preprocessed stores


def write_directory(d, s, inten, idx, stored_rotation=0):
    """The preprocessed directory of the scene.  ``stored_rotation`` (clockwise degrees) turns BOTH stored LiDAR images, as a LiDAR
    mounted on its side would deliver them."""
    k = -(stored_rotation // 90)
    inten, idx = np.ascontiguousarray(np.rot90(inten, k=k)), np.ascontiguousarray(np.rot90(idx, k=k))
    dataset.write_preprocessed(d, (s.model, s.intrinsics, s.distortion), [(BAG, s.image_u8, s.points, s.intensities)], lidar_images={BAG: (inten, idx)})
    return inten, idx


def reprojection_error(s, kpts, pts):
    """Pixels between each camera keypoint and its 3D point projected under the true pose."""
    T = se3.to_matrix(s.T_camera_lidar_true)
    pc = np.asarray(pts)[:, :3] @ T[:3, :3].T + T[:3, 3]
    uv = oracle_lib.project(s.model, s.intrinsics, s.distortion, pc)
    with np.errstate(invalid="ignore"):
        err = np.linalg.norm(uv - np.asarray(kpts), axis=1)
    return np.where((pc[:, 2] > 0) & np.isfinite(err), err, np.inf)


def ground_truth_matches(s, idx, kpts1_xy):
    """The matches file a perfect matcher would write for the LiDAR keypoints ``kpts1_xy`` (n, 2): each one's 3D point projected
    under the true pose and rounded to integer pixels; keypoints that leave the image are unmatched."""
    kpts1_xy = np.asarray(kpts1_xy, dtype=np.int64).reshape(-1, 2)
    T = se3.to_matrix(s.T_camera_lidar_true)
    index = idx[kpts1_xy[:, 1], kpts1_xy[:, 0]]
    pc = s.points[np.maximum(index, 0), :3] @ T[:3, :3].T + T[:3, 3]
    uv = np.rint(oracle_lib.project(s.model, s.intrinsics, s.distortion, pc))
    ok = (index >= 0) & (pc[:, 2] > 0.1) & (uv[:, 0] >= 0) & (uv[:, 0] < s.width) & (uv[:, 1] >= 0) & (uv[:, 1] < s.height)
    sel = np.flatnonzero(ok)
    return {"kpts0": uv[sel].astype(int).reshape(-1).tolist(), "kpts1": kpts1_xy.reshape(-1).tolist(), "matches": sel.tolist(), "confidence": [1.0] * len(sel)}


def write_matches(d, result):
    with open(os.path.join(d, BAG + "_matches.json"), "w") as f:
        json.dump(result, f)


def read_matches(d):
    with open(os.path.join(d, BAG + "_matches.json")) as f:
        return json.load(f)


def initial_guess(d, s, log=None):
    """initial_guess_auto on the directory: dict(T 4x4, dt, dr against the truth, inliers, err: reprojection error of every
    correspondence the command read, in its order)."""
    lines = []
    _, T, inliers = initial_guess_auto.run(initial_guess_auto.build_parser().parse_args([d]), log=lines.append if log is None else log)
    kp, pts = pose.read_correspondences(d, BAG, s.points)
    dt, dr = se3.delta_trans_rot(s.T_camera_lidar_true, se3.from_matrix(T))
    return dict(T=T, dt=dt, dr=dr, inliers=np.asarray(inliers, dtype=bool), err=reprojection_error(s, kp, pts), x=se3.from_matrix(T))


def run_calibrate(d):
    """calibrate on the directory from whatever initial guess calib.json holds: the Sophus-order T_camera_lidar it ends at."""
    _, _, x = calibrate.run(calibrate.build_parser().parse_args([d]), log=lambda *_: None)
    return x


def set_manual_guess(d, x):
    """results.init_T_lidar_camera (the key that takes precedence) = the pose ``x`` (Sophus order, T_camera_lidar)."""
    config = dataset.read_calib(d)
    config.setdefault("results", {})["init_T_lidar_camera"] = dataset.T_camera_lidar_to_tum(x)
    dataset.write_calib(d, config)


def clear_guesses(d):
    config = dataset.read_calib(d)
    config.pop("results", None)
    dataset.write_calib(d, config)
