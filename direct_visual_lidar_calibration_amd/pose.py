"""Pose from 2D-3D correspondences: the reference's ``vlcal::PoseEstimation`` (src/vlcal/common/estimate_pose.cpp).

=========================================  ==========================================================
here                                       reference
=========================================  ==========================================================
``PoseEstimationParams``                   include/vlcal/common/estimate_pose.hpp (the header's defaults)
``PoseEstimation.estimate``                ``PoseEstimation::estimate`` (estimate_pose.cpp:20-38)
``PoseEstimation.estimate_rotation_ransac``  ``estimate_rotation_ransac`` (:40-145): bearings on the host
                                           (``nidreg_estimate_directions``), the hypothesis loop on the GPU
                                           (``nidreg_estimate_rotation_ransac``)
``PoseEstimation.estimate_pose_lsq``       ``estimate_pose_lsq`` (:148-177) over ``ReprojectionCost``
                                           (include/vlcal/costs/reprojection_cost.hpp): host code
``read_correspondences``                   ``InitialGuessAuto::read_correspondences`` (src/initial_guess_auto.cpp:61-111)
=========================================  ==========================================================

The RANSAC loop -- iterations x correspondences projections through the camera model -- is the only heavy part and the only
one on the device; there is no CPU implementation of it here.  The least squares is a 6-parameter problem over a few
thousand residuals: numpy on the host, like the reference's Ceres.
"""
import ctypes
import json
import os
from dataclasses import dataclass

import numpy as np

from . import _lib, dataset, se3


@dataclass
class PoseEstimationParams:  # estimate_pose.hpp
    ransac_iterations: int = 8192
    ransac_error_thresh: float = 5.0
    robust_kernel_width: float = 10.0


def _dp(a):
    return None if a is None else a.ctypes.data_as(_lib.c_double_p)


def _i32p(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def estimate_directions(proj, kpts_2d):
    """``estimate_direction`` (estimate_fov.cpp:17-34) for every pixel of ``kpts_2d`` (n, 2): (n, 3) bearings.  Host code."""
    uv = np.ascontiguousarray(np.asarray(kpts_2d, dtype=np.float64).reshape(-1, 2))
    dirs = np.empty((uv.shape[0], 3))
    rc = _lib.load().nidreg_estimate_directions(proj.model_id, _dp(proj._intr5), _dp(proj._dist8), _dp(uv), uv.shape[0], _dp(dirs))
    _lib.check(rc, "nidreg_estimate_directions")
    return dirs


def sample_pairs(seed, n, iterations):
    """The hypotheses the device draws for ``(seed, n)``: (iterations, 2) distinct indices (``nidreg_ransac_sample_pairs``)."""
    pairs = np.empty((int(iterations), 2), dtype=np.int32)
    _lib.check(_lib.load().nidreg_ransac_sample_pairs(int(seed), int(n), int(iterations), _i32p(pairs)), "nidreg_ransac_sample_pairs")
    return pairs


def ransac_rotation(proj, kpts_2d, dirs_camera, dirs_lidar, iterations, error_thresh, device=0, seed=0, pairs=None):
    """``nidreg_estimate_rotation_ransac``: ``(R_camera_lidar (3, 3), best_iteration, best_inliers, flags (n,) bool, counts
    (iterations,) int32)``.  ``pairs`` (iterations, 2) dictates the hypotheses; ``None`` draws them from ``seed``."""
    kp = np.ascontiguousarray(kpts_2d, dtype=np.float64).reshape(-1, 2)
    dc = np.ascontiguousarray(dirs_camera, dtype=np.float64).reshape(-1, 3)
    dl = np.ascontiguousarray(dirs_lidar, dtype=np.float64).reshape(-1, 3)
    n = kp.shape[0]
    if dc.shape[0] != n or dl.shape[0] != n:
        raise ValueError("kpts_2d, dirs_camera and dirs_lidar must have one row per correspondence")
    if pairs is not None:
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        if pairs.shape[0] != int(iterations):
            raise ValueError("pairs must be (iterations, 2)")
    R = np.empty(9)
    best_k, best_n = ctypes.c_int32(-1), ctypes.c_int32(0)
    flags = np.zeros(n, dtype=np.uint8)
    counts = np.zeros(max(int(iterations), 0), dtype=np.int32)
    rc = _lib.load().nidreg_estimate_rotation_ransac(
        proj.model_id, _dp(proj._intr5), _dp(proj._dist8), int(device), _dp(kp), _dp(dc), _dp(dl), n, int(iterations), float(error_thresh), int(seed), _i32p(pairs), _dp(R),
        ctypes.byref(best_k), ctypes.byref(best_n), flags.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), _i32p(counts))
    _lib.check(rc, "nidreg_estimate_rotation_ransac")
    return R.reshape(3, 3), int(best_k.value), int(best_n.value), flags.astype(bool), counts


def _cauchy(s, width):
    """ceres::CauchyLoss(width): rho(s) = b log(1 + s / b), b = width^2; returns (rho, rho')."""
    b = float(width) ** 2
    return b * np.log1p(s / b), 1.0 / (1.0 + s / b)


def reprojection_terms(proj, kpts_2d, points_3d, x):
    """Residuals (n, 2) of ``ReprojectionCost`` at the Sophus-order pose ``x`` and their Jacobians (n, 2, 6) with respect to the
    right-multiplicative update ``T <- T exp(delta)``, delta = [upsilon; omega] (``Sophus::Manifold<SE3>::Plus``): the camera-frame
    point moves by R (upsilon + omega x p), so d r / d delta = J_proj [R, -R hat(p)].  Projection and its 2x3 Jacobian come from
    the device's scalar projection code compiled for the host (``nidreg_project_model(..., NIDREG_DEVICE_HOST, ...)``)."""
    p = np.asarray(points_3d, dtype=np.float64)[:, :3]
    R = se3.quat_to_rot(x[:4])
    pc = p @ R.T + x[4:7]
    uv, jp = proj.project(pc, device=-1, jacobian=True)
    r = uv - np.asarray(kpts_2d, dtype=np.float64)
    n = p.shape[0]
    hat = np.zeros((n, 3, 3))
    hat[:, 0, 1], hat[:, 0, 2] = -p[:, 2], p[:, 1]
    hat[:, 1, 0], hat[:, 1, 2] = p[:, 2], -p[:, 0]
    hat[:, 2, 0], hat[:, 2, 1] = -p[:, 1], p[:, 0]
    JR = jp @ R  # (n, 2, 3)
    J = np.concatenate([JR, -(JR @ hat)], axis=2)
    return r, J


def robust_cost_and_gradient(proj, kpts_2d, points_3d, x, robust_kernel_width):
    """What ``estimate_pose_lsq`` minimises, 1/2 sum rho(|r_i|^2) (Ceres' convention), and its manifold gradient
    sum J_i^T rho'_i r_i at the pose ``x``.  A residual that is not finite is left out of both (Ceres would fail the solve)."""
    r, J = reprojection_terms(proj, kpts_2d, points_3d, x)
    ok = np.isfinite(r).all(axis=1) & np.isfinite(J).all(axis=(1, 2))
    r, J = r[ok], J[ok]
    rho, rho1 = _cauchy((r * r).sum(axis=1), robust_kernel_width)
    return 0.5 * float(rho.sum()), np.einsum("nij,ni,n->j", J, r, rho1)


def estimate_pose_lsq(proj, kpts_2d, points_3d, init_T_camera_lidar, robust_kernel_width=10.0, log=None):
    """estimate_pose.cpp:148-177: minimise the Cauchy-robustified reprojection error over SE(3), starting at
    ``init_T_camera_lidar`` (4x4).  Returns the 4x4 ``T_camera_lidar``.  Host code; needs no GPU.

    The robust loss enters the way Ceres' corrector (Triggs) puts it there: residual and Jacobian of a block are scaled by
    sqrt(rho') and, where rho'' > 0 only, corrected by the second-order term -- the Cauchy loss has rho'' < 0 everywhere, for
    which Ceres drops that term, so the corrector IS iteratively re-weighted least squares with weights rho'.  The optimiser is
    Levenberg-Marquardt with Ceres' documented defaults (at most 50 iterations, initial trust-region radius 1e4, step
    acceptance at a relative decrease of 1e-3, radius update radius / max(1/3, 1 - (2 q - 1)^3), on rejection radius / 2, 4, 8...;
    function / gradient / parameter tolerances 1e-6 / 1e-10 / 1e-8; diagonal clamped to [1e-6, 1e32]); the 6x6 system is solved
    in numpy where Ceres runs DENSE_QR on the stacked Jacobian.  Ceres' own arithmetic is not reproduced."""
    kp = np.asarray(kpts_2d, dtype=np.float64).reshape(-1, 2)
    pts = np.asarray(points_3d, dtype=np.float64)
    x = se3.from_matrix(np.asarray(init_T_camera_lidar, dtype=np.float64))

    def linearise(xx):
        r, J = reprojection_terms(proj, kp, pts, xx)
        ok = np.isfinite(r).all(axis=1) & np.isfinite(J).all(axis=(1, 2))
        r, J = r[ok], J[ok]
        rho, rho1 = _cauchy((r * r).sum(axis=1), robust_kernel_width)
        w = np.sqrt(rho1)
        rs = (r * w[:, None]).reshape(-1)
        Js = (J * w[:, None, None]).reshape(-1, 6)
        return 0.5 * float(rho.sum()), Js.T @ rs, Js.T @ Js

    def cost_at(xx):
        r, _ = reprojection_terms(proj, kp, pts, xx)
        r = r[np.isfinite(r).all(axis=1)]
        return 0.5 * float(_cauchy((r * r).sum(axis=1), robust_kernel_width)[0].sum())

    radius, decrease = 1e4, 2.0
    cost, g, H = linearise(x)
    why = "max_num_iterations"
    it = 0
    for it in range(50):
        if np.abs(g).max() <= 1e-10:
            why = "gradient_tolerance"
            break
        D = np.clip(np.diag(H), 1e-6, 1e32) / radius
        try:
            delta = np.linalg.solve(H + np.diag(D), -g)
        except np.linalg.LinAlgError:
            delta = None
        good = delta is not None and np.all(np.isfinite(delta))
        if good:
            if np.linalg.norm(delta) <= 1e-8 * (np.linalg.norm(x) + 1e-8):
                why = "parameter_tolerance"
                break
            x_new = se3.plus(x, delta)
            new_cost = cost_at(x_new)
            model_change = -float(delta @ (g + 0.5 * (H @ delta)))
            q = (cost - new_cost) / model_change if model_change > 0.0 else -1.0
            good = np.isfinite(new_cost) and q > 1e-3
        if good:
            change = cost - new_cost
            x = x_new
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * q - 1.0) ** 3))
            decrease = 2.0
            old_cost = cost
            cost, g, H = linearise(x)
            if abs(change) <= 1e-6 * old_cost:
                why = "function_tolerance"
                break
        else:
            radius /= decrease
            decrease *= 2.0
            if radius < 1e-32:
                why = "trust_region_too_small"
                break
    if log:
        log(f"LM: {it + 1} iterations, final cost {cost:.6e}, {why}")
    return se3.to_matrix(x)


class PoseEstimation:
    """``vlcal::PoseEstimation``"""

    def __init__(self, params=None):
        self.params = params or PoseEstimationParams()

    def estimate(self, proj, kpts_2d, points_3d, device=0, seed=0, log=None):
        """estimate_pose.cpp:20-38: rotation by RANSAC, then the pose by least squares from (R, t = 0).  ``kpts_2d`` (n, 2)
        pixels, ``points_3d`` (n, 3 or 4) LiDAR points.  Returns ``(T_camera_lidar 4x4, inlier_flags (n,) bool)``."""
        R, flags = self.estimate_rotation_ransac(proj, kpts_2d, points_3d, device=device, seed=seed, log=log)
        T = np.eye(4)
        T[:3, :3] = R
        if log:
            log("--- T_camera_lidar (RANSAC) ---")
            log(str(T))
        T = self.estimate_pose_lsq(proj, kpts_2d, points_3d, T, log=log)
        if log:
            log("--- T_camera_lidar (LSQ) ---")
            log(str(T))
        return T, flags

    def estimate_rotation_ransac(self, proj, kpts_2d, points_3d, device=0, seed=0, pairs=None, log=None):
        """estimate_pose.cpp:40-145.  Returns ``(R_camera_lidar (3, 3), inlier_flags)``; ``self.last_ransac`` keeps the winning
        iteration, its inlier count and every hypothesis' count.  Raises ``ValueError`` when no hypothesis has an inlier (the
        winner is then iteration 0 and, if that pair is degenerate, its rotation is not finite)."""
        kp = np.asarray(kpts_2d, dtype=np.float64).reshape(-1, 2)
        p = np.asarray(points_3d, dtype=np.float64)[:, :3]
        if log:
            log("estimating bearing vectors")
        dirs_camera = estimate_directions(proj, kp)
        norm = np.linalg.norm(p, axis=1, keepdims=True)
        dirs_lidar = np.where(norm > 0.0, p / np.where(norm > 0.0, norm, 1.0), p)  # Eigen normalized(): unchanged at norm 0
        if log:
            log("estimating rotation using RANSAC")
        R, best_k, best_n, flags, counts = ransac_rotation(proj, kp, dirs_camera, dirs_lidar, self.params.ransac_iterations, self.params.ransac_error_thresh, device=device, seed=seed,
                                                           pairs=pairs)
        self.last_ransac = {"best_iteration": best_k, "best_inliers": best_n, "counts": counts}
        if best_n <= 0 or not np.isfinite(R).all():
            # every hypothesis was degenerate (coincident or opposite bearings: its rotation is NaN) or fitted nothing; the
            # reference would hand its uninitialised best rotation on to the least squares
            raise ValueError(f"estimate_rotation_ransac: no hypothesis with an inlier among {len(counts)} ({kp.shape[0]} correspondences, threshold {self.params.ransac_error_thresh} px)")
        if log:
            log(f"num_inliers: {best_n} / {kp.shape[0]}")
        return R, flags

    def estimate_pose_lsq(self, proj, kpts_2d, points_3d, init_T_camera_lidar, log=None):
        """estimate_pose.cpp:148-177 (all correspondences enter, inliers or not: the Cauchy loss does the rejecting)."""
        return estimate_pose_lsq(proj, kpts_2d, points_3d, init_T_camera_lidar, self.params.robust_kernel_width, log=log)


def read_index_image(path):
    """``<bag>_lidar_indices.png`` as int32 (H, W): the CV_8UC4 buffer reinterpreted (initial_guess_auto.cpp:63-64).  The PNG
    stores RGBA where OpenCV's buffer is BGRA -- the channel order ``dataset.write_preprocessed`` writes, undone here."""
    img, depth = dataset.read_png(path)
    if depth != 8 or img.ndim != 3 or img.shape[2] != 4:
        raise ValueError(f"{path}: an 8-bit RGBA index image expected")
    return np.ascontiguousarray(img[:, :, [2, 1, 0, 3]]).view("<i4").reshape(img.shape[0], img.shape[1]).astype(np.int32)


_PICK_OFFSETS = sorted(((i, j) for i in (-1, 0, 1) for j in (-1, 0, 1) if (i, j) != (0, 0)), key=lambda o: o[0] * o[0] + o[1] * o[1])


def read_correspondences(data_path, bag_name, points, log=None):
    """initial_guess_auto.cpp:61-111: the 2D-3D correspondences of one bag from ``<bag>_matches.json`` (``kpts0`` camera pixels,
    ``kpts1`` LiDAR-image pixels, flat integer lists; ``matches[i]`` = index into kpts1 or < 0) and ``<bag>_lidar_indices.png``.
    Returns ``(kpts_2d (m, 2) float64, points (m, 4))``."""
    matches_path = os.path.join(data_path, bag_name + "_matches.json")
    if not os.path.exists(matches_path):
        raise FileNotFoundError(f"error: failed to open {matches_path}")
    indices = read_index_image(os.path.join(data_path, bag_name + "_lidar_indices.png"))
    with open(matches_path) as f:
        result = json.load(f)
    kpts0, kpts1, matches = result["kpts0"], result["kpts1"], result["matches"]
    H, W = indices.shape
    pts = np.asarray(points, dtype=np.float64)
    kps, picked = [], []
    for i, m in enumerate(matches):
        if m < 0:
            continue
        x1, y1 = int(kpts1[2 * m]), int(kpts1[2 * m + 1])
        if not (0 <= x1 < W and 0 <= y1 < H):
            raise ValueError(f"{matches_path}: keypoint ({x1}, {y1}) outside the {W}x{H} index image")
        index = int(indices[y1, x1])
        if index < 0:
            # initial_guess_auto.cpp:92-104: the reference searches the 8 neighbours for a point and then `continue`s REGARDLESS
            # of what it found, so a keypoint on a blank pixel is always dropped; the search only decides whether it warns.
            # Kept as it is: the matches a reference run uses are the matches used here.
            if log and all(indices[y1 + dy, x1 + dx] < 0 for dx, dy in _PICK_OFFSETS if 0 <= x1 + dx < W and 0 <= y1 + dy < H):
                log("warning: ignore keypoint in a blank region!!")
            continue
        if index >= pts.shape[0]:
            raise ValueError(f"{matches_path}: point index {index} beyond the cloud ({pts.shape[0]} points)")
        kps.append((float(int(kpts0[2 * i])), float(int(kpts0[2 * i + 1]))))
        picked.append(index)
    return np.array(kps, dtype=np.float64).reshape(-1, 2), pts[np.array(picked, dtype=np.int64)].reshape(-1, pts.shape[1])
