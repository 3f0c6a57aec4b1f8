"""Inputs shared by tests/test_select_host.py and tests/test_select_gpu.py: a 64 x 48 camera of each of the six models, a cloud whose
points are BUILT from a pixel, a fraction in [0.25, 0.75] and a depth through the model's inverse (so that no pixel decision lies
within an ulp of a boundary: that is the cull's known libm caveat, not what these tests are about), and the masks."""
import math

import numpy as np
import torch

from direct_visual_lidar_calibration_amd import camera_models, se3
from test_image_edges import MODELS, POSE, Cam, cached

W, H = 64, 48
MARGINS = (0, 1, 2, 5)


def pose():
    """``(x7, T 4x4)``: one pose in both forms, consistent to rounding (POSE itself is orthonormal to four digits only)"""
    x7 = se3.from_matrix(POSE)
    return x7, se3.to_matrix(x7)


def pixel_cloud(model, extra=1200, outside=300, seed=5):
    """dict(cam, pts (n, 4), inten (n,), T, x7, min_z, image_u8): one point per pixel of the image plus ``extra`` on random pixels,
    at fractions in [0.25, 0.75] and depths in [2, 20] m, the last ``outside`` of
    them moved W + 4 pixels to the right, out of the image; points the inverse does not bring back to their pixel position are left out"""

    def make():
        cam = Cam(model, W, H)
        rng = np.random.default_rng(seed + MODELS.index(model))
        x7, T = pose()
        ys, xs = np.mgrid[0:H, 0:W]
        px = np.concatenate([xs.ravel(), rng.integers(0, W, extra)]).astype(np.float64)
        py = np.concatenate([ys.ravel(), rng.integers(0, H, extra)]).astype(np.float64)
        n = len(px)
        px[-outside:] += W + 4  # right of the image: the in-image test's to remove (an equirectangular image wraps them back in, at the same fraction)
        uv = np.stack([px + rng.uniform(0.25, 0.75, n), py + rng.uniform(0.25, 0.75, n)], axis=1)
        bearing = camera_models.unproject(cam.model, cam.intr, cam.dist, torch.tensor(uv, dtype=torch.float64)).numpy()
        pc = bearing * rng.uniform(2.0, 20.0, n)[:, None]
        Tinv = np.linalg.inv(T)
        pl = pc @ Tinv[:3, :3].T + Tinv[:3, 3]
        # the inverse is iterative: a point it did not bring back to its pixel position (to 1e-6 px) is not part of the cloud
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(pl).all(axis=1) & (np.abs(cam.project(pc) - uv).max(axis=1) < 1e-6)
        order = rng.permutation(int(ok.sum()))  # pixel order is not input order
        pts = np.ones((int(ok.sum()), 4))
        pts[:, :3] = pl[ok][order]
        inten = rng.integers(0, 256, len(pts)) / 256.0
        image = rng.integers(0, 256, (H, W)).astype(np.uint8)
        return dict(cam=cam, pts=np.ascontiguousarray(pts), inten=inten, T=T, x7=x7, min_z=math.cos(cam.fov()), image_u8=image)

    return cached(("select_pixel_cloud", model, extra, outside, seed), make)


def masks():
    """name -> (H, W) uint8, non-zero = use"""

    def make():
        rng = np.random.default_rng(99)
        random = np.where(rng.uniform(size=(H, W)) < 0.04, 0, rng.integers(1, 256, (H, W))).astype(np.uint8)
        striped = np.full((H, W), 255, dtype=np.uint8)
        striped[:, 10:14] = 0
        striped[30:33, :] = 0
        single = np.full((H, W), 1, dtype=np.uint8)
        single[20, 31] = 0
        return {"random": random, "striped": striped, "single": single, "zero": np.zeros((H, W), dtype=np.uint8), "valid": np.full((H, W), 255, dtype=np.uint8)}

    return cached("select_masks", make)


def padded(mask, row_stride):
    """the mask as a view into rows ``row_stride`` bytes apart, 0 between the rows (a reader that ignores the stride sees zeros)"""
    buf = np.zeros((mask.shape[0], row_stride), dtype=np.uint8)
    buf[:, : mask.shape[1]] = mask
    return buf[:, : mask.shape[1]]
