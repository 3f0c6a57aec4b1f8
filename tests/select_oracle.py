"""A numpy restatement of ``nidreg_cloud_select`` (include/nidreg.h) -- TEST INFRASTRUCTURE ONLY, written from the rules, not
from the kernels:

* the survivors are ``oracle_lib.view_culling``'s;
* a survivor's pixel is the truncation of ``oracle_lib.project`` of the point transformed as the cull transforms it (Eigen's 4x4 * 4x1,
  summed left to right);
* the eroded mask is a plain double loop: the minimum of the mask over the (2R + 1)^2 window clipped to the image;
* the range rule is ``min^2 <= (x x + y y) + z z <= max^2`` on the cloud's own coordinates.
"""
import math

import numpy as np

import oracle_lib


def erode(mask_u8, R):
    """eroded[y, x] = min of mask over [x - R, x + R] x [y - R, y + R] clipped to the image (outside counts as valid)"""
    m = np.asarray(mask_u8, dtype=np.uint8)
    H, W = m.shape
    out = np.empty_like(m)
    for y in range(H):
        for x in range(W):
            out[y, x] = m[max(y - R, 0) : min(y + R, H - 1) + 1, max(x - R, 0) : min(x + R, W - 1) + 1].min()
    return out


def camera_frame(points, T):
    """((m0 x + m1 y) + m2 z) + m3 w per row, as k_cull_zbuf and the oracle's cull evaluate it"""
    p = np.asarray(points, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    x, y, z, w = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] * w for r in range(3)], axis=1)


def pixels(model, intrinsics, distortion, points, T):
    """``(px, py, fractions (n, 2))`` of the points under ``T``: the truncated projection and what was cut off"""
    uv = oracle_lib.project(model, intrinsics, distortion, camera_frame(points, T))
    px, py = np.trunc(uv[:, 0]).astype(np.int64), np.trunc(uv[:, 1]).astype(np.int64)
    return px, py, uv - np.stack([px, py], axis=1)


def range_ok(points, min_range=0.0, max_range=math.inf):
    p = np.asarray(points, dtype=np.float64)
    r2 = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    return (r2 >= min_range * min_range) & (r2 <= max_range * max_range)


def select(model, intrinsics, distortion, width, height, points, T, depth, min_z, mask=None, margin=2, min_range=0.0, max_range=math.inf, return_parts=False):
    """The selected indices (ascending int32).  ``return_parts``: also ``dict(kept, mask_removed, range_removed, fractions)`` -- the
    counts of the three stages and the pixel fractions of the cull's survivors."""
    keep = oracle_lib.view_culling(model, intrinsics, distortion, width, height, points, T, depth, min_z=min_z)
    pts = np.asarray(points, dtype=np.float64)[keep]
    valid = np.ones(len(keep), dtype=bool)
    frac = np.zeros((len(keep), 2))
    if len(keep):
        px, py, frac = pixels(model, intrinsics, distortion, pts, T)
        if mask is not None:
            valid = erode(mask, margin)[py, px] != 0
    inside = range_ok(pts, min_range, max_range)
    idx = keep[valid & inside].astype(np.int32)
    if return_parts:
        return idx, dict(kept=int(len(keep)), mask_removed=int((~valid).sum()), range_removed=int((valid & ~inside).sum()), fractions=frac)
    return idx
