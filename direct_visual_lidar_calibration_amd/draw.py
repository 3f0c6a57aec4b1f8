"""Match pictures on the GPU: a ctypes wrapper of ``nidreg_draw`` (csrc/nid_draw_kernels.hpp: lines, rings and discs over one gray
image or two side by side, integer arithmetic, painter's order) and the two pictures built from it.

``match_picture`` is what the reference's matcher script saves as ``<bag>_superglue.png`` (scripts/find_matches_superglue.py: both
images side by side, every keypoint circled, every match a line coloured by its confidence); ``find_matches --picture`` writes it as
``<bag>_matches.png``.  Three DELIBERATE DIFFERENCES from that script:

* images and keypoints are the UNROTATED ones (``<bag>_matches.json`` holds unrotated pixels; the script draws on the rotated images);
* colours are RGB (the script hands matplotlib's RGBA to OpenCV, which reads it as BGR: its pictures have red and blue swapped);
* the LiDAR image is brought to the camera image's size by the integer bilinear rule of ``nidreg_draw`` (include/nidreg.h), not by
  ``cv2.resize``; nothing here is pinned against OpenCV.

``residual_primitives`` is the picture ``initial_guess_auto --picture`` draws in place of the window the reference opens on its
result.  There is no CPU path here (tests/draw_oracle.py is the checker's restatement); no anti-aliasing, no line width.
"""
import ctypes
import math

import numpy as np

from . import _lib
from .matching import _p, _rows_u8

LINE, RING, DISC = 0, 1, 2  # NIDREG_DRAW_*
COORD_MIN, COORD_MAX = -32768, 32767
WHITE, GREEN, RED = 0xFFFFFF, 0x00FF00, 0xFF0000
KEYPOINT_RADIUS = 3

# TURBO-BEGIN (tools/make_turbo_table.py)
TURBO = np.array([
    (48, 18, 59), (49, 21, 66), (50, 24, 74), (52, 27, 81), (53, 30, 88), (54, 33, 95), (55, 35, 101), (56, 38, 108),
    (57, 41, 114), (58, 44, 121), (59, 47, 127), (60, 50, 133), (60, 53, 139), (61, 55, 145), (62, 58, 150), (63, 61, 156),
    (64, 64, 161), (64, 67, 166), (65, 69, 171), (65, 72, 176), (66, 75, 181), (67, 78, 186), (67, 80, 190), (67, 83, 194),
    (68, 86, 199), (68, 88, 203), (69, 91, 206), (69, 94, 210), (69, 96, 214), (69, 99, 217), (70, 102, 221), (70, 104, 224),
    (70, 107, 227), (70, 109, 230), (70, 112, 232), (70, 115, 235), (70, 117, 237), (70, 120, 240), (70, 122, 242), (70, 125, 244),
    (70, 127, 246), (70, 130, 248), (69, 132, 249), (69, 135, 251), (69, 137, 252), (68, 140, 253), (67, 142, 253), (66, 145, 254),
    (65, 147, 254), (64, 150, 254), (63, 152, 254), (62, 155, 254), (60, 157, 253), (59, 160, 252), (57, 162, 252), (56, 165, 251),
    (54, 168, 249), (52, 170, 248), (51, 172, 246), (49, 175, 245), (47, 177, 243), (45, 180, 241), (43, 182, 239), (42, 185, 237),
    (40, 187, 235), (38, 189, 233), (37, 192, 230), (35, 194, 228), (33, 196, 225), (32, 198, 223), (30, 201, 220), (29, 203, 218),
    (28, 205, 215), (27, 207, 212), (26, 209, 210), (25, 211, 207), (24, 213, 204), (24, 215, 202), (23, 217, 199), (23, 218, 196),
    (23, 220, 194), (23, 222, 191), (24, 224, 189), (24, 225, 186), (25, 227, 184), (26, 228, 182), (27, 229, 180), (29, 231, 177),
    (30, 232, 175), (32, 233, 172), (34, 235, 169), (36, 236, 166), (39, 237, 163), (41, 238, 160), (44, 239, 157), (47, 240, 154),
    (50, 241, 151), (53, 243, 148), (56, 244, 145), (59, 244, 141), (63, 245, 138), (66, 246, 135), (70, 247, 131), (74, 248, 128),
    (77, 249, 124), (81, 249, 121), (85, 250, 118), (89, 251, 114), (93, 251, 111), (97, 252, 108), (101, 252, 104), (105, 253, 101),
    (109, 253, 98), (113, 253, 95), (116, 254, 92), (120, 254, 89), (124, 254, 86), (128, 254, 83), (132, 254, 80), (135, 254, 77),
    (139, 254, 75), (142, 254, 72), (146, 254, 70), (149, 254, 68), (152, 254, 66), (155, 253, 64), (158, 253, 62), (161, 252, 61),
    (164, 252, 59), (166, 251, 58), (169, 251, 57), (172, 250, 55), (174, 249, 55), (177, 248, 54), (179, 248, 53), (182, 247, 53),
    (185, 245, 52), (187, 244, 52), (190, 243, 52), (192, 242, 51), (195, 241, 51), (197, 239, 51), (200, 238, 51), (202, 237, 51),
    (205, 235, 52), (207, 234, 52), (209, 232, 52), (212, 231, 53), (214, 229, 53), (216, 227, 53), (218, 226, 54), (221, 224, 54),
    (223, 222, 54), (225, 220, 55), (227, 218, 55), (229, 216, 56), (231, 215, 56), (232, 213, 56), (234, 211, 57), (236, 209, 57),
    (237, 207, 57), (239, 205, 57), (240, 203, 58), (242, 200, 58), (243, 198, 58), (244, 196, 58), (246, 194, 58), (247, 192, 57),
    (248, 190, 57), (249, 188, 57), (249, 186, 56), (250, 183, 55), (251, 181, 55), (251, 179, 54), (252, 176, 53), (252, 174, 52),
    (253, 171, 51), (253, 169, 50), (253, 166, 49), (253, 163, 48), (254, 161, 47), (254, 158, 46), (254, 155, 45), (254, 152, 44),
    (253, 149, 43), (253, 146, 41), (253, 143, 40), (253, 140, 39), (252, 137, 38), (252, 134, 36), (251, 131, 35), (251, 128, 34),
    (250, 125, 32), (250, 122, 31), (249, 119, 30), (248, 116, 28), (247, 113, 27), (247, 110, 26), (246, 107, 24), (245, 104, 23),
    (244, 101, 22), (243, 99, 21), (242, 96, 20), (241, 93, 19), (239, 90, 17), (238, 88, 16), (237, 85, 15), (236, 82, 14),
    (234, 80, 13), (233, 77, 13), (232, 75, 12), (230, 73, 11), (229, 70, 10), (227, 68, 10), (226, 66, 9), (224, 64, 8),
    (222, 62, 8), (221, 60, 7), (219, 58, 7), (217, 56, 6), (215, 54, 6), (214, 52, 5), (212, 50, 5), (210, 48, 5),
    (208, 47, 4), (206, 45, 4), (203, 43, 3), (201, 41, 3), (199, 40, 3), (197, 38, 2), (195, 36, 2), (192, 35, 2),
    (190, 33, 2), (187, 31, 1), (185, 30, 1), (182, 28, 1), (180, 27, 1), (177, 25, 1), (174, 24, 1), (172, 22, 1),
    (169, 21, 1), (166, 20, 1), (163, 18, 1), (160, 17, 1), (157, 16, 1), (154, 14, 1), (151, 13, 1), (148, 12, 1),
    (145, 11, 1), (142, 10, 1), (139, 9, 1), (135, 8, 1), (132, 7, 1), (129, 6, 2), (125, 5, 2), (122, 4, 2),
], dtype=np.uint8)
# TURBO-END


def _rgb(c):
    """0xRRGGBB from an integer or an (r, g, b) triple"""
    if isinstance(c, (int, np.integer)):
        return int(c)
    r, g, b = (int(v) for v in c)
    if not all(0 <= v <= 255 for v in (r, g, b)):
        raise ValueError("colour channels must lie in [0, 255]")
    return (r << 16) | (g << 8) | b


def line(x0, y0, x1, y1, rgb):
    """A ``nidreg_draw`` record: the one-pixel-wide line FROM (x0, y0) to (x1, y1)"""
    return [LINE, int(x0), int(y0), int(x1), int(y1), _rgb(rgb), 0, 0]


def ring(x, y, radius, rgb):
    return [RING, int(x), int(y), int(radius), 0, _rgb(rgb), 0, 0]


def disc(x, y, radius, rgb):
    return [DISC, int(x), int(y), int(radius), 0, _rgb(rgb), 0, 0]


def draw(left, right, prims, device=0):
    """``nidreg_draw``: the (H, W, 3) or -- with a ``right`` image, resized to the left one's size -- (H, 2 W, 3) uint8 RGB picture of
    ``prims`` (records of ``line`` / ``ring`` / ``disc``, or an (n, 8) integer array) over the gray images.  Later primitives lie over
    earlier ones.  Row-padded views are passed as they are."""
    l = _rows_u8(left, "draw: left image")
    r = None if right is None else _rows_u8(right, "draw: right image")
    pr = np.asarray(prims if len(prims) else np.zeros((0, 8)), dtype=np.int64)
    if pr.ndim != 2 or pr.shape[1] != 8:
        raise ValueError("draw: primitives are records of 8 integers")
    if pr.size and (pr.min() < -2 ** 31 or pr.max() >= 2 ** 31):
        raise ValueError("draw: a primitive field beyond 32 bits")
    pr = np.ascontiguousarray(pr, dtype=np.int32)
    H, W = l.shape
    out = np.empty((H, W if r is None else 2 * W, 3), dtype=np.uint8)
    rc = _lib.load().nidreg_draw(int(device), _p(l, ctypes.c_uint8), W, H, l.strides[0] if l.size else W, _p(r, ctypes.c_uint8), 0 if r is None else r.shape[1],
                                 0 if r is None else r.shape[0], 0 if r is None else (r.strides[0] if r.size else r.shape[1]), pr.shape[0],
                                 _p(pr, ctypes.c_int32) if pr.shape[0] else None, _p(out, ctypes.c_uint8))
    _lib.check(rc, "nidreg_draw")
    return out


def _keypoints(flat, width, height, what):
    """A flat x, y list as (n, 2) integers; floats (the reference script's file) are truncated.  Refuses a keypoint outside its image."""
    if len(flat) % 2:
        raise ValueError(f"{what}: an even number of values expected")
    xy = np.array([int(v) for v in flat], dtype=np.int64).reshape(-1, 2)
    bad = (xy[:, 0] < 0) | (xy[:, 0] >= width) | (xy[:, 1] < 0) | (xy[:, 1] >= height)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"{what}: keypoint {i} at ({xy[i, 0]}, {xy[i, 1]}) lies outside its {width}x{height} image")
    return xy


def match_primitives(result, cam_shape, lidar_shape):
    """The primitives of the match picture, from the dictionary ``<bag>_matches.json`` holds and the two images' (H, W):
    a white ring of radius 3 at every camera keypoint; one at every LiDAR keypoint, mapped into the right panel as
    X = W + ((2 x + 1) W) // (2 W_l), Y = ((2 y + 1) H) // (2 H_l); then one line per matched camera keypoint, in ascending index, from
    the camera keypoint to its LiDAR keypoint's ring -- lines over rings, as in the reference.  Line colour: q = round(256 confidence),
    q_max the largest q among matched rows, ``TURBO[min(255, (256 q) // q_max)]`` (``TURBO[0]`` when q_max is 0).  No match: no line."""
    H, W = int(cam_shape[0]), int(cam_shape[1])
    Hl, Wl = int(lidar_shape[0]), int(lidar_shape[1])
    k0 = _keypoints(result["kpts0"], W, H, "kpts0")
    k1 = _keypoints(result["kpts1"], Wl, Hl, "kpts1")
    matches, confidence = result["matches"], result["confidence"]
    if len(matches) != k0.shape[0] or len(confidence) != k0.shape[0]:
        raise ValueError("matches / confidence: one entry per camera keypoint expected")
    k1[:, 0] = W + ((2 * k1[:, 0] + 1) * W) // (2 * Wl)
    k1[:, 1] = ((2 * k1[:, 1] + 1) * H) // (2 * Hl)
    prims = [ring(x, y, KEYPOINT_RADIUS, WHITE) for x, y in k0] + [ring(x, y, KEYPOINT_RADIUS, WHITE) for x, y in k1]
    rows = [i for i, m in enumerate(matches) if int(m) >= 0]
    if not rows:
        return prims
    q = {i: int(round(256.0 * float(confidence[i]))) for i in rows}
    q_max = max(q.values())
    for i in rows:
        m = int(matches[i])
        if m >= k1.shape[0]:
            raise ValueError(f"matches: row {i} names LiDAR keypoint {m} of {k1.shape[0]}")
        c = TURBO[min(255, max(0, (256 * q[i]) // q_max))] if q_max > 0 else TURBO[0]
        prims.append(line(k0[i, 0], k0[i, 1], k1[m, 0], k1[m, 1], c))
    return prims


def match_picture(camera, lidar, result, device=0):
    """The (H, 2 W, 3) RGB match picture of one bag: camera image left, LiDAR intensity image right (module docstring)."""
    cam, lid = np.asarray(camera), np.asarray(lidar)
    return draw(cam, lid, match_primitives(result, cam.shape, lid.shape), device=device)


def residual_primitives(proj, kpts_2d, points_3d, T_camera_lidar, error_thresh):
    """What ``initial_guess_auto --picture`` draws over one bag's camera image: for every correspondence, in order, a ring of radius 3
    at the camera keypoint, a line from the keypoint to the floor of its 3-D point's projection under ``T_camera_lidar`` (4x4) and a disc
    of radius 1 at that projection -- green where the float64 reprojection error is below ``error_thresh``, red otherwise.  A point
    behind the camera (z <= 0), a projection that is not finite or one outside the coordinate range of ``nidreg_draw`` gets the red
    ring only.  The projection is the host one ``pose.reprojection_terms`` uses.  Returns ``(prims, green, red)``."""
    kp = np.asarray(kpts_2d, dtype=np.float64).reshape(-1, 2)
    if kp.shape[0] == 0:
        return [], 0, 0
    p = np.asarray(points_3d, dtype=np.float64).reshape(kp.shape[0], -1)[:, :3]
    T = np.asarray(T_camera_lidar, dtype=np.float64)
    pc = p @ T[:3, :3].T + T[:3, 3]
    uv = proj.project(pc, device=-1)
    prims, green = [], 0
    for i in range(kp.shape[0]):
        x, y = int(kp[i, 0]), int(kp[i, 1])
        u, v = float(uv[i, 0]), float(uv[i, 1])
        ok = pc[i, 2] > 0.0 and math.isfinite(u) and math.isfinite(v)
        if ok:
            pu, pv = math.floor(u), math.floor(v)
            ok = COORD_MIN <= pu <= COORD_MAX and COORD_MIN <= pv <= COORD_MAX
        if not ok:
            prims.append(ring(x, y, KEYPOINT_RADIUS, RED))
            continue
        inlier = math.sqrt((u - kp[i, 0]) ** 2 + (v - kp[i, 1]) ** 2) < float(error_thresh)
        green += int(inlier)
        c = GREEN if inlier else RED
        prims += [ring(x, y, KEYPOINT_RADIUS, c), line(x, y, pu, pv, c), disc(pu, pv, 1, c)]
    return prims, green, kp.shape[0] - green
