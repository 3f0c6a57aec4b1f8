"""2D-2D matches between a camera image and a LiDAR intensity image on the GPU: ctypes wrappers of ``nidreg_features_detect`` /
``nidreg_features_match`` (csrc/nid_match_kernels.hpp) and the ``find_matches`` step built from them.

A classical, licence-free, deterministic STAND-IN for the reference's ``scripts/find_matches_superglue.py`` (SuperGlue needs
pretrained weights under a non-commercial licence, and OpenCV) -- not a port of it: FAST-9 corners over a 6/5 pyramid, upright
BRIEF-256, mutual-best Hamming matching with a ratio test, all in integer arithmetic.  Its quality on real camera / LiDAR pairs is
unmeasured; the defaults below were chosen on the synthetic scene of tests/test_find_matches_e2e.py (profiles/find_matches.json).
There is no CPU path here (tests/matching_oracle.py is the checker's restatement).
"""
import ctypes
import functools
from fractions import Fraction

import numpy as np

from . import _lib

CAPACITY = _lib.FEATURES_CAPACITY
NO_DISTANCE = 257  # best / second-best distance where there is no such column

# defaults of the command line (profiles/find_matches.json says what they were chosen on)
MAX_KEYPOINTS = 2048
NMS_RADIUS = 4
LEVELS = 8
FILL_PASSES = 2
FAST_THRESHOLD = 20
MAX_DISTANCE = 64
RATIO = 0.8


def _p(a, ctype):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctype))


def _rows_u8(a, what):
    """A 2-D uint8 array whose rows are contiguous (the row stride may exceed the width: a view into a wider array is passed as it is)."""
    a = np.asarray(a)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError(f"{what}: a 2-D uint8 array expected")
    if a.size and (a.strides[1] != 1 or a.strides[0] < a.shape[1]):
        a = np.ascontiguousarray(a)
    return a


def detect_features(image_u8, mask=None, levels=LEVELS, fast_threshold=FAST_THRESHOLD, nms_radius=NMS_RADIUS, fill_passes=FILL_PASSES, max_keypoints=MAX_KEYPOINTS, device=0):
    """``nidreg_features_detect``: ``(kpts (n, 4) int32: x0 y0 level score, desc (n, 8) uint32)`` in (score descending, level, y, x)
    order.  ``mask`` (H, W; non-zero or True = valid) marks the pixels that hold data: holes are filled before detection and no
    keypoint is reported on one.  ``max_keypoints`` -1 keeps all, capped at ``CAPACITY``."""
    img = _rows_u8(image_u8, "detect_features: image")
    H, W = img.shape
    m = None
    if mask is not None:
        m = np.asarray(mask)
        if m.shape != img.shape:
            raise ValueError("detect_features: the mask must have the image's shape")
        m = _rows_u8(m.astype(np.uint8) if m.dtype != np.uint8 else m, "detect_features: mask")
    cap = CAPACITY if int(max_keypoints) < 0 else max(int(max_keypoints), 1)
    kpts = np.zeros((cap, 4), dtype=np.int32)
    desc = np.zeros((cap, 8), dtype=np.uint32)
    count = ctypes.c_int32(0)
    rc = _lib.load().nidreg_features_detect(int(device), _p(img, ctypes.c_uint8), W, H, img.strides[0] if img.size else W, _p(m, ctypes.c_uint8), m.strides[0] if m is not None else 0,
                                            int(levels), int(fast_threshold), int(nms_radius), int(fill_passes), int(max_keypoints), _p(kpts, ctypes.c_int32), _p(desc, ctypes.c_uint32),
                                            ctypes.byref(count))
    _lib.check(rc, "nidreg_features_detect")
    n = int(count.value)
    return kpts[:n].copy(), desc[:n].copy()


def ratio_fraction(ratio):
    """``--ratio`` as the integer fraction the kernel compares with: d1 * den < d2 * num (at most three decimals are kept)."""
    f = Fraction(int(round(float(ratio) * 1000)), 1000)
    return f.numerator, f.denominator


def match_features(desc0, desc1, max_distance=MAX_DISTANCE, ratio_num=None, ratio_den=None, device=0):
    """``nidreg_features_match``: ``(match01 (n0,) int32: index into desc1 or -1, best distance (n0,), second-best distance (n0,))``.
    Accepted: mutual best, best <= ``max_distance`` and best * ratio_den < second * ratio_num (default ``RATIO``)."""
    if ratio_num is None or ratio_den is None:
        ratio_num, ratio_den = ratio_fraction(RATIO)
    d0 = np.ascontiguousarray(desc0, dtype=np.uint32).reshape(-1, 8)
    d1 = np.ascontiguousarray(desc1, dtype=np.uint32).reshape(-1, 8)
    n0, n1 = d0.shape[0], d1.shape[0]
    m = np.full(n0, -1, dtype=np.int32)
    best = np.full(n0, NO_DISTANCE, dtype=np.int32)
    second = np.full(n0, NO_DISTANCE, dtype=np.int32)
    rc = _lib.load().nidreg_features_match(int(device), _p(d0, ctypes.c_uint32), n0, _p(d1, ctypes.c_uint32), n1, int(max_distance), int(ratio_num), int(ratio_den), _p(m, ctypes.c_int32),
                                           _p(best, ctypes.c_int32), _p(second, ctypes.c_int32))
    _lib.check(rc, "nidreg_features_match")
    return m, best, second


def rotate_cw(image, angle):
    """The image turned clockwise by 0 / 90 / 180 / 270 degrees (``cv2.rotate``'s three codes)."""
    if angle not in (0, 90, 180, 270):
        raise ValueError("rotation must be 0, 90, 180 or 270")
    return np.ascontiguousarray(np.rot90(np.asarray(image), k=-(angle // 90)))


def unrotate_points(xy, angle, width, height):
    """Pixels (n, 2) of the image turned clockwise by ``angle`` back to pixels of the ORIGINAL ``width`` x ``height`` image, exactly:
    90: (y_r, H - 1 - x_r); 180: (W - 1 - x_r, H - 1 - y_r); 270: (W - 1 - y_r, x_r).  (The reference script subtracts from W and H,
    not W - 1 and H - 1: one pixel off.  Deliberately not reproduced.)"""
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    xr, yr = xy[:, 0], xy[:, 1]
    if angle == 0:
        out = (xr, yr)
    elif angle == 90:
        out = (yr, height - 1 - xr)
    elif angle == 180:
        out = (width - 1 - xr, height - 1 - yr)
    elif angle == 270:
        out = (width - 1 - yr, xr)
    else:
        raise ValueError("rotation must be 0, 90, 180 or 270")
    return np.stack(out, axis=1)


def find_matches(camera_u8, lidar_u8, lidar_valid_mask=None, max_keypoints=MAX_KEYPOINTS, nms_radius=NMS_RADIUS, fast_threshold=FAST_THRESHOLD, max_distance=MAX_DISTANCE, ratio=RATIO,
                 levels=LEVELS, fill_passes=FILL_PASSES, rotate_camera=0, rotate_lidar=0, device=0, detect=None, match=None, camera_valid_mask=None):
    """Keypoints of both images and the accepted matches, as the dictionary ``<bag>_matches.json`` holds: ``kpts0`` / ``kpts1`` flat
    integer x, y lists (pixels of the UNROTATED images), ``matches`` one entry per camera keypoint (index into kpts1 or -1),
    ``confidence`` 1 - d / 256 for a matched row and 0 otherwise.  ``detect`` / ``match`` replace the device calls by functions of the same
    signature without ``device`` (the checker runs the whole step on its numpy restatement).  ``camera_valid_mask`` (H, W; non-zero or
    True = valid; the camera image's shape) keeps camera keypoints off its zero pixels: it is used as given, with no margin, turned
    with ``rotate_camera``, and nothing is filled on the camera side (``fill_passes=0``: a masked region of a photograph holds pixels
    that are unwanted, not missing)."""
    detect = detect or functools.partial(detect_features, device=device)
    match = match or functools.partial(match_features, device=device)
    cam = np.asarray(camera_u8)
    lid = np.asarray(lidar_u8)
    mask = None if lidar_valid_mask is None else np.asarray(lidar_valid_mask) != 0
    if camera_valid_mask is None:
        k0, d0 = detect(rotate_cw(cam, rotate_camera), None, levels=levels, fast_threshold=fast_threshold, nms_radius=nms_radius, fill_passes=fill_passes, max_keypoints=max_keypoints)
    else:
        cam_mask = np.asarray(camera_valid_mask) != 0
        if cam_mask.shape != cam.shape:
            raise ValueError("find_matches: camera_valid_mask must have the camera image's shape")
        k0, d0 = detect(rotate_cw(cam, rotate_camera), rotate_cw(cam_mask, rotate_camera), levels=levels, fast_threshold=fast_threshold, nms_radius=nms_radius, fill_passes=0,
                        max_keypoints=max_keypoints)
    k1, d1 = detect(rotate_cw(lid, rotate_lidar), None if mask is None else rotate_cw(mask, rotate_lidar), levels=levels, fast_threshold=fast_threshold, nms_radius=nms_radius,
                    fill_passes=fill_passes, max_keypoints=max_keypoints)
    num, den = ratio_fraction(ratio)
    m, best, _ = match(d0, d1, max_distance=max_distance, ratio_num=num, ratio_den=den)
    xy0 = unrotate_points(k0[:, :2], rotate_camera, cam.shape[1], cam.shape[0])
    xy1 = unrotate_points(k1[:, :2], rotate_lidar, lid.shape[1], lid.shape[0])
    conf = np.where(m >= 0, 1.0 - best.astype(np.float64) / 256.0, 0.0)
    return {"kpts0": xy0.reshape(-1).tolist(), "kpts1": xy1.reshape(-1).tolist(), "matches": [int(v) for v in m], "confidence": [float(v) for v in conf]}
