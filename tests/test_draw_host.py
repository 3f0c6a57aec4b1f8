"""CPU tests of the match pictures (draw.py, the argument checks of nidreg_draw, the two command lines' new options) and of the
checker's own restatement (tests/draw_oracle.py) against pixel sets listed by hand.  No GPU: nidreg_draw refuses bad arguments
before it touches a device, and the primitive lists are host code."""
import ctypes
import json
import os

import numpy as np
import pytest

import draw_oracle as do
from direct_visual_lidar_calibration_amd import _lib, dataset, draw, find_matches, initial_guess_auto, nid


# ------------------------------------------------------------------------------------------ the oracle, by hand
def test_oracle_lines_equal_hand_listed_pixel_sets():
    # n = 5: y = (4 k + 5) // 10 -> 0 0 1 1 2 2
    assert do.pixel_set(draw.line(0, 0, 5, 2, 0)) == {(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)}
    # from the other end: y = 2 - (4 k + 5) // 10 -> 2 2 1 1 0 0 at x = 5 4 3 2 1 0
    assert do.pixel_set(draw.line(5, 2, 0, 0, 0)) == {(5, 2), (4, 2), (3, 1), (2, 1), (1, 0), (0, 0)}
    # defined FROM the first point: n = 2, k = 1 -> (2 + 2) // 4 = 1 step in y away from whichever end it starts at
    assert do.pixel_set(draw.line(0, 0, 2, 1, 0)) == {(0, 0), (1, 1), (2, 1)}
    assert do.pixel_set(draw.line(2, 1, 0, 0, 0)) == {(2, 1), (1, 0), (0, 0)}
    assert do.pixel_set(draw.line(-3, 4, -3, 4, 0)) == {(-3, 4)}
    assert do.pixel_set(draw.line(1, 1, -2, -2, 0)) == {(1, 1), (0, 0), (-1, -1), (-2, -2)}
    # the 361 lines from the origin to |dx|, |dy| <= 9: 112 cover other pixels when their ends are swapped
    swapped = sum(do.pixel_set(draw.line(0, 0, dx, dy, 0)) != do.pixel_set(draw.line(dx, dy, 0, 0, 0)) for dx in range(-9, 10) for dy in range(-9, 10))
    assert swapped == 112


def test_oracle_rings_and_discs_equal_hand_listed_pixel_sets():
    assert do.pixel_set(draw.ring(7, -2, 0, 0)) == {(7, -2)} == do.pixel_set(draw.disc(7, -2, 0, 0))
    # radius 3: 25 <= 4 d2 < 49, d2 in {8, 9, 10} (7, 11 and 12 are no sums of two squares)
    r3 = {(2, 2), (2, -2), (-2, 2), (-2, -2), (3, 0), (-3, 0), (0, 3), (0, -3), (1, 3), (1, -3), (-1, 3), (-1, -3), (3, 1), (3, -1), (-3, 1), (-3, -1)}
    assert do.pixel_set(draw.ring(10, 20, 3, 0)) == {(10 + x, 20 + y) for x, y in r3}
    assert [len(do.pixel_set(draw.ring(0, 0, r, 0))) for r in range(4)] == [1, 8, 12, 16]
    # disc of radius 1: 4 d2 < 9, the 3 x 3 square
    assert do.pixel_set(draw.disc(0, 0, 1, 0)) == {(x, y) for x in (-1, 0, 1) for y in (-1, 0, 1)}
    for a in range(17):  # a disc is its ring and everything inside it
        assert do.pixel_set(draw.ring(0, 0, a, 0)) <= do.pixel_set(draw.disc(0, 0, a, 0))
        assert do.pixel_set(draw.disc(0, 0, a, 0)) == set().union(*(do.pixel_set(draw.ring(0, 0, r, 0)) for r in range(a + 1)))


def test_oracle_resize_identity_constant_and_range():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (7, 13), dtype=np.uint8)
    assert np.array_equal(do.resize(a, 13, 7), a)  # equal sizes: the identity
    for w, h in ((1, 1), (29, 5), (3, 40), (26, 14)):
        assert (do.resize(np.full((7, 13), 201, dtype=np.uint8), w, h) == 201).all()
        r = do.resize(a, w, h)
        assert r.shape == (h, w) and a.min() <= r.min() and r.max() <= a.max()
    # 2 x 1 -> 4 x 1 by hand: centres at 1/4, 3/4, 5/4, 7/4 source pixels minus 1/2: taps (0, 0), (0, 1) f 2/8, (0, 1) f 6/8, (1, 1)
    assert do.resize(np.array([[0, 80]], dtype=np.uint8), 4, 1).tolist() == [[0, 20, 60, 80]]
    # painter's order and per-pixel clipping on a 3 x 2 canvas
    pic = do.draw(np.zeros((2, 3), dtype=np.uint8), None, [draw.line(-5, 0, 5, 0, 0x010203), draw.disc(2, 1, 0, 0x0A0B0C), draw.line(2, -3, 2, 3, (9, 8, 7))])
    assert pic.tolist() == [[[1, 2, 3], [1, 2, 3], [9, 8, 7]], [[0, 0, 0], [0, 0, 0], [9, 8, 7]]]


# ------------------------------------------------------------------------------------------ draw.py
def test_turbo_equals_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    cmap = matplotlib.colormaps["turbo"]
    ref = np.array([[int(255 * c) for c in cmap(i)[:3]] for i in range(256)])
    assert draw.TURBO.shape == (256, 3) and draw.TURBO.dtype == np.uint8 and np.array_equal(draw.TURBO, ref)


def test_turbo_literal_is_a_colour_table():
    """(without matplotlib) the committed literal: 256 rows, dark blue to dark red through green"""
    assert draw.TURBO.shape == (256, 3) and draw.TURBO.dtype == np.uint8
    assert tuple(draw.TURBO[0]) == (48, 18, 59) and tuple(draw.TURBO[255]) == (122, 4, 2) and draw.TURBO[128, 1] > 250


def _colour(prim):
    return ((prim[5] >> 16) & 255, (prim[5] >> 8) & 255, prim[5] & 255)


def test_match_primitives_order_mapping_and_colour_index():
    cam_shape = (64, 96)
    result = {"kpts0": [10, 5, 95, 63, 0, 0, 40, 30], "kpts1": [10, 5, 47, 31, 0, 0], "matches": [1, -1, 0, 2], "confidence": [0.75, 0.0, 1.0, 1.0]}
    # a LiDAR image SMALLER than the camera's: 48 x 32.  X = 96 + ((2 x + 1) 96) // 96, Y = ((2 y + 1) 64) // 64
    prims = draw.match_primitives(result, cam_shape, (32, 48))
    white = draw.WHITE
    assert prims[:4] == [[draw.RING, 10, 5, 3, 0, white, 0, 0], [draw.RING, 95, 63, 3, 0, white, 0, 0], [draw.RING, 0, 0, 3, 0, white, 0, 0], [draw.RING, 40, 30, 3, 0, white, 0, 0]]
    assert prims[4:7] == [[draw.RING, 96 + 21, 11, 3, 0, white, 0, 0], [draw.RING, 96 + 95, 63, 3, 0, white, 0, 0], [draw.RING, 96 + 1, 1, 3, 0, white, 0, 0]]
    # lines after every ring, ascending camera keypoint; q = 192, 256, 256, q_max = 256 attained twice
    assert [p[:5] for p in prims[7:]] == [[draw.LINE, 10, 5, 96 + 95, 63], [draw.LINE, 0, 0, 96 + 21, 11], [draw.LINE, 40, 30, 96 + 1, 1]]
    assert [_colour(p) for p in prims[7:]] == [tuple(draw.TURBO[192]), tuple(draw.TURBO[255]), tuple(draw.TURBO[255])]
    # ... and LARGER: 200 x 128.  x = 199 -> (399 * 96) // 400 = 95, y = 127 -> (255 * 64) // 256 = 63; x = 0 -> 96 // 400 = 0
    big = dict(result, kpts1=[199, 127, 0, 0, 100, 64])
    prims = draw.match_primitives(big, cam_shape, (128, 200))
    assert [p[1:3] for p in prims[4:7]] == [[96 + 95, 63], [96 + 0, 0], [96 + (201 * 96) // 400, (129 * 64) // 256]]
    # a single match: it is its own q_max, (256 q) // q = 256 -> 255 whatever its confidence
    one = {"kpts0": [1, 2, 3, 4], "kpts1": [5, 6], "matches": [-1, 0], "confidence": [0.0, 0.5]}
    prims = draw.match_primitives(one, cam_shape, (64, 96))
    assert len(prims) == 4 and prims[3] == draw.line(3, 4, 96 + 5, 6, tuple(draw.TURBO[255]))
    # no match: rings only; no keypoints at all: nothing
    none = dict(one, matches=[-1, -1], confidence=[0.0, 0.0])
    assert [p[0] for p in draw.match_primitives(none, cam_shape, (64, 96))] == [draw.RING] * 3
    assert draw.match_primitives({"kpts0": [], "kpts1": [], "matches": [], "confidence": []}, cam_shape, (64, 96)) == []
    # a distinct confidence per line: q = 128 of q_max = 192 -> (256 * 128) // 192 = 170
    two = {"kpts0": [1, 2, 3, 4], "kpts1": [5, 6], "matches": [0, 0], "confidence": [0.5, 0.75]}
    assert [_colour(p) for p in draw.match_primitives(two, cam_shape, (64, 96))[3:]] == [tuple(draw.TURBO[170]), tuple(draw.TURBO[255])]


def test_match_primitives_truncates_float_keypoints_and_refuses_one_outside_its_image():
    """the reference script's file holds float pixels"""
    ok = {"kpts0": [10.9, 5.2, 95.99, 63.5], "kpts1": [47.9, 31.9], "matches": [0, -1], "confidence": [0.9, 0.0]}
    prims = draw.match_primitives(ok, (64, 96), (32, 48))
    assert [p[1:3] for p in prims[:2]] == [[10, 5], [95, 63]] and prims[3][:5] == [draw.LINE, 10, 5, 96 + 95, 63]
    with pytest.raises(ValueError, match=r"kpts0: keypoint 1 at \(96, 63\) lies outside its 96x64 image"):
        draw.match_primitives(dict(ok, kpts0=[10.9, 5.2, 96.0, 63.5]), (64, 96), (32, 48))
    with pytest.raises(ValueError, match=r"kpts1: keypoint 0 at \(47, 32\) lies outside its 48x32 image"):
        draw.match_primitives(dict(ok, kpts1=[47.9, 32.0]), (64, 96), (32, 48))
    with pytest.raises(ValueError, match=r"kpts0: keypoint 0 at \(-1, 5\)"):
        draw.match_primitives(dict(ok, kpts0=[-1.5, 5.2, 3, 4]), (64, 96), (32, 48))
    with pytest.raises(ValueError, match="names LiDAR keypoint 1 of 1"):
        draw.match_primitives(dict(ok, matches=[1, -1]), (64, 96), (32, 48))


def test_residual_primitives_on_an_exact_pinhole_case():
    """fx = fy = 100, cx = 50, cy = 40, no distortion, identity pose: (x, y, 1) projects to (100 x + 50, 100 y + 40) exactly"""
    proj = nid.create_camera("plumb_bob", [100.0, 100.0, 50.0, 40.0], [])
    kpts = np.array([[52.0, 41.0], [10.0, 10.0], [30.0, 20.0], [5.0, 6.0], [60.0, 60.0]])
    points = np.array([[0.0, 0.0, 1.0, 1.0],      # -> (50, 40): sqrt(5) px from its keypoint, an inlier
                       [0.25, 0.125, 1.0, 1.0],   # -> (75, 52.5): 78 px, an outlier
                       [0.0, 0.0, -1.0, 1.0],     # behind the camera
                       [1000.0, 0.0, 1.0, 1.0],   # -> u = 100050: outside the coordinate range
                       [0.125, 0.255, 1.0, 1.0]])  # -> (62.5, 65.5): floor (62, 65); sqrt(2.5^2 + 5.5^2) = 6.04 px
    prims, green, red = draw.residual_primitives(proj, kpts, points, np.eye(4), 10.0)
    g, r = draw.GREEN, draw.RED
    assert (g, r) == (0x00FF00, 0xFF0000)
    assert prims == [
        draw.ring(52, 41, 3, g), draw.line(52, 41, 50, 40, g), draw.disc(50, 40, 1, g),
        draw.ring(10, 10, 3, r), draw.line(10, 10, 75, 52, r), draw.disc(75, 52, 1, r),
        draw.ring(30, 20, 3, r),
        draw.ring(5, 6, 3, r),
        draw.ring(60, 60, 3, g), draw.line(60, 60, 62, 65, g), draw.disc(62, 65, 1, g),
    ]
    assert (green, red) == (2, 3)
    # the threshold is strict and the error the float64 one: 6.04 px is red at a threshold of 6
    _, green, red = draw.residual_primitives(proj, kpts, points, np.eye(4), 6.0)
    assert (green, red) == (1, 4)
    # the pose enters: a shift of the LiDAR frame by -1/32 in x moves every projection 3.125 px to the left
    T = np.eye(4)
    T[0, 3] = -0.03125
    prims, _, _ = draw.residual_primitives(proj, kpts[:1], points[:1], T, 10.0)
    assert prims[1] == draw.line(52, 41, 46, 40, g)
    assert draw.residual_primitives(proj, np.zeros((0, 2)), np.zeros((0, 4)), np.eye(4), 10.0) == ([], 0, 0)


# ------------------------------------------------------------------------------------------ the ABI's refusals
def _call(left, lw, lh, ls, right, rw, rh, rs, n, prims, out):
    u8 = ctypes.POINTER(ctypes.c_uint8)
    return _lib.load().nidreg_draw(0, None if left is None else left.ctypes.data_as(u8), lw, lh, ls, None if right is None else right.ctypes.data_as(u8), rw, rh, rs, n,
                                   None if prims is None else prims.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None if out is None else out.ctypes.data_as(u8))


def test_every_invalid_argument_is_refused_with_its_message_and_nothing_written():
    img = np.zeros((7, 13), dtype=np.uint8)
    out = np.full((7, 26, 3), 0xAB, dtype=np.uint8)
    one = np.array([draw.ring(1, 1, 3, 0x123456)], dtype=np.int32)

    def refused(message, left=img, lw=13, lh=7, ls=13, right=None, rw=0, rh=0, rs=0, n=1, prims=one, o=out):
        assert _call(left, lw, lh, ls, right, rw, rh, rs, n, prims, o) == _lib.NIDREG_ERR_INVALID
        assert message in _lib.last_error(), _lib.last_error()
        assert (out == 0xAB).all()

    refused("nidreg_draw: null left_gray or out_rgb", left=None)
    refused("nidreg_draw: null left_gray or out_rgb", o=None)
    refused("nidreg_draw: null prims with num_prims > 0", prims=None)
    for lw, lh in ((0, 7), (13, 0), (-1, 7), (16385, 7), (13, 16385)):
        refused("nidreg_draw: width and height must lie in [1, 16384]", lw=lw, lh=lh, ls=max(lw, 13))
    for rw, rh in ((0, 7), (13, 0), (16385, 7), (13, 16385)):
        refused("nidreg_draw: width and height must lie in [1, 16384]", right=img, rw=rw, rh=rh, rs=max(rw, 13))
    refused("nidreg_draw: a row stride below the width", ls=12)
    refused("nidreg_draw: a row stride below the width", right=img, rw=13, rh=7, rs=12)
    refused("nidreg_draw: num_prims must lie in [0, 16777216]", n=-1)
    refused("nidreg_draw: num_prims must lie in [0, 16777216]", n=(1 << 24) + 1)

    def bad(record, message):
        recs = np.array([draw.disc(0, 0, 0, 0), record], dtype=np.int32)
        refused("nidreg_draw: primitive 1: " + message, n=2, prims=recs)

    bad([3, 0, 0, 0, 0, 0, 0, 0], "unknown kind 3")
    bad([-1, 0, 0, 0, 0, 0, 0, 0], "unknown kind -1")
    for rec in ([0, 32768, 0, 0, 0, 0, 0, 0], [0, 0, -32769, 0, 0, 0, 0, 0], [0, 0, 0, 32768, 0, 0, 0, 0], [0, 0, 0, 0, -32769, 0, 0, 0], [1, -32769, 0, 3, 0, 0, 0, 0],
                [2, 0, 32768, 3, 0, 0, 0, 0]):
        bad(rec, "a coordinate outside [-32768, 32767]")
    for kind in (draw.RING, draw.DISC):
        bad([kind, 0, 0, 17, 0, 0, 0, 0], "radius must lie in [0, 16]")
        bad([kind, 0, 0, -1, 0, 0, 0, 0], "radius must lie in [0, 16]")
    bad([0, 0, 0, 0, 0, 0x1000000, 0, 0], "rgb above 0xFFFFFF")
    bad([2, 0, 0, 0, 0, -1, 0, 0], "rgb above 0xFFFFFF")
    # the Python wrapper raises with the library's text
    with pytest.raises(RuntimeError, match=r"nidreg_draw failed \(-1\): nidreg_draw: primitive 0: radius must lie in \[0, 16\]"):
        draw.draw(img, None, [draw.ring(0, 0, 17, 0)])
    with pytest.raises(ValueError, match="records of 8 integers"):
        draw.draw(img, None, [[0, 1, 2]])
    with pytest.raises(ValueError, match="2-D uint8 array expected"):
        draw.draw(img.astype(np.float64), None, [])
    # what is valid passes every check and gets as far as the device
    if _lib.load().nidreg_device_count() == 0:
        edge = np.array([draw.line(-32768, -32768, 32767, 32767, 0xFFFFFF), draw.ring(32767, -32768, 16, 0), draw.disc(0, 0, 0, 0)], dtype=np.int32)
        assert _call(img, 13, 7, 13, img, 13, 7, 13, 3, edge, out) < 0 and "no HIP device" in _lib.last_error()


# ------------------------------------------------------------------------------------------ command lines
def test_parsers_know_the_picture_options():
    p = find_matches.build_parser()
    a = p.parse_args(["d"])
    assert a.picture is False and a.picture_only is False
    assert p.parse_args(["d", "--picture"]).picture is True and p.parse_args(["d", "--picture"]).picture_only is False
    assert p.parse_args(["d", "--picture_only"]).picture_only is True
    with pytest.raises(SystemExit):
        p.parse_args(["d", "--picture", "--picture_only"])
    q = initial_guess_auto.build_parser()
    assert q.parse_args(["d"]).picture is False and q.parse_args(["d", "--picture", "--seed", "2"]).picture is True


def test_picture_only_refuses_a_keypoint_outside_its_image(tmp_path):
    d = str(tmp_path / "data")
    os.makedirs(d)
    dataset.write_png_gray(os.path.join(d, "bag0.png"), np.zeros((64, 96), dtype=np.uint8))
    dataset.write_png_gray(os.path.join(d, "bag0_lidar_intensities.png"), np.zeros((32, 48), dtype=np.uint8))
    dataset.write_calib(d, {"meta": {"bag_names": ["bag0"]}})
    with pytest.raises(FileNotFoundError, match=r"error: failed to open .*bag0_matches\.json"):
        find_matches.main([d, "--picture_only"])
    with open(os.path.join(d, "bag0_matches.json"), "w") as f:
        json.dump({"keypoints0": [], "kpts0": [10.5, 5.0, 20.0, 64.2], "kpts1": [1.0, 1.0], "matches": [0, -1], "confidence": [0.9, 0.0]}, f)
    with pytest.raises(ValueError, match=r"bag0_matches\.json: kpts0: keypoint 1 at \(20, 64\) lies outside its 96x64 image"):
        find_matches.main([d, "--picture_only"])
    assert sorted(os.listdir(d)) == ["bag0.png", "bag0_lidar_intensities.png", "bag0_matches.json", "calib.json"]  # no picture, nothing else
