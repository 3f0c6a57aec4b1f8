"""Host-side tests of find_matches (no GPU): the BRIEF table generator against the committed header, the numpy restatement
(tests/matching_oracle.py) on hand-made images, the matches file through pose.read_correspondences, the rotation undo, and the
argument refusals of the C ABI, which come before any device call."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest

import matching_oracle as mo
from direct_visual_lidar_calibration_amd import _lib, dataset, matching, pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location("gen_brief_table", os.path.join(ROOT, "tools", "gen_brief_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_table_generator_reproduces_the_committed_header_byte_for_byte():
    gen = _generator()
    with open(os.path.join(_lib.CSRC_DIR, "nid_brief_table.hpp"), "rb") as f:
        committed = f.read()
    assert gen.header().encode() == committed
    pairs = np.array(gen.pairs())
    assert pairs.shape == (256, 4) and pairs.min() >= -15 and pairs.max() <= 15
    assert not (pairs[:, :2] == pairs[:, 2:]).all(axis=1).any()
    assert np.array_equal(pairs, mo.brief_pairs())  # the restatement draws the same table with its own generator
    assert pairs.min() == -15 and pairs.max() == 15  # the whole reach is in use


def test_single_bright_pixel_is_a_corner_of_its_contrast_and_the_only_one():
    """One bright pixel on black: at the pixel itself all 16 circle pixels are darker by 200, so it IS a (dark-arc) corner of score
    200; a pixel 3 away has one bright circle pixel only: no arc of 9."""
    img = np.zeros((41, 41), dtype=np.uint8)
    img[20, 20] = 200
    s = mo.fast_scores(img)
    assert s[20, 20] == 200 and (s > 0).sum() == 1
    k, d = mo.detect(img, fast_threshold=20, levels=1)
    assert k.tolist() == [[20, 20, 0, 200]] and d.shape == (1, 8)
    assert mo.detect(img, fast_threshold=201, levels=1)[0].shape == (0, 4)


def test_step_corner_scores_its_contrast_and_a_straight_edge_scores_nothing():
    img = np.full((48, 48), 50, dtype=np.uint8)
    img[24:, 24:] = 150  # a bright quadrant: its tip (24, 24) sees 11 darker circle pixels
    s = mo.fast_scores(img)
    assert s[24, 24] == 100
    edge = np.full((48, 48), 50, dtype=np.uint8)
    edge[:, 24:] = 150
    assert mo.fast_scores(edge).max() == 0  # next to a straight edge 7 circle pixels lie across it: never 9 contiguous
    k, _ = mo.detect(img, fast_threshold=20, nms_radius=4, levels=1)
    assert [24, 24, 0, 100] in k.tolist()


def test_flat_image_has_no_keypoint_and_a_small_one_no_level():
    assert mo.detect(np.full((64, 80), 7, dtype=np.uint8))[0].shape == (0, 4)
    assert mo.detect(np.random.default_rng(0).integers(0, 255, (32, 200)).astype(np.uint8))[0].shape == (0, 4)


def test_plateau_of_equal_scores_keeps_the_first_in_row_major_order():
    score = np.zeros((40, 40), dtype=np.int64)
    score[20, 18:23] = 60  # five equal scores inside one window
    score[30, 5] = 60
    keep = mo.nms(score, 4, 20)
    assert np.argwhere(keep).tolist() == [[20, 18], [30, 5]]
    score[19, 22] = 60  # an equal score on an earlier row suppresses (20, 18) too: it is within the radius of it
    assert np.argwhere(mo.nms(score, 4, 20)).tolist() == [[19, 22], [30, 5]]
    assert np.argwhere(mo.nms(score, 0, 20)).shape[0] == 7  # radius 0: every pixel at or above the threshold


def test_pyramid_smoothing_and_fill_by_hand():
    src = np.arange(36, dtype=np.uint8).reshape(6, 6) * 7
    dst = mo.pyr_down(src)
    assert dst.shape == (5, 5)
    # destination (0, 0) sits at source (0.1, 0.1): (81 a + 9 b + 9 c + d + 50) // 100
    assert dst[0, 0] == (81 * int(src[0, 0]) + 9 * int(src[0, 1]) + 9 * int(src[1, 0]) + int(src[1, 1]) + 50) // 100
    # destination 4 sits at source 4.9: taps 4 and 5, weights 1 and 9
    assert dst[4, 4] == (1 * (1 * int(src[4, 4]) + 9 * int(src[4, 5])) + 9 * (1 * int(src[5, 4]) + 9 * int(src[5, 5])) + 50) // 100
    assert (mo.smooth(np.full((9, 11), 93, dtype=np.uint8)) == 93).all()
    one = np.zeros((9, 9), dtype=np.uint8)
    one[4, 4] = 255
    assert mo.smooth(one)[4, 4] == (36 * 255 + 128) >> 8 and mo.smooth(one)[2, 2] == (255 + 128) >> 8
    img = np.array([[10, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 21]], dtype=np.uint8)
    mask = np.array([[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]], dtype=np.uint8)
    f1, v1 = mo.fill_holes(img, mask, 1)
    assert f1[0, 1] == 10 and f1[1, 1] == 10 and f1[1, 2] == 21 and not v1[0, 2] and not v1[0, 3] and f1[0, 3] == 0
    f2, v2 = mo.fill_holes(img, mask, 2)
    assert v2.all() and f2[0, 2] == (10 + 10 + 21 + 21 + 2) // 4  # its valid neighbours after pass 1: (0,1)=10, (1,1)=10, (1,2)=21, (1,3)=21
    assert f2[0, 3] == 21


def test_matches_file_round_trips_through_read_correspondences(tmp_path):
    rng = np.random.default_rng(3)
    n = 400
    points = np.concatenate([rng.normal(size=(n, 3)), np.ones((n, 1))], axis=1)
    idx = np.full((40, 50), -1, dtype=np.int32)
    idx.reshape(-1)[rng.choice(2000, size=n, replace=False)] = np.arange(n)
    cam = rng.integers(0, 255, (60, 70)).astype(np.uint8)
    d = str(tmp_path / "data")
    dataset.write_preprocessed(d, ("plumb_bob", [50.0, 50.0, 35.0, 30.0], [0.0] * 5), [("bag0", cam, points, rng.random(n))], lidar_images={"bag0": (np.zeros(idx.shape), idx)})
    k0 = np.stack([rng.integers(0, 70, 30), rng.integers(0, 60, 30), np.zeros(30, int), np.full(30, 50)], axis=1).astype(np.int32)
    ys, xs = np.nonzero(idx >= 0)
    pick = rng.choice(len(ys), size=25, replace=False)
    k1 = np.stack([xs[pick], ys[pick], np.zeros(25, int), np.full(25, 50)], axis=1).astype(np.int32)
    m = np.full(30, -1, dtype=np.int32)
    m[:20] = rng.permutation(25)[:20]
    best = np.where(m >= 0, 32, 100).astype(np.int32)
    result = matching.find_matches(cam, np.zeros(idx.shape, np.uint8), idx >= 0, detect=lambda img, mask, **kw: (k0, None) if mask is None else (k1, None),
                                   match=lambda d0, d1, **kw: (m, best, best))
    assert all(isinstance(v, int) for v in result["kpts0"] + result["kpts1"] + result["matches"])
    assert result["confidence"][:20] == [1.0 - 32 / 256.0] * 20 and result["confidence"][20:] == [0.0] * 10
    with open(os.path.join(d, "bag0_matches.json"), "w") as f:
        json.dump(result, f)
    kp, pts = pose.read_correspondences(d, "bag0", points)
    assert np.array_equal(kp, k0[:20, :2].astype(np.float64))
    assert np.array_equal(pts, points[idx[k1[m[:20], 1], k1[m[:20], 0]]])


@pytest.mark.parametrize("angle", [0, 90, 180, 270])
def test_rotation_is_undone_exactly_on_a_non_square_image(angle):
    H, W = 5, 8
    img = np.arange(H * W).reshape(H, W)
    rot = matching.rotate_cw(img, angle)
    assert rot.shape == ((H, W) if angle in (0, 180) else (W, H))
    if angle == 90:
        assert rot[0, 0] == img[H - 1, 0] and rot[0, H - 1] == img[0, 0]  # clockwise: the left column becomes the top row
    ys, xs = np.mgrid[0:rot.shape[0], 0:rot.shape[1]]
    back = matching.unrotate_points(np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1), angle, W, H)
    assert back[:, 0].min() == 0 and back[:, 0].max() == W - 1 and back[:, 1].min() == 0 and back[:, 1].max() == H - 1
    assert np.array_equal(img[back[:, 1], back[:, 0]], rot.reshape(-1))


def test_abi_refuses_bad_arguments_before_any_device_call():
    lib = _lib.load()
    img = np.zeros((40, 48), dtype=np.uint8)
    kp, de, cnt = np.zeros((16, 4), np.int32), np.zeros((16, 8), np.uint32), ctypes.c_int32(-7)
    u8, u32, i32 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)
    P = lambda a, t: a.ctypes.data_as(t)  # noqa: E731

    def detect(image=img, w=48, h=40, stride=48, mask=None, mstride=0, levels=8, thr=20, r=4, fill=2, maxk=16, kpts=kp, desc=de, count=cnt):
        return lib.nidreg_features_detect(0, None if image is None else P(image, u8), w, h, stride, None if mask is None else P(mask, u8), mstride, levels, thr, r, fill, maxk,
                                          None if kpts is None else P(kpts, i32), None if desc is None else P(desc, u32), None if count is None else ctypes.byref(count))

    bad = [dict(image=None), dict(kpts=None), dict(desc=None), dict(count=None), dict(w=0), dict(h=-1), dict(w=40000), dict(stride=47), dict(mask=img, mstride=47), dict(levels=0),
           dict(levels=17), dict(thr=0), dict(thr=256), dict(r=-1), dict(r=17), dict(fill=-1), dict(maxk=0), dict(maxk=-2), dict(maxk=_lib.FEATURES_CAPACITY + 1)]
    for kw in bad:
        assert detect(**kw) == _lib.NIDREG_ERR_INVALID, kw
        assert "nidreg_features_detect" in _lib.last_error()
    # an image too small for one level is valid: no keypoint, no device call (this machine has none)
    small = np.zeros((32, 64), dtype=np.uint8)
    assert detect(image=small, w=64, h=32, stride=64) == _lib.NIDREG_OK and cnt.value == 0

    d0, d1 = np.zeros((3, 8), np.uint32), np.zeros((2, 8), np.uint32)
    m, b, s = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32)

    def match(a=d0, n0=3, c=d1, n1=2, maxd=64, num=8, den=10, mm=m, bb=b, ss=s):
        return lib.nidreg_features_match(0, None if a is None else P(a, u32), n0, None if c is None else P(c, u32), n1, maxd, num, den, None if mm is None else P(mm, i32),
                                         None if bb is None else P(bb, i32), None if ss is None else P(ss, i32))

    for kw in [dict(a=None), dict(c=None), dict(mm=None), dict(bb=None), dict(n0=-1), dict(n1=-1), dict(den=0), dict(den=-3), dict(num=-1), dict(maxd=-1)]:
        assert match(**kw) == _lib.NIDREG_ERR_INVALID, kw
        assert "nidreg_features_match" in _lib.last_error()
    # an empty side is valid and needs no device: no match, distances at the sentinel
    assert match(n1=0, c=None) == _lib.NIDREG_OK and m.tolist() == [-1] * 3 and b.tolist() == [257] * 3 and s.tolist() == [257] * 3
    assert match(n0=0, a=None, mm=None, bb=None, ss=None) == _lib.NIDREG_OK
    assert match(n1=0, c=None, ss=None) == _lib.NIDREG_OK
    with pytest.raises(RuntimeError, match="max_keypoints"):
        matching.detect_features(img, max_keypoints=0)
    assert matching.ratio_fraction(0.8) == (4, 5) and matching.ratio_fraction(1.0) == (1, 1)


def test_oracle_matcher_ties_sentinel_and_ratio_equality():
    z, o = np.zeros(8, np.uint32), np.full(8, 0xFFFFFFFF, np.uint32)
    one = z.copy()
    one[3] = 1 << 9
    best, d1, d2 = mo.hamming_best([z, o], [one, one, z])
    assert best.tolist() == [2, 0] and d1.tolist() == [0, 255] and d2.tolist() == [1, 255]  # a tie goes to the lowest column
    assert mo.hamming_best([z], [o])[1:] == (np.array([256]), np.array([257]))
    two = one.copy()
    two[0] = 1
    # row z: best `one` at 1, second `two` at 2; 1 * 2 < 2 * 1 is false: equality rejects, a hair more accepts
    assert mo.match([z], [one, two], max_distance=256, ratio_num=1, ratio_den=2)[0].tolist() == [-1]
    assert mo.match([z], [one, two], max_distance=256, ratio_num=501, ratio_den=1000)[0].tolist() == [0]
    assert mo.match([z], [one, two], max_distance=0, ratio_num=1, ratio_den=1)[0].tolist() == [-1]
