"""The point-splat renderer (nidreg_splat_*: k_splat_depth, k_splat_resolve) against its numpy restatement (tests/viewer_oracle.py).

Every comparison is EXACT: the RGB image and the index image must equal the oracle's, np.array_equal.  No tolerance appears in this
file.  Where a case is about one rule (the tie direction, the clipping, a point just outside the image), the test first asserts on the
ORACLE's output that the rule decided something -- which pixel holds which index -- so that it cannot pass vacuously, then compares.

Most cases use a distortion-free pinhole whose numbers are powers of two and a pose that is a signed permutation (test_image_edges.PERM),
so that a point can be put onto a pixel exactly: camera (X, Y, Z) = LiDAR (Z, -X, -Y), u = 32 X / Z + W / 2.  The FoV gate is dictated
(min_nz = -1) except where the derived one is the subject."""
import ctypes
import math

import numpy as np
import pytest

import viewer_oracle
from direct_visual_lidar_calibration_amd import _lib, nid, render
from test_image_edges import PERM, POSE, Cam, dp, strided

u8p = ctypes.POINTER(ctypes.c_uint8)
i32p = ctypes.POINTER(ctypes.c_int32)
F = 32.0  # focal length of the exact pinhole, pixels


class Pinhole:
    """distortion-free plumb_bob, principal point at the image centre, focal length F"""

    def __init__(self, W, H):
        self.model, self.intr, self.dist, self.W, self.H = "plumb_bob", [F, F, W / 2.0, H / 2.0], [0.0] * 5, W, H
        self._proj = None

    @property
    def proj(self):
        if self._proj is None:
            self._proj = nid.create_camera(self.model, self.intr, self.dist)
        return self._proj


def at_pixel(cam, px, py, Z, du=0.5, dv=0.5):
    """the LiDAR-frame point that PERM and `cam` put at (px + du, py + dv), Z metres ahead"""
    X, Y = (px + du - cam.W / 2.0) / F * Z, (py + dv - cam.H / 2.0) / F * Z
    return [Z, -X, -Y, 1.0]


def colors(n, seed=0, alpha=None):
    c = np.random.default_rng(seed).integers(0, 256, size=(n, 4), dtype=np.uint8)
    if alpha is not None:
        c[:, 3] = alpha
    return c


def cloud(n, seed=1):
    """points 1 to 6 m in front of POSE's camera (LiDAR +x), wider than the pinhole cameras see; every fourth one is behind it"""
    rng = np.random.default_rng(seed)
    pts = np.ones((n, 4))
    pts[:, 0], pts[:, 1], pts[:, 2] = rng.uniform(1.0, 6.0, n), rng.uniform(-8.0, 8.0, n), rng.uniform(-6.0, 6.0, n)
    pts[3::4, 0] *= -1.0
    return pts


class Handle:
    """nidreg_splat_* through the C ABI as declared: no wrapper makes anything contiguous"""

    def __init__(self, pts, stride=32):
        self.buf, self.n = strided(pts, stride), len(pts)
        self.h = ctypes.c_void_p()
        _lib.check(_lib.load().nidreg_splat_create(0, self.n, dp(self.buf), stride, ctypes.byref(self.h)), "nidreg_splat_create")

    def set_colors(self, rgba):
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        _lib.check(_lib.load().nidreg_splat_set_colors(self.h, rgba.ctypes.data_as(u8p)), "nidreg_splat_set_colors")

    def draw_rc(self, cam, T, radius, background, alpha, min_nz, bg_stride=0, W=None, H=None, want_index=True):
        """(rc, rgb, index): the outputs are pre-filled with 7 / -7 so that a refusal can be seen to have written nothing"""
        W, H = cam.W if W is None else W, cam.H if H is None else H
        bw, bh = (1, 1) if W * H > 1 << 20 else (max(W, 1), max(H, 1))  # (a refused size: the outputs are never touched)
        rgb = np.full((bh, bw, 3), 7, dtype=np.uint8)
        idx = np.full((bh, bw), -7, dtype=np.int32) if want_index else None
        rc = _lib.load().nidreg_splat_draw(self.h, cam.proj.model_id, dp(cam.proj._intr5), dp(cam.proj._dist8), W, H, float(min_nz), dp(np.ascontiguousarray(T, dtype=np.float64)), radius,
                                           None if background is None else background.ctypes.data_as(u8p), bg_stride, alpha, rgb.ctypes.data_as(u8p),
                                           None if idx is None else idx.ctypes.data_as(i32p))
        return rc, rgb, idx

    def draw(self, cam, T, radius=1, background=None, alpha=255, min_nz=-1.0, bg_stride=0, want_index=True):
        rc, rgb, idx = self.draw_rc(cam, T, radius, background, alpha, min_nz, bg_stride, want_index=want_index)
        _lib.check(rc, "nidreg_splat_draw")
        return rgb, idx

    def close(self):
        _lib.load().nidreg_splat_destroy(self.h)


def gpu_draw(cam, pts, rgba, T, radius=1, background=None, alpha=255, min_nz=-1.0, stride=32):
    h = Handle(pts, stride)
    if len(pts):
        h.set_colors(rgba)
    out = h.draw(cam, T, radius, background, alpha, min_nz)
    h.close()
    return out


def cpu_draw(cam, pts, rgba, T, radius=1, background=None, alpha=255, min_nz=-1.0):
    return viewer_oracle.draw(cam.model, cam.intr, cam.dist, pts, rgba, T, cam.W, cam.H, min_nz, radius, background, alpha)


def same(got, want):
    assert np.array_equal(got[1], want[1]), f"index image differs at {np.argwhere(got[1] != want[1])[:8].tolist()}"
    assert np.array_equal(got[0], want[0]), f"rgb image differs at {np.argwhere(got[0] != want[0])[:8].tolist()}"


def background(cam, seed=3):
    return np.random.default_rng(seed).integers(0, 256, size=(cam.H, cam.W, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------------ the oracle alone
def test_the_oracle_at_radius_0_agrees_with_the_lidar_image_oracle():
    """(CPU) viewer_oracle's front end (transform, gate, projection, truncation) against the independent C++ restatement of
    generate_lidar_image: at radius 0 the index images are equal wherever no two points of a pixel share a float32 depth -- here
    everywhere (checked) -- for every camera model."""
    pts = cloud(2000)
    for model in ("plumb_bob", "fisheye", "omnidir", "equirectangular", "atan", "rational_polynomial"):
        cam = Cam(model, 64, 48)
        min_nz = math.cos(cam.fov())
        q, sq = viewer_oracle.point_to_pixel(cam.model, cam.intr, cam.dist, pts, POSE, cam.W, cam.H, min_nz)
        assert (q >= 0).sum() > 100 and ((q < 0).sum() > 100 or model == "equirectangular")  # (the full sphere: nothing to cut)
        keys = sorted(zip(q[q >= 0], sq[q >= 0].astype(np.float32)))
        assert all(a != b for a, b in zip(keys, keys[1:]))
        _, index = viewer_oracle.draw(cam.model, cam.intr, cam.dist, pts, colors(len(pts)), POSE, cam.W, cam.H, min_nz, radius=0)
        assert np.array_equal(index, cam.o_lidar(pts, np.zeros(len(pts)), POSE, min_z=min_nz)[1])


def test_create_refusals_need_no_device():
    """nidreg_splat_create: more than 2^31 - 1 points, a negative count, null points, point strides 24 and 36, a null `out` -- each
    NIDREG_ERR_INVALID with its message and a NULL handle, decided before any device call (this test runs without a GPU)."""
    lib = _lib.load()
    one = np.ones((1, 4))
    for n, pts, stride, text in ((2**31, one, 32, "more than 2^31 - 1 points"), (2**40, one, 32, "more than 2^31 - 1 points"), (-1, one, 32, "negative num_points"),
                                 (1, None, 32, "null points"), (1, one, 24, "point_stride"), (1, one, 36, "point_stride")):
        h = ctypes.c_void_p(1234)
        assert lib.nidreg_splat_create(0, n, dp(pts), stride, ctypes.byref(h)) == _lib.NIDREG_ERR_INVALID
        assert h.value is None and text in _lib.last_error() and "nidreg_splat_create" in _lib.last_error()
    assert lib.nidreg_splat_create(0, 1, dp(one), 32, None) == _lib.NIDREG_ERR_INVALID and "null out" in _lib.last_error()
    assert lib.nidreg_splat_set_colors(None, None) == _lib.NIDREG_ERR_INVALID
    lib.nidreg_splat_destroy(None)


# ------------------------------------------------------------------------------------------------------------------ single points
@pytest.mark.gpu
def test_no_point_and_one_point():
    """n = 0 returns the background (given, or black) and index -1 everywhere, with no colours ever set; one point at radius 1 covers
    exactly its 3 x 3 square with index 0."""
    cam = Pinhole(37, 23)
    bg = background(cam)
    for b in (None, bg):
        rgb, idx = gpu_draw(cam, np.zeros((0, 4)), None, PERM, background=b)
        assert np.array_equal(rgb, np.zeros_like(bg) if b is None else bg) and np.all(idx == -1)
    pts, c = np.array([at_pixel(cam, 18, 11, 2.0)]), colors(1, alpha=255)
    want = cpu_draw(cam, pts, c, PERM, background=bg)
    assert np.array_equal(np.argwhere(want[1] == 0), [[y, x] for y in (10, 11, 12) for x in (17, 18, 19)])
    assert np.all(want[0][11, 18] == c[0, :3]) and np.array_equal(want[0][0, 0], bg[0, 0])
    same(gpu_draw(cam, pts, c, PERM, background=bg), want)


@pytest.mark.gpu
def test_depth_order_and_the_tie_rule():
    """Two points on one pixel: the nearer wins in either index order.  Equal depths (a duplicated point, and two distinct points
    mirrored about the optical axis whose squares overlap): the LARGER index wins.  Depths that differ in fp64 and round to one float32
    (2 m and 2 m x (1 + 2^-40)): the larger index wins although it is the farther one -- and the nearer one when IT has the larger index."""
    cam = Pinhole(37, 23)
    near, far = at_pixel(cam, 18, 11, 2.0), at_pixel(cam, 18, 11, 4.0)
    c = colors(2, alpha=255)
    for pts, winner in (([near, far], 0), ([far, near], 1), ([near, near], 1), ([far, far, near, near, far], 3)):
        pts = np.array(pts)
        cc = colors(len(pts), seed=4, alpha=255)
        want = cpu_draw(cam, pts, cc, PERM, radius=2)
        assert np.all(want[1][9:14, 16:21] == winner) and (want[1] >= 0).sum() == 25
        same(gpu_draw(cam, pts, cc, PERM, radius=2), want)
    # distinct points, equal depth: mirrored about the axis in x, one pixel apart either side of the centre column -> squares overlap
    cam2 = Pinhole(36, 22)
    a, b = at_pixel(cam2, 17, 11, 2.0, du=0.75), at_pixel(cam2, 18, 11, 2.0, du=0.25)  # X = -0.25 / 32 * 2 and +0.25 / 32 * 2
    q, sq = viewer_oracle.point_to_pixel(cam2.model, cam2.intr, cam2.dist, [a, b], PERM, cam2.W, cam2.H, -1.0)
    assert q[0] + 1 == q[1] and sq[0] == sq[1]
    for pts, left_col_owner in (([a, b], 1), ([b, a], 1)):
        want = cpu_draw(cam2, np.array(pts), c, PERM, radius=1)
        shared = want[1][10:13, 17:19]
        assert np.all(shared == left_col_owner)  # both squares cover columns 17 and 18: index 1 whichever point that is
        same(gpu_draw(cam2, np.array(pts), c, PERM, radius=1), want)
    # fp64-unequal, float32-equal
    eps = 2.0**-40
    farther = at_pixel(cam, 18, 11, 2.0 * (1.0 + eps))
    q, sq = viewer_oracle.point_to_pixel(cam.model, cam.intr, cam.dist, [near, farther], PERM, cam.W, cam.H, -1.0)
    assert q[0] == q[1] and sq[0] < sq[1] and np.float32(sq[0]) == np.float32(sq[1])
    for pts, winner in (([near, farther], 1), ([farther, near], 1)):
        want = cpu_draw(cam, np.array(pts), c, PERM, radius=0)
        assert want[1][11, 18] == winner
        same(gpu_draw(cam, np.array(pts), c, PERM, radius=0), want)


# ------------------------------------------------------------------------------------------------------------------ clipping
@pytest.mark.gpu
@pytest.mark.parametrize("radius", [0, 1, 2, 8])
def test_splats_at_the_image_border(radius):
    """A point at each corner and in the middle of each edge of a 37 x 23 image, one at a time and all together (distinct depths):
    the square is clipped to the image, never wrapped into the next row."""
    cam = Pinhole(37, 23)
    W, H = cam.W, cam.H
    spots = [(0, 0), (W - 1, H - 1), (W - 1, 0), (0, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2)]
    pts = np.array([at_pixel(cam, x, y, 2.0 + 0.25 * k) for k, (x, y) in enumerate(spots)])
    c = colors(len(pts), alpha=255)
    for k, (x, y) in enumerate(spots):
        want = cpu_draw(cam, pts[k : k + 1], c[k : k + 1], PERM, radius=radius)
        cover = (min(x + radius, W - 1) - max(x - radius, 0) + 1) * (min(y + radius, H - 1) - max(y - radius, 0) + 1)
        assert (want[1] == 0).sum() == cover and want[1][y, x] == 0
        same(gpu_draw(cam, pts[k : k + 1], c[k : k + 1], PERM, radius=radius), want)
    same(gpu_draw(cam, pts, c, PERM, radius=radius), cpu_draw(cam, pts, c, PERM, radius=radius))


@pytest.mark.gpu
def test_a_splat_wider_than_the_image():
    """radius 8 on a 5 x 3 image: one point covers all 15 pixels; a nearer second point takes all of them."""
    cam = Pinhole(5, 3)
    pts, c = np.array([at_pixel(cam, 4, 0, 4.0), at_pixel(cam, 0, 2, 2.0)]), colors(2, alpha=255)
    for n, owner in ((1, 0), (2, 1)):
        want = cpu_draw(cam, pts[:n], c[:n], PERM, radius=8)
        assert np.all(want[1] == owner)
        same(gpu_draw(cam, pts[:n], c[:n], PERM, radius=8), want)


@pytest.mark.gpu
def test_a_point_just_outside_the_image_draws_nothing():
    """u in [W, W + 1), v in [H, H + 1), u or v in (-2, -1]: the centre is outside, the square would reach in, nothing is drawn.  In
    contrast u in (-1, 0) truncates to pixel 0 (the reference's cast) and IS drawn."""
    cam = Pinhole(37, 23)
    c = colors(1, alpha=255)
    outside = [at_pixel(cam, cam.W, 11, 2.0, du=0.0), at_pixel(cam, cam.W, 11, 2.0), at_pixel(cam, 18, cam.H, 2.0, dv=0.0), at_pixel(cam, -2, 11, 2.0), at_pixel(cam, -1, 11, 2.0, du=0.0),
               at_pixel(cam, 18, -2, 2.0), at_pixel(cam, cam.W, cam.H, 2.0, du=0.0, dv=0.0)]
    for p in outside:
        want = cpu_draw(cam, np.array([p]), c, PERM, radius=8)
        assert np.all(want[1] == -1) and not want[0].any()
        same(gpu_draw(cam, np.array([p]), c, PERM, radius=8), want)
    for p, (x, y) in ((at_pixel(cam, -1, 11, 2.0), (0, 11)), (at_pixel(cam, 18, -1, 2.0, dv=0.25), (18, 0))):
        want = cpu_draw(cam, np.array([p]), c, PERM, radius=0)
        assert (want[1] == 0).sum() == 1 and want[1][y, x] == 0
        same(gpu_draw(cam, np.array([p]), c, PERM, radius=0), want)
    pts = np.array(outside + [at_pixel(cam, 18, 11, 2.0)])
    same(gpu_draw(cam, pts, colors(len(pts)), PERM, radius=2), cpu_draw(cam, pts, colors(len(pts)), PERM, radius=2))


@pytest.mark.gpu
def test_a_near_splat_over_a_far_one_that_it_overlaps_in_part():
    """radius 2 at (10, 10), near, and at (12, 11), far, in both index orders: the 3 x 4 overlap belongs to the near point, the rest
    of each square to its own."""
    cam = Pinhole(37, 23)
    near, far = at_pixel(cam, 10, 10, 2.0), at_pixel(cam, 12, 11, 4.0)
    c = colors(2, alpha=255)
    for pts, n_idx in (([near, far], 0), ([far, near], 1)):
        want = cpu_draw(cam, np.array(pts), c, PERM, radius=2)
        assert (want[1] == n_idx).sum() == 25 and (want[1] == 1 - n_idx).sum() == 25 - 12 and np.all(want[1][9:13, 10:13] == n_idx)
        same(gpu_draw(cam, np.array(pts), c, PERM, radius=2), want)


# ------------------------------------------------------------------------------------------------------------------ shapes and layouts
@pytest.mark.gpu
@pytest.mark.parametrize("n", [255, 256, 257, 256 * 3 + 1])
def test_point_counts_around_a_block_on_odd_image_sizes(n):
    """Counts around the 256-thread block on 37 x 23 (851 pixels: a ragged tail for k_splat_resolve), 1 x 1 and 64 x 48, with a
    background and mixed per-point alpha; the last point of the cloud is put where it is seen, so a dropped tail thread shows."""
    pts = cloud(n, seed=n)
    c = colors(n, seed=n + 1)
    for W, H in ((37, 23), (1, 1), (64, 48)):
        cam = Cam("plumb_bob", W, H)
        pts[-1] = np.linalg.inv(POSE) @ [0.0, 0.0, 0.5, 1.0]  # on the optical axis, nearer than everything else
        bg = background(cam)
        want = cpu_draw(cam, pts, c, POSE, radius=1, background=bg, alpha=200)
        assert (want[1] == n - 1).sum() >= 1
        same(gpu_draw(cam, pts, c, POSE, radius=1, background=bg, alpha=200), want)


@pytest.mark.gpu
def test_a_point_row_stride_of_40_bytes():
    """NaN between the points; equal to the contiguous call, which equals the oracle."""
    cam, pts, c = Cam("plumb_bob", 37, 23), cloud(513), colors(513)
    want = cpu_draw(cam, pts, c, POSE, radius=1)
    assert (want[1] >= 0).sum() > 100
    same(gpu_draw(cam, pts, c, POSE, radius=1, stride=40), want)
    same(gpu_draw(cam, pts, c, POSE, radius=1, stride=32), want)


@pytest.mark.gpu
def test_alpha_and_backgrounds():
    """alpha 0, 128 and 255 over backgrounds of 0, of 255 and of noise; per-point alpha 0 (the point still owns its pixels -- the index
    image says so -- and leaves the background as it is), 1, 128, 254, 255; a null background; a background whose rows are padded (the
    padding holds 99, the oracle never sees it).  alpha 0 gives back the background whatever the colours; alpha 255 with per-point
    alpha 255 gives the colours themselves."""
    cam, pts = Cam("plumb_bob", 37, 23), cloud(300)
    c = colors(300)
    c[:, 3] = np.resize(np.array([0, 1, 128, 254, 255], dtype=np.uint8), 300)
    h = Handle(pts)
    h.set_colors(c)
    backgrounds = [None, np.zeros((cam.H, cam.W, 3), dtype=np.uint8), np.full((cam.H, cam.W, 3), 255, dtype=np.uint8), background(cam)]
    for bg in backgrounds:
        for alpha in (0, 128, 255):
            want = cpu_draw(cam, pts, c, POSE, radius=1, background=bg, alpha=alpha)
            same(h.draw(cam, POSE, 1, bg, alpha), want)
            if alpha == 0:
                assert np.array_equal(want[0], np.zeros_like(backgrounds[1]) if bg is None else bg) and (want[1] >= 0).any()
    want = cpu_draw(cam, pts, c, POSE, radius=1, background=backgrounds[3], alpha=255)
    own0 = c[np.maximum(want[1], 0), 3] == 0
    assert (own0 & (want[1] >= 0)).any() and np.array_equal(want[0][own0 & (want[1] >= 0)], backgrounds[3][own0 & (want[1] >= 0)])
    own255 = (want[1] >= 0) & (c[np.maximum(want[1], 0), 3] == 255)
    assert own255.any() and np.array_equal(want[0][own255], c[want[1][own255], :3])
    for pad in (1, 64):
        rows = np.full((cam.H, cam.W * 3 + pad), 99, dtype=np.uint8)
        rows[:, : cam.W * 3] = backgrounds[3].reshape(cam.H, -1)
        same(h.draw(cam, POSE, 1, rows, 128, bg_stride=rows.strides[0]), cpu_draw(cam, pts, c, POSE, radius=1, background=backgrounds[3], alpha=128))
    # a null index image: the picture alone
    rgb, idx = h.draw(cam, POSE, 1, backgrounds[3], 128, want_index=False)
    assert idx is None and np.array_equal(rgb, cpu_draw(cam, pts, c, POSE, radius=1, background=backgrounds[3], alpha=128)[0])
    h.close()


@pytest.mark.gpu
def test_two_draws_on_one_handle_and_new_colours_after_a_draw():
    """The key buffer is reset by every draw: a second draw under another pose (then at another image size, smaller and larger, then
    back) equals a fresh handle's, with no pixel left over from the draw before.  set_colors after a draw changes the next picture
    and not the index image."""
    pts, c = cloud(700), colors(700, alpha=255)
    cam, small, large = Cam("plumb_bob", 37, 23), Cam("plumb_bob", 7, 5), Cam("plumb_bob", 64, 48)
    other = POSE.copy()
    other[:3, 3] += [0.4, -0.2, 1.5]
    h = Handle(pts)
    h.set_colors(c)
    first = h.draw(cam, POSE, 2)
    assert not np.array_equal(cpu_draw(cam, pts, c, POSE, radius=2)[1], cpu_draw(cam, pts, c, other, radius=2)[1])
    for cm, T, r in ((cam, other, 2), (small, POSE, 1), (large, other, 0), (cam, POSE, 2)):
        got = h.draw(cm, T, r)
        same(got, cpu_draw(cm, pts, c, T, radius=r))
        same(got, gpu_draw(cm, pts, c, T, radius=r))
    same(h.draw(cam, POSE, 2), first)
    c2 = colors(700, seed=9, alpha=255)
    h.set_colors(c2)
    again = h.draw(cam, POSE, 2)
    assert np.array_equal(again[1], first[1]) and not np.array_equal(again[0], first[0])
    same(again, cpu_draw(cam, pts, c2, POSE, radius=2))
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["plumb_bob", "fisheye", "omnidir", "equirectangular", "atan", "rational_polynomial"])
def test_every_camera_model_on_a_random_cloud(model):
    """2 000 points in front of the camera on 64 x 48 under the gate SplatRenderer derives (cos(fov + 0.5 deg)), through the Python
    class: some points are drawn, some are cut (none on equirectangular, which sees the full sphere), many pixels are contested."""
    cam, pts, c = Cam(model, 64, 48), cloud(2000, seed=11), colors(2000, seed=12)
    min_nz = math.cos(cam.fov() + 0.5 * math.pi / 180.0)
    q, _ = viewer_oracle.point_to_pixel(cam.model, cam.intr, cam.dist, pts, POSE, cam.W, cam.H, min_nz)
    assert (q >= 0).sum() > 100 and ((q < 0).sum() > 100 or model == "equirectangular") and len(np.unique(q[q >= 0])) < (q >= 0).sum()
    bg = background(cam)
    r = render.SplatRenderer(pts)
    r.set_colors(c)
    for radius in (0, 2):
        same(r.draw(cam.proj, (cam.W, cam.H), POSE, radius=radius, background=bg, alpha=178), cpu_draw(cam, pts, c, POSE, radius=radius, background=bg, alpha=178, min_nz=min_nz))
    same(r.draw(cam.proj, (cam.W, cam.H), POSE, radius=1, min_nz=min_nz), cpu_draw(cam, pts, c, POSE, radius=1, min_nz=min_nz))
    r.close()


@pytest.mark.gpu
def test_non_finite_coordinates_and_depths_beyond_float32():
    """NaN and infinite coordinates, w = NaN, and a finite point on the optical axis 1e25 m away -- it projects onto the centre pixel
    and its squared distance, 1e50, is infinite as a float32: none of them draws anything, alone or among ordinary points."""
    cam = Pinhole(37, 23)
    ok = [at_pixel(cam, 5, 5, 2.0), at_pixel(cam, 30, 20, 3.0)]
    nan, inf = float("nan"), float("inf")
    bad = [[nan, 0.0, 0.0, 1.0], [2.0, nan, 0.0, 1.0], [2.0, 0.0, nan, 1.0], [2.0, 0.0, 0.0, nan], [inf, 0.0, 0.0, 1.0], [2.0, -inf, 0.0, 1.0], [inf, inf, inf, 1.0], [1e25, 0.0, 0.0, 1.0],
           [1e200, 0.0, 0.0, 1.0]]
    q, sq = viewer_oracle.point_to_pixel(cam.model, cam.intr, cam.dist, [bad[7]], PERM, cam.W, cam.H, -1.0)
    with np.errstate(over="ignore"):
        assert q[0] == 11 * cam.W + 18 and np.isfinite(sq[0]) and np.isinf(np.float32(sq[0]))
    for p in bad:
        want = cpu_draw(cam, np.array([p]), colors(1), PERM, radius=1)
        assert np.all(want[1] == -1)
        same(gpu_draw(cam, np.array([p]), colors(1), PERM, radius=1), want)
    pts = np.array(ok[:1] + bad + ok[1:])
    want = cpu_draw(cam, pts, colors(len(pts)), PERM, radius=1)
    assert sorted(np.unique(want[1])) == [-1, 0, len(pts) - 1]
    same(gpu_draw(cam, pts, colors(len(pts)), PERM, radius=1), want)


@pytest.mark.gpu
def test_refusals_of_draw():
    """radius -1 and 9, alpha -1 and 256, width * height = 2^31, a non-positive size, a background row stride of 3 W - 1, model 6, a
    null pose, a draw before any colours were set: NIDREG_ERR_INVALID, the message names the argument, and neither output is written
    (they keep their fill).  The handle still draws afterwards."""
    cam, pts, c = Pinhole(37, 23), cloud(50), colors(50)
    h = Handle(pts)
    rc, rgb, idx = h.draw_rc(cam, PERM, 1, None, 255, -1.0)
    assert rc == _lib.NIDREG_ERR_INVALID and "no colours set" in _lib.last_error() and np.all(rgb == 7) and np.all(idx == -7)
    h.set_colors(c)
    bg = background(cam)
    cases = [(dict(radius=-1), "radius"), (dict(radius=9), "radius"), (dict(alpha=-1), "alpha"), (dict(alpha=256), "alpha"), (dict(W=65536, H=32768), "overflows int"),
             (dict(W=0), "positive"), (dict(H=-3), "positive"), (dict(background=bg, bg_stride=3 * cam.W - 1), "background_row_stride")]
    for kw, text in cases:
        args = dict(radius=1, background=None, alpha=255, min_nz=-1.0, bg_stride=0, W=None, H=None)
        args.update(kw)
        rc, rgb, idx = h.draw_rc(cam, PERM, args["radius"], args["background"], args["alpha"], args["min_nz"], args["bg_stride"], args["W"], args["H"])
        assert rc == _lib.NIDREG_ERR_INVALID, kw
        assert text in _lib.last_error() and "nidreg_splat_draw" in _lib.last_error(), (kw, _lib.last_error())
        assert np.all(rgb == 7) and np.all(idx == -7), kw
    lib = _lib.load()
    rgb, idx = np.full((cam.H, cam.W, 3), 7, dtype=np.uint8), np.full((cam.H, cam.W), -7, dtype=np.int32)
    T = np.ascontiguousarray(PERM)
    for model, Tp, out, text in ((6, dp(T), rgb.ctypes.data_as(u8p), "unknown model"), (0, None, rgb.ctypes.data_as(u8p), "null argument"), (0, dp(T), None, "null argument")):
        rc = lib.nidreg_splat_draw(h.h, model, dp(cam.proj._intr5), dp(cam.proj._dist8), cam.W, cam.H, -1.0, Tp, 1, None, 0, 255, out, idx.ctypes.data_as(i32p))
        assert rc == _lib.NIDREG_ERR_INVALID and text in _lib.last_error() and np.all(rgb == 7) and np.all(idx == -7)
    same(h.draw(cam, PERM, 1, bg, 255), cpu_draw(cam, pts, c, PERM, radius=1, background=bg))
    h.close()
    r = render.SplatRenderer(pts)
    with pytest.raises(ValueError, match="one RGBA8 colour per point"):
        r.set_colors(c[:10])
    r.close()
