"""nidreg_draw on the GPU against tests/draw_oracle.py, byte for byte: canvases of 1 x 1, 13 x 7 and 64 x 48 with and without a right
panel (right images of 1 x 1, 5 x 29, 40 x 3 and the left one's size; contiguous and row-padded inputs), lines in every direction and
across every side and corner, the line that needs the 64-bit intermediate, rings and discs on and beyond every corner, and the
painter's order among 3 000 primitives that cross one pixel.  Integer rules on both sides: the bar is equality."""
import functools
import math

import numpy as np
import pytest

import draw_oracle as do
from direct_visual_lidar_calibration_amd import draw

pytestmark = pytest.mark.gpu

CANVASES = [(1, 1), (13, 7), (64, 48)]  # left image, width x height
RIGHTS = [None, (1, 1), (5, 29), (40, 3), "same"]  # right image, width x height


def _image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _padded(img, pad):
    """the same pixels as a view into a wider array: a row stride above the width"""
    wide = np.full((img.shape[0], img.shape[1] + pad), 0xEE, dtype=np.uint8)
    wide[:, :img.shape[1]] = img
    return wide[:, :img.shape[1]]


def _colours(prims):
    """a distinct colour per primitive, so that a wrong winner shows"""
    return [p[:5] + [(i * 5003 + 17) & 0xFFFFFF, 0, 0] for i, p in enumerate(prims)]


def edge_prims(cw, h):
    """The edge list for a canvas of cw x h (module docstring)"""
    x1, y1, mx, my = cw - 1, h - 1, cw // 2, h // 2
    L = lambda a, b, c, d: draw.line(a, b, c, d, 0)  # noqa: E731
    prims = [L(mx, my, mx, my)]  # n = 0
    for a, b, c, d in [(0, my, x1, my), (mx, 0, mx, y1),                                   # horizontal, vertical
                       (0, 0, x1, y1), (x1, 0, 0, y1), (0, 0, 5, 5), (5, 0, 0, 5),         # the four diagonals (with the reverses below)
                       (0, 0, x1, y1 // 3), (1, 0, x1 // 3, y1), (2, 1, 9, 3), (3, 0, 5, 6),  # shallow, steep
                       (-10, my, cw + 10, my + 3), (mx, -9, mx - 2, h + 11),               # both ends outside: left-right, top-bottom
                       (-7, -5, cw + 6, h + 4), (cw + 5, -6, -8, h + 7),                   # ... and through the corners
                       (-3, 2, 2, -3), (cw - 3, -2, cw + 2, 3), (-2, h - 3, 3, h + 2), (cw + 1, h - 4, cw - 4, h + 1),  # clipping each corner
                       (-20, -20, -1, -1)]:                                                # stops one pixel short of the canvas
        prims += [L(a, b, c, d), L(c, d, a, b)]  # in both directions
    prims.append(L(-32768, -32768, 32767, 32760))  # 2 k |dx| up to 2^33: the 64-bit intermediate
    prims.append(L(-300, h + 50, 300, h + 40))     # misses the canvas entirely
    for kind in (draw.ring, draw.disc):
        for r in (0, 3, 16):
            for cx, cy in ((0, 0), (x1, 0), (0, y1), (x1, y1), (-20, -20), (cw + 19, -20), (-20, h + 19), (cw + 19, h + 19), (mx, my)):
                prims.append(kind(cx, cy, r, 0))
    return _colours(prims)


@functools.lru_cache(maxsize=None)
def case(canvas, right):
    w, h = canvas
    left = _image(w, h, 3)
    rimg = None if right is None else _image(*(canvas if right == "same" else right), 4)
    prims = edge_prims(w if right is None else 2 * w, h)
    return left, rimg, prims, do.draw(left, rimg, prims)


@pytest.mark.parametrize("right", RIGHTS, ids=lambda r: "none" if r is None else r if isinstance(r, str) else "%dx%d" % r)
@pytest.mark.parametrize("canvas", CANVASES, ids=lambda c: "%dx%d" % c)
def test_picture_equals_the_oracle_byte_for_byte(canvas, right):
    left, rimg, prims, want = case(canvas, right)
    got = draw.draw(left, rimg, prims)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), np.argwhere((got != want).any(axis=2))[:8]
    # row-padded inputs: the same picture
    got = draw.draw(_padded(left, 5), None if rimg is None else _padded(rimg, 3), prims)
    assert np.array_equal(got, want)
    # no primitive: the bare canvas
    assert np.array_equal(draw.draw(left, rimg, []), do.canvas(left, rimg))


def test_the_edge_list_holds_what_it_claims():
    """(oracle only) the long line crosses the 13 x 7 canvas, the missing line misses it, every kind of clipping happens"""
    inside = lambda p, cw, h: {(x, y) for x, y in do.pixel_set(p) if 0 <= x < cw and 0 <= y < h}  # noqa: E731
    prims = edge_prims(13, 7)
    long_line = next(p for p in prims if p[:5] == [draw.LINE, -32768, -32768, 32767, 32760])
    assert len(do.pixel_set(long_line)) == 65536 and len(inside(long_line, 13, 7)) >= 6
    assert 2 * 65535 * 65535 > 2 ** 32
    missing = next(p for p in prims if p[:3] == [draw.LINE, -300, 57])
    assert not inside(missing, 13, 7)
    partly = sum(1 for p in prims if 0 < len(inside(p, 13, 7)) < len(do.pixel_set(p)))
    assert partly >= 20  # the 16 lines with an end outside that reach in, and the radius-3 and -16 rings and discs on the four corners


@functools.lru_cache(maxsize=None)
def crossing():
    """3 000 primitives of distinct colours on the 64 x 48 canvas, every one of which covers pixel (31, 23): lines whose ends mirror each
    other through it (dx and dy even: k = n / 2 is the pixel itself), discs whose centre lies within their radius of it, and rings of radius 3
    centred 3 pixels from it."""
    rng = np.random.default_rng(9)
    prims = []
    for i in range(3000):
        if i % 3 == 0:
            x, y = int(rng.integers(-40, 100)), int(rng.integers(-30, 80))
            prims.append(draw.line(x, y, 62 - x, 46 - y, 0))
        elif i % 3 == 1:
            r = int(rng.integers(0, 17))
            ox = int(rng.integers(-r, r + 1))
            m = math.isqrt(r * r - ox * ox)
            oy = int(rng.integers(-m, m + 1))
            prims.append(draw.disc(31 + ox, 23 + oy, r, 0))
        else:
            ox, oy = [(3, 0), (-3, 0), (0, 3), (0, -3), (2, 2), (-1, 3), (3, -1)][int(rng.integers(0, 7))]
            prims.append(draw.ring(31 + ox, 23 + oy, 3, 0))
    prims = _colours(prims)
    assert all((31, 23) in do.pixel_set(p) for p in prims)
    left = _image(64, 48, 5)
    return left, prims, do.draw(left, None, prims), do.draw(left, None, prims[::-1])


def _rgb(p):
    return [(p[5] >> 16) & 255, (p[5] >> 8) & 255, p[5] & 255]


def test_the_last_of_3000_primitives_across_one_pixel_wins_in_either_order_on_every_run():
    left, prims, want, want_reversed = crossing()
    got = draw.draw(left, None, prims)
    assert got[23, 31].tolist() == _rgb(prims[-1]) and np.array_equal(got, want)
    again = draw.draw(left, None, prims)
    assert again.tobytes() == got.tobytes()  # two runs: identical bytes
    got = draw.draw(left, None, prims[::-1])
    assert got[23, 31].tolist() == _rgb(prims[0]) and np.array_equal(got, want_reversed)
    assert not np.array_equal(want, want_reversed)


def test_the_larger_index_wins_between_two_workgroups():
    """one workgroup per primitive: primitives 0 and 1 race for the 33 x 33 pixels both discs cover, and 1 has to win each of them"""
    left = _image(64, 48, 6)
    for first, second in ((draw.disc(30, 24, 16, 0x0000FF), draw.disc(34, 22, 16, 0xFF0000)), (draw.disc(34, 22, 16, 0xFF0000), draw.disc(30, 24, 16, 0x0000FF))):
        got = draw.draw(left, None, [first, second])
        assert np.array_equal(got, do.draw(left, None, [first, second]))
        both = do.pixel_set(first) & do.pixel_set(second)
        assert len(both) > 500 and all(got[y, x].tolist() == _rgb(second) for x, y in both if 0 <= x < 64 and 0 <= y < 48)
