"""numpy restatement of ``nidreg_draw`` (include/nidreg.h), written from the rules and not from the kernel: the primitives are
painted one after another onto the canvas, so a later one simply overwrites an earlier one -- the painter's rule the device has to
reproduce with its owner words.  Integers throughout (Python / int64)."""
import numpy as np

LINE, RING, DISC = 0, 1, 2


def _axis(n_d, n_s):
    """taps (clamped) and the second tap's weight of every destination index along one axis; the denominator"""
    i = np.arange(n_d, dtype=np.int64)
    num = (2 * i + 1) * n_s - n_d
    den = 2 * n_d
    i0 = num // den  # floor (numpy's // floors for negative numerators)
    f = num - i0 * den
    return np.clip(i0, 0, n_s - 1), np.clip(i0 + 1, 0, n_s - 1), f, den


def resize(src, width, height):
    """``src`` (h, w) uint8 resized to ``width`` x ``height``: exact integer bilinear interpolation, pixel centres aligned"""
    s = np.asarray(src).astype(np.int64)
    xa, xb, fx, dx = _axis(width, s.shape[1])
    ya, yb, fy, dy = _axis(height, s.shape[0])
    wx0, wx1 = (dx - fx)[None, :], fx[None, :]
    wy0, wy1 = (dy - fy)[:, None], fy[:, None]
    total = s[ya][:, xa] * wx0 * wy0 + s[ya][:, xb] * wx1 * wy0 + s[yb][:, xa] * wx0 * wy1 + s[yb][:, xb] * wx1 * wy1
    return ((total + (dx * dy) // 2) // (dx * dy)).astype(np.uint8)


def canvas(left, right=None):
    l = np.asarray(left)
    panels = [l] if right is None else [l, resize(right, l.shape[1], l.shape[0])]
    gray = np.concatenate(panels, axis=1)
    return np.repeat(gray[:, :, None], 3, axis=2).astype(np.uint8)


def _sgn(v):
    return (v > 0) - (v < 0)


def pixels(prim):
    """Every pixel (x, y) of one primitive as two int64 arrays, canvas or not (a pixel may appear twice)"""
    kind, x0, y0, a, b = (int(v) for v in prim[:5])
    if kind == LINE:
        dx, dy = a - x0, b - y0
        n = max(abs(dx), abs(dy))
        if n == 0:
            return np.array([x0], dtype=np.int64), np.array([y0], dtype=np.int64)
        k = np.arange(n + 1, dtype=np.int64)
        return x0 + _sgn(dx) * ((2 * k * abs(dx) + n) // (2 * n)), y0 + _sgn(dy) * ((2 * k * abs(dy) + n) // (2 * n))
    if kind not in (RING, DISC):
        raise ValueError(f"unknown kind {kind}")
    o = np.arange(-a - 1, a + 2, dtype=np.int64)  # one beyond the radius on each side: the rule itself says where it ends
    ox, oy = np.meshgrid(o, o)
    d4 = 4 * (ox * ox + oy * oy)
    keep = d4 < (2 * a + 1) ** 2
    if kind == RING and a != 0:
        keep &= d4 >= (2 * a - 1) ** 2
    return x0 + ox[keep], y0 + oy[keep]


def pixel_set(prim):
    x, y = pixels(prim)
    return set(zip(x.tolist(), y.tolist()))


def draw(left, right, prims):
    """The picture ``nidreg_draw`` has to give, byte for byte"""
    out = canvas(left, right)
    h, w = out.shape[:2]
    for prim in np.asarray(prims, dtype=np.int64).reshape(-1, 8):
        x, y = pixels(prim)
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        rgb = int(prim[5])
        out[y[inside], x[inside]] = ((rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255)
    return out
