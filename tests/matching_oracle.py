"""numpy restatement of find_matches' device stages (csrc/nid_match_kernels.hpp), written from the description in include/nidreg.h
and not from the kernels: whole-array operations and plain loops.  Integer arithmetic throughout, so the device must EQUAL what this
returns.  It is the yardstick of tests/test_matching_gpu.py and the tool the defaults of find_matches were chosen with
(profiles/find_matches.json).  A classical stand-in for the reference's SuperGlue script, not a port of it."""
import numpy as np

BORDER = 16
NONE = 257
SEED = 0x42524945462D3235
_M = (1 << 64) - 1
# the radius-3 Bresenham circle, clockwise from 12 o'clock
CIRCLE = [(0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3)]


def _splitmix(z):
    z = (z + 0x9E3779B97F4A7C15) & _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


def brief_pairs():
    """(256, 4) int: ax ay bx by in [-15, 15]; draw c = splitmix(splitmix(SEED) + c) scaled to 31 values, coincident samples redrawn."""
    start, c, rows = _splitmix(SEED), 0, []
    while len(rows) < 256:
        v = [((_splitmix((start + c + k) & _M) * 31) >> 64) - 15 for k in range(4)]
        c += 4
        if v[:2] != v[2:]:
            rows.append(v)
    return np.array(rows, dtype=np.int64)


_PAIRS = brief_pairs()


def fill_holes(image, mask, passes):
    """``passes`` passes; each replaces an invalid pixel that has a valid 3x3 neighbour by round-half-up(mean of the valid neighbours)
    and marks it valid, reading the previous pass's arrays only.  Returns (image uint8, valid bool)."""
    img = np.asarray(image, dtype=np.int64).copy()
    ok = np.asarray(mask) != 0
    H, W = img.shape
    for _ in range(int(passes)):
        pv = np.pad(img * ok, 1)
        pk = np.pad(ok.astype(np.int64), 1)
        s = np.zeros((H, W), dtype=np.int64)
        n = np.zeros((H, W), dtype=np.int64)
        for dy in range(3):
            for dx in range(3):
                if (dy, dx) != (1, 1):
                    s += pv[dy:dy + H, dx:dx + W]
                    n += pk[dy:dy + H, dx:dx + W]
        new = ~ok & (n > 0)
        img = np.where(new, (s + n // 2) // np.maximum(n, 1), img)
        ok = ok | new
    return img.astype(np.uint8), ok


def pyr_down(src):
    """The next level at ratio 6/5: size floor(5 size / 6), destination x at source (12 x + 1) / 10, weights in tenths."""
    src = np.asarray(src, dtype=np.int64)
    sh, sw = src.shape
    dh, dw = 5 * sh // 6, 5 * sw // 6
    cy, cx = 12 * np.arange(dh) + 1, 12 * np.arange(dw) + 1
    y0, fy, x0, fx = cy // 10, cy % 10, cx // 10, cx % 10
    y1, x1 = np.minimum(y0 + 1, sh - 1), np.minimum(x0 + 1, sw - 1)
    fx, fy = fx[None, :], fy[:, None]
    top = (10 - fx) * src[y0][:, x0] + fx * src[y0][:, x1]
    bot = (10 - fx) * src[y1][:, x0] + fx * src[y1][:, x1]
    return (((10 - fy) * top + fy * bot + 50) // 100).astype(np.uint8)


def smooth(img):
    """[1 4 6 4 1] along x and along y on the edge-replicated image, one rounding: (sum + 128) >> 8."""
    p = np.pad(np.asarray(img, dtype=np.int64), 2, mode="edge")
    H, W = np.asarray(img).shape
    wt = (1, 4, 6, 4, 1)
    rows = sum(wt[i] * p[:, i:i + W] for i in range(5))
    both = sum(wt[j] * rows[j:j + H, :] for j in range(5))
    return ((both + 128) >> 8).astype(np.uint8)


def fast_scores(img):
    """Per pixel the largest t at which 9 contiguous circle pixels are all >= centre + t or all <= centre - t (0: none); 0 within 16
    pixels of the edge."""
    img = np.asarray(img, dtype=np.int64)
    H, W = img.shape
    out = np.zeros((H, W), dtype=np.int64)
    if H <= 2 * BORDER or W <= 2 * BORDER:
        return out
    ys, xs = slice(BORDER, H - BORDER), slice(BORDER, W - BORDER)
    c = img[ys, xs]
    diffs = np.stack([img[BORDER + dy:H - BORDER + dy, BORDER + dx:W - BORDER + dx] - c for dx, dy in CIRCLE])  # (16, h, w)
    best = np.zeros_like(c)
    for sign in (1, -1):
        d = sign * diffs
        for start in range(16):
            arc = [(start + k) % 16 for k in range(9)]
            best = np.maximum(best, d[arc].min(axis=0))
    out[ys, xs] = best
    return out


def nms(score, radius, threshold):
    """bool map: score >= threshold, nothing higher in the (2 r + 1)^2 window, nothing equal earlier in (y, x) order."""
    s = np.asarray(score, dtype=np.int64)
    H, W = s.shape
    keep = s >= threshold
    p = np.pad(s, radius, constant_values=-1)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if dy == 0 and dx == 0:
                continue
            o = p[radius + dy:radius + dy + H, radius + dx:radius + dx + W]
            keep &= (o <= s) if (dy, dx) > (0, 0) else (o < s)
    return keep


def to_level0(v, level, size0):
    return np.minimum(((2 * np.asarray(v, dtype=np.int64) + 1) * 6 ** level) // (2 * 5 ** level), size0 - 1)


def describe(smoothed, xs, ys):
    """(n, 8) uint32 for keypoints (xs, ys) of one level: bit k of word k // 32 = smoothed[first sample of pair k] < smoothed[second]."""
    s = np.asarray(smoothed, dtype=np.int64)
    xs, ys = np.asarray(xs, dtype=np.int64).reshape(-1, 1), np.asarray(ys, dtype=np.int64).reshape(-1, 1)
    bits = s[ys + _PAIRS[:, 1], xs + _PAIRS[:, 0]] < s[ys + _PAIRS[:, 3], xs + _PAIRS[:, 2]]  # (n, 256)
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u4").astype(np.uint32).reshape(-1, 8)


def detect(image, mask=None, levels=8, fast_threshold=20, nms_radius=4, fill_passes=2, max_keypoints=2048, capacity=65536):
    """(kpts (n, 4) int32: x0 y0 level score; desc (n, 8) uint32), ordered by (score descending, level, y, x)."""
    img = np.ascontiguousarray(image, dtype=np.uint8)
    H0, W0 = img.shape
    valid = None
    if mask is not None:
        valid = np.asarray(mask) != 0
        img, _ = fill_holes(img, valid, fill_passes)
    found, smoothed = [], {}
    for level in range(levels):
        if level > 0:
            img = pyr_down(img)
        if min(img.shape) <= 2 * BORDER:
            break
        smoothed[level] = smooth(img)
        score = fast_scores(img)
        ys, xs = np.nonzero(nms(score, nms_radius, fast_threshold))
        for y, x in zip(ys.tolist(), xs.tolist()):
            x0, y0 = int(to_level0(x, level, W0)), int(to_level0(y, level, H0))
            if valid is None or valid[y0, x0]:
                found.append((-int(score[y, x]), level, y, x, x0, y0))
    found.sort()
    found = found[: capacity if max_keypoints < 0 else max_keypoints]
    kpts = np.array([(x0, y0, level, -ns) for ns, level, y, x, x0, y0 in found], dtype=np.int32).reshape(-1, 4)
    desc = np.zeros((len(found), 8), dtype=np.uint32)
    for level in smoothed:
        sel = [i for i, f in enumerate(found) if f[1] == level]
        if sel:
            desc[sel] = describe(smoothed[level], [found[i][3] for i in sel], [found[i][2] for i in sel])
    return kpts, desc


def hamming_best(rows, cols, chunk=256):
    """Per row: (best column (lowest on a tie; -1 without columns), best distance, second-best distance; 257 where there is none)."""
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, 8)
    cols = np.asarray(cols, dtype=np.uint32).reshape(-1, 8)
    n = rows.shape[0]
    best, d1, d2 = np.full(n, -1, dtype=np.int32), np.full(n, NONE, dtype=np.int32), np.full(n, NONE, dtype=np.int32)
    if cols.shape[0] == 0:
        return best, d1, d2
    for s in range(0, n, chunk):
        d = np.bitwise_count(rows[s:s + chunk, None, :] ^ cols[None, :, :]).sum(axis=2, dtype=np.int32)  # (chunk, n1)
        j = d.argmin(axis=1)  # first minimum: the lowest column
        best[s:s + chunk] = j
        d1[s:s + chunk] = d[np.arange(d.shape[0]), j]
        if cols.shape[0] > 1:
            d[np.arange(d.shape[0]), j] = NONE
            d2[s:s + chunk] = d.min(axis=1)
    return best, d1, d2


def match(desc0, desc1, max_distance=64, ratio_num=8, ratio_den=10):
    """(match01 (n0,) int32: column or -1; best distance; second-best distance)."""
    b01, d1, d2 = hamming_best(desc0, desc1)
    b10, _, _ = hamming_best(desc1, desc0)
    out = np.full(b01.shape[0], -1, dtype=np.int32)
    for i in range(b01.shape[0]):
        j = int(b01[i])
        if j >= 0 and int(b10[j]) == i and int(d1[i]) <= max_distance and int(d1[i]) * ratio_den < int(d2[i]) * ratio_num:
            out[i] = j
    return out, d1, d2
