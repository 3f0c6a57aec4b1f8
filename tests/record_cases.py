"""Inputs of the record-builder tests (test_record_builder_host.py checks their conditions on the CPU, test_record_builder_gpu.py feeds
them to the device) -- TEST INFRASTRUCTURE ONLY.

The scene is the undistorted plumb_bob camera of test_bin_image_edges.py on a 64 x 48 image at the identity pose.  The cloud is a pool of
4096 points unprojected from pixels strictly inside the image and rounded to float32: every one is an inlier, so hist_points is the
bincount of the bin rule.  The images hold at most 230 grey levels, so that bins = 300 and 4096 are accepted."""
import numpy as np

import record_oracle as ro
from test_bin_image_edges import IDENTITY, MAX_FOV, T_IDENTITY, Scene, cached  # noqa: F401  (re-exported)

W, H = 64, 48
POOL = 4096
EDGE_BINS = (2, 7, 16, 100, 255, 256, 300)
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)  # the smallest normal float
FLT_DENORM = 2.0**-149
# ViewCulling's gate on z / |(x y z 1)|, dictated: a point inside the image lies at most 41.8 degrees off the axis and at least 2 away,
# z / |(x y z 1)| >= cos(41.8 deg) * 2 / sqrt(5) = 0.66, so 0.5 removes none of them and every point behind the camera
MIN_Z = 0.5


def scene():
    def make():
        s = Scene(W, H, targets=lambda rng: np.stack([rng.uniform(1.0, W - 1.0, POOL), rng.uniform(1.0, H - 1.0, POOL)], -1))
        s.levels_f64 = s.rng.integers(0, 230, (H, W)) / 255.0
        s.levels_u8 = s.rng.integers(0, 230, (H, W)).astype(np.uint8)
        return s

    return cached("record scene", make)


def pool_points(n, start=0):
    assert start + n <= POOL
    return scene().pts[start:start + n].copy()


# ---- a: the intensity ladder ------------------------------------------------------------------------------------------------------------


def edges_off(B):
    """the edges k for which k / B does NOT land in bin k"""
    return [k for k in range(B + 1) if ro.cast_int(np.float64(k / B) * np.float64(B)) != k]


def ladder(B, edges=None):
    v = []
    for k in range(B + 1) if edges is None else edges:
        v += [k / B, np.nextafter(k / B, -np.inf), np.nextafter(k / B, np.inf)]
    return np.array(v)


def specials(B):
    """(values the rule puts into bin 0, values it puts into bin B - 1)"""
    first = [-0.0, -1e-300, 5e-324, np.nan, np.inf, -np.inf, 1e10, 2.0**31 / B, -2147483649.0 / B]
    last = [1.0, np.nextafter(1.0, 0.0), 1.5, (2.0**31 - 1) / B]
    return np.array(first), np.array(last)


def device_edges(B):
    """The edges whose ladder goes to the device.  Every edge -- except at 300 bins, where the whole ladder occupies 300 intensity bins
    and the library refuses more than 256 occupied ones: there every third edge, the two ends and every edge that k / B misses."""
    if B <= 256:
        return list(range(B + 1))
    return sorted(set(range(0, B + 1, 3)) | {B} | set(edges_off(B)))


def ladder_intensities(B):
    a, b = specials(B)
    return np.concatenate([ladder(B, device_edges(B)), a, b])


def ladder_cloud(B):
    v = ladder_intensities(B)
    return pool_points(len(v)), v


# ---- b: wide bins -----------------------------------------------------------------------------------------------------------------------

WIDE = 4096


def wide_intensities(occupied):
    """`occupied` point bins at 4096: bin 0 only through NaN, bin 4095 only through 1.5, the others through bin centres, several points each"""
    rng = np.random.default_rng(5)
    inner = np.sort(rng.choice(np.arange(1, WIDE - 1), occupied - 2, replace=False))
    v = np.concatenate([[np.nan, 1.5], (inner + 0.5) / WIDE])
    v = np.concatenate([v, v[rng.integers(0, len(v), 3 * len(v))]])
    return v[rng.permutation(len(v))]


# ---- c: column groups -------------------------------------------------------------------------------------------------------------------

GROUP_CONFIGS = [(16, 1), (16, 3), (16, 16), (100, 0), (256, 0)]  # (bins, columns_per_group; 0 = the default)
GROUP_SIZES = (0, 1, 2, 255, 256, 257, 1025)


def group_layout(B, cpg):
    GW = cpg if cpg else ro.default_group_width(B)
    return GW, ro.groups(B, GW)


def columns_to_intensities(cols, B):
    return (np.asarray(cols, dtype=np.float64) + 0.5) / B


def group_patterns(B, GW, NG, n=600):
    """name -> the columns of n points"""
    rng = np.random.default_rng(B * 100 + GW)
    allc = np.arange(B)

    def spread(allowed):  # every allowed column occupied, in a shuffled order
        return rng.permutation(np.resize(rng.permutation(allowed), n))

    out = {"one column": np.full(n, B // 2), "first group": spread(allc[allc // GW == 0]), "last group": spread(allc[allc // GW == NG - 1])}
    if NG > 1:
        out["first group empty"] = spread(allc[allc // GW >= 1])
        out["alternate groups empty"] = spread(allc[(allc // GW) % 2 == 1])
    return out


def random_columns(B, n, seed=0):
    return np.random.default_rng(1000 + seed).integers(0, B, n)


# ---- d: the Morton lattice --------------------------------------------------------------------------------------------------------------

LATTICE_CELLS, LATTICE_COLUMNS, LATTICE_REPEATS = 40, 3, 3


def lattice(B):
    """Bearings at the centres of cells of the 65536 x 65536 grid the Morton code interleaves, inside the image (more than 63.5 degrees of
    elevation above the x-y plane = less than 26.5 degrees off the optical axis); in every cell LATTICE_COLUMNS columns, in every
    (cell, column) LATTICE_REPEATS points at different ranges -- equal keys, which a stable sort leaves in input order.  Shuffled."""
    rng = np.random.default_rng(77 + B)
    qa = rng.choice(65535, LATTICE_CELLS, replace=False)
    qe = rng.choice(np.arange(56200, 64000), LATTICE_CELLS, replace=False)
    cols = rng.choice(B, LATTICE_COLUMNS, replace=False) if B > LATTICE_COLUMNS else np.arange(B)
    pts, columns = [], []
    for a, e in zip(qa, qe):
        az = (a + 0.5) * (2.0 * ro.PI / 65535.0) - ro.PI
        el = (e + 0.5) * (ro.PI / 65535.0) - 0.5 * ro.PI
        d = np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
        for c in cols:
            for r in rng.uniform(2.0, 9.0, LATTICE_REPEATS):
                pts.append(np.concatenate([(d * r).astype(np.float32).astype(np.float64), [1.0]]))
                columns.append(c)
    order = rng.permutation(len(pts))
    return np.array(pts)[order], np.array(columns)[order], list(zip(qa, qe))


# ---- e: the cull ------------------------------------------------------------------------------------------------------------------------


def behind(pts, which):
    """the cloud with the points `which` mirrored through the origin: behind the camera, removed by the cull"""
    out = pts.copy()
    out[which, :3] *= -1.0
    return out


def cull_cases(n=1025):
    """name -> (points, depth-buffer culling on?)"""
    base = pool_points(n, start=1024)
    idx = np.arange(n)
    return {
        "nothing removed": (base, False),
        "first removed": (behind(base, idx == 0), False),
        "last removed": (behind(base, idx == n - 1), False),
        "everything removed": (behind(base, idx >= 0), False),
        "every seventh removed": (behind(base, idx % 7 == 3), False),
        "occluded points removed": (behind(base, idx % 50 == 0), True),
    }


# ---- f: the record format ---------------------------------------------------------------------------------------------------------------

NOT_FLOAT32 = {"1 + 2^-24": 1.0 + 2.0**-24, "1e39": 1e39, "FLT_MAX (1 + 2^-25)": FLT_MAX * (1.0 + 2.0**-25)}
FORMAT_SIZES = (257, 512)  # the last index is the only lane of the last 256-thread block / its last lane


def float32_cloud(n):
    """pool points (float32 values) with the float32 values a format rule could trip over planted; returns (points, the planted rows)"""
    pts = pool_points(n, start=2048)
    planted = {3: (0, -0.0), 5: (2, FLT_MAX), 7: (0, np.inf), 8: (1, -np.inf), 9: (2, np.nan), 11: (0, FLT_MIN), 200: (1, np.nan), n - 1: (2, FLT_MAX)}
    for row, (col, value) in planted.items():
        pts[row, col] = value
    return pts, sorted(planted)


def with_last_point(pts, z):
    """the cloud with its LAST point replaced by one on the optical axis at depth z"""
    out = pts.copy()
    out[-1] = [0.0, 0.0, z, 1.0]
    return out
