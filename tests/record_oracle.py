"""What the device record builder (csrc/nid_build.hip) has to produce, restated in Python ints and numpy -- TEST INFRASTRUCTURE ONLY.

It imports nothing of the project.  The rules, each as the reference or the library's documents state it:

  bin        t = int(intensity * bins) as the reference's x86-64 build converts (cvttsd2si): truncation toward zero, and INT_MIN when the
             product is NaN or outside (-2147483649, 2147483648); bin = max(0, min(bins - 1, t)) (nid_cost.hpp:49).  So NaN, +-inf and
             products of 2^31 and more land in bin 0.
  groups     a workgroup owns GW histogram columns: NG = ceil(bins / GW), group of a column = column // GW, gcount[g] = number of
             records in the groups before g (gcount[NG] = all records).
  wide bins  above 256 bins the occupied bins are relabelled 0, 1, 2, ... in ascending order.
  order      records are sorted by (group, column, Morton code of the bearing, input index); under NIDREG_FLAG_INPUT_ORDER by
             (group, input index).
  format     16-byte float32 records unless some KEPT point has a non-NaN coordinate that does not round-trip through float32.
"""
import math

import numpy as np

INT_MIN = -(2**31)
PI = 3.14159265358979323846


def cast_int(p):
    """double -> int as cvttsd2si does it"""
    p = float(p)
    if p != p or not (-2147483649.0 < p < 2147483648.0):
        return INT_MIN
    return math.trunc(p)


def point_bin(v, B):
    t = cast_int(np.float64(v) * np.float64(B))
    return max(0, min(int(B) - 1, t))


def point_bins(values, B):
    with np.errstate(all="ignore"):
        return np.array([point_bin(v, B) for v in np.asarray(values, dtype=np.float64)], dtype=np.int64).reshape(-1)


def default_group_width(bins):
    """columns per workgroup when the caller names none: about 256 cells"""
    return min(max(1, 256 // int(bins)), int(bins))


def groups(bins, GW):
    """NG, the number of column groups"""
    return (int(bins) + int(GW) - 1) // int(GW)


def gcount(columns, GW, NG):
    """int64[NG + 1]: record offsets of the column groups"""
    counts = np.bincount(np.asarray(columns, dtype=np.int64) // int(GW), minlength=int(NG))
    assert len(counts) == NG
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def compact(bins_of_points):
    """(labels of the points, the occupied bins ascending): label k = the k-th occupied bin"""
    occupied, labels = np.unique(np.asarray(bins_of_points, dtype=np.int64), return_inverse=True)
    return labels.astype(np.int64).reshape(-1), occupied


def quantised_bearing(x, y, z):
    """the two bearing coordinates BEFORE truncation, in float64 (NaN where the bearing is)"""
    x, y, z = float(x), float(y), float(z)
    az = math.atan2(y, x)
    el = math.atan2(z, math.sqrt(x * x + y * y))
    return (az + PI) * (65535.0 / (2.0 * PI)), (el + 0.5 * PI) * (65535.0 / PI)


def morton(x, y, z):
    fa, fe = quantised_bearing(x, y, z)
    if fa != fa or fe != fe:
        qa = qe = 0
    else:
        qa = int(min(65535.0, max(0.0, fa)))
        qe = int(min(65535.0, max(0.0, fe)))
    m = 0
    for b in range(16):
        m |= ((qa >> b) & 1) << (2 * b) | ((qe >> b) & 1) << (2 * b + 1)
    return m


def record_order(points, columns, GW, input_order):
    """indices of the points in the order their records are stored"""
    columns = np.asarray(columns, dtype=np.int64)
    n = len(columns)
    idx = np.arange(n)
    if input_order:
        return np.lexsort((idx, columns // int(GW)))
    m = np.array([morton(*p[:3]) for p in np.asarray(points, dtype=np.float64)], dtype=np.int64).reshape(-1)
    return np.lexsort((idx, m, columns, columns // int(GW)))


def needs_rec64(points):
    """the format rule over the KEPT points (n, >= 3)"""
    xyz = np.asarray(points, dtype=np.float64)[:, :3]
    with np.errstate(all="ignore"):
        back = xyz.astype(np.float32).astype(np.float64)
    return bool(np.any((back != xyz) & ~np.isnan(xyz)))


def bits(a):
    """float64 array -> its bit patterns, every NaN as one pattern (NaN coordinates compare by isnan)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = a.view(np.int64).copy()
    out[np.isnan(a)] = np.int64(0x7FF8000000000000)
    return out
