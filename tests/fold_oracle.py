"""numpy restatement of the fold rule of include/nidreg.h (nidreg_cloud_fold_ids / nidreg_cloud_fold): uint64 arrays, wrap-around
arithmetic, one double division.  The checker of tests/test_cloud_fold_host.py and tests/test_cloud_fold_gpu.py."""
import numpy as np

U = np.uint64
GOLDEN = U(0x9E3779B97F4A7C15)
AXIS = 1 << 20


def mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def keys(points, cell):
    """uint64 key per point: ``points`` (N, >=3) float64 (only its length matters when ``cell`` == 0)"""
    n = len(points)
    i = np.arange(n, dtype=np.uint64)
    if cell == 0:
        return i
    p = np.asarray(points, dtype=np.float64)[:, :3]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c = np.floor(p / np.float64(cell))
    ok = np.isfinite(p).all(axis=1) & ((c >= -AXIS) & (c < AXIS)).all(axis=1)
    ci = np.where(ok[:, None], c, 0.0).astype(np.int64) + AXIS
    packed = ci[:, 0].astype(np.uint64) | (ci[:, 1].astype(np.uint64) << U(21)) | (ci[:, 2].astype(np.uint64) << U(42))
    return np.where(ok, packed, (U(1) << U(63)) | i)


def hashes(key, seed):
    with np.errstate(over="ignore"):
        return mix64(U(int(seed) & 0xFFFFFFFFFFFFFFFF) + GOLDEN * (np.asarray(key, dtype=np.uint64) + U(1)))


def fold_ids(points, seed, num_folds, cell=0.0):
    """``(ids int32 (N,), sizes int64 (num_folds,))``"""
    h = hashes(keys(points, cell), seed)
    ids = (((h >> U(32)) * U(num_folds)) >> U(32)).astype(np.int32)
    return ids, np.bincount(ids, minlength=num_folds).astype(np.int64)


def fold_indices(points, seed, num_folds, fold, complement=False, cell=0.0):
    ids, _ = fold_ids(points, seed, num_folds, cell)
    return np.flatnonzero((ids == fold) != bool(complement)).astype(np.int32)
