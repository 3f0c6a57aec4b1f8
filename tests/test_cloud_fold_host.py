"""The fold rule of include/nidreg.h (nidreg_cloud_fold_ids / nidreg_cloud_fold) without a GPU: the known vectors and the properties
of its numpy restatement (tests/fold_oracle.py), the refusals of the two entry points (which come before any device call), and the
agreement of the header with ``_lib.EXPORTS``."""
import ctypes
import math
import os
import re

import numpy as np

import fold_oracle as fo
from direct_visual_lidar_calibration_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_known_vectors():
    h = fo.hashes(np.array([0, 1, 2], dtype=np.uint64), 0)
    assert [int(v) for v in h] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    # fold = the high word of h scaled by the number of folds
    ids, sizes = fo.fold_ids(np.zeros((3, 4)), 0, 8)
    assert ids.tolist() == [(0xE220A839 * 8) >> 32, (0x6E789E6A * 8) >> 32, (0x06C45D18 * 8) >> 32] == [7, 3, 0]
    assert sizes.tolist() == [1, 0, 0, 1, 0, 0, 0, 1]


def test_oracle_properties():
    rng = np.random.default_rng(5)
    pts = np.ones((5000, 4))
    pts[:, :3] = rng.normal(size=(5000, 3)) * 20
    for K in (1, 2, 7, 64, 1024):
        for cell in (0.0, 0.5):
            ids, sizes = fo.fold_ids(pts, 11, K, cell)
            assert ids.dtype == np.int32 and ids.min() >= 0 and ids.max() < K and sizes.sum() == len(pts) and len(sizes) == K
            if K == 1:
                assert (ids == 0).all()
    a, b = fo.fold_ids(pts, 11, 8)[0], fo.fold_ids(pts, 12, 8)[0]
    assert (a != b).any()
    assert (fo.fold_ids(pts, 11, 8, 0.5)[0] != fo.fold_ids(pts, 12, 8, 0.5)[0]).any()
    # per-point folds of a few thousand points are near balanced: every fold within 5 sigma of n / K (binomial)
    _, sizes = fo.fold_ids(pts, 11, 8)
    assert np.abs(sizes - 625).max() < 5 * math.sqrt(5000 * (1 / 8) * (7 / 8))
    # two points of one cube share a fold under every seed; so do -0.0 and +0.0
    pair = np.array([[1.01, -2.99, 0.26, 1.0], [1.49, -2.51, 0.49, 1.0], [-0.0, 0.0, -0.0, 1.0], [0.0, -0.0, 0.0, 1.0], [0.25, 0.25, 0.25, 1.0]])
    k = fo.keys(pair, 0.5)
    assert k[0] == k[1] and k[2] == k[3] == k[4]
    assert k[2] == (1 << 20) | (1 << 20) << 21 | (1 << 20) << 42
    for seed in range(20):
        ids, _ = fo.fold_ids(pair, seed, 7, 0.5)
        assert ids[0] == ids[1] and ids[2] == ids[3] == ids[4]
    # what the packing cannot hold is folded on its own: key = 2^63 | i
    L = float(1 << 20)
    odd = np.array([[np.nan, 0, 0, 1], [0, np.inf, 0, 1], [0, 0, -np.inf, 1], [L * 0.5, 0, 0, 1], [-(L + 1) * 0.5, 0, 0, 1], [(L - 1) * 0.5, 0, 0, 1], [-L * 0.5, 0, 0, 1]])
    k = fo.keys(odd, 0.5)
    assert [int(v) for v in k[:5]] == [(1 << 63) | i for i in range(5)]
    assert int(k[5]) == (2 * (1 << 20) - 1) | (1 << 20) << 21 | (1 << 20) << 42 and int(k[6]) == 0 | (1 << 20) << 21 | (1 << 20) << 42
    # subset and complement partition the cloud
    s, c = fo.fold_indices(pts, 3, 8, 2, cell=0.5), fo.fold_indices(pts, 3, 8, 2, True, cell=0.5)
    assert len(np.intersect1d(s, c)) == 0 and np.array_equal(np.sort(np.concatenate([s, c])), np.arange(5000))


def test_refusals_come_before_any_device_call():
    """every call below returns NIDREG_ERR_INVALID from the argument checks: no device exists here, and none is asked for.  The cloud
    is a block of zero bytes (an empty cloud as far as the checks read it); the refusal of a NULL ``folds_out`` needs a cloud with
    points and is in tests/test_cloud_fold_gpu.py."""
    lib = _lib.load()
    fake = ctypes.create_string_buffer(256)
    cloud = ctypes.cast(fake, ctypes.c_void_p)
    ids = (ctypes.c_int32 * 4)()
    sizes = (ctypes.c_int64 * 1024)()
    out, count = ctypes.c_void_p(), ctypes.c_int64(-3)

    def fold_ids(cl=cloud, cell=0.0, K=8, idp=ids):
        return lib.nidreg_cloud_fold_ids(cl, 0, cell, K, idp, sizes)

    def fold(cl=cloud, cell=0.0, K=8, k=0, outp=out, countp=count):
        return lib.nidreg_cloud_fold(cl, 0, cell, K, k, 0, None if outp is None else ctypes.byref(outp), None, None if countp is None else ctypes.byref(countp))

    for kw in (dict(cl=None), dict(K=0), dict(K=-1), dict(K=1025), dict(cell=-1e-300), dict(cell=-1.0), dict(cell=math.nan), dict(cell=math.inf), dict(cell=-math.inf)):
        assert fold_ids(**kw) == _lib.NIDREG_ERR_INVALID, kw
        assert "nidreg_cloud_fold_ids" in _lib.last_error()
        assert fold(**kw) == _lib.NIDREG_ERR_INVALID, kw
        assert "nidreg_cloud_fold" in _lib.last_error() and not out.value and count.value == 0
    for kw in (dict(k=-1), dict(k=8), dict(K=1, k=1), dict(K=1024, k=1024), dict(outp=None), dict(countp=None)):
        assert fold(**kw) == _lib.NIDREG_ERR_INVALID, kw
        assert not out.value
    # an empty cloud's ids need no device either: every size is zero
    sizes[0] = sizes[7] = 99
    assert lib.nidreg_cloud_fold_ids(cloud, 0, 0.0, 8, None, sizes) == 0 and list(sizes[:8]) == [0] * 8


def test_header_and_exports_agree():
    src = open(os.path.join(ROOT, "include", "nidreg.h")).read()
    assert "#define NIDREG_FOLD_MAX 1024" in src and _lib.FOLD_MAX == 1024
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(nidreg_[a-z0-9_]+)\s*\(", src))
    assert {"nidreg_cloud_fold_ids", "nidreg_cloud_fold"} <= declared and declared == set(_lib.EXPORTS)
    lib = _lib.load()
    assert hasattr(lib, "nidreg_cloud_fold_ids") and hasattr(lib, "nidreg_cloud_fold")
    # the kernel sources of the folds are part of the hash the library carries
    mk = open(os.path.join(_lib.CSRC_DIR, "Makefile")).read()
    ksrc = re.search(r"^KSRC = (.*)$", mk, flags=re.M).group(1).split()
    assert "nid_fold_kernels.hpp" in ksrc and "nidreg_fold.hip" in ksrc and _lib.library_kernel_build() == _lib.kernel_source_hash()
