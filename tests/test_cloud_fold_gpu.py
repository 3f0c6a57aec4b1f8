"""Folds of a device-resident cloud (include/nidreg.h: nidreg_cloud_fold_ids, nidreg_cloud_fold; kernels: csrc/nid_fold_kernels.hpp)
against the numpy restatement of the rule (tests/fold_oracle.py).  Everything is compared bit for bit: fold ids, sizes, index lists,
gathered bytes, and the cost and gradient of a handle built from a fold cloud against one built from the host-gathered points."""
import ctypes
import math

import numpy as np
import pytest

import fold_oracle as fo
from direct_visual_lidar_calibration_amd import _lib, nid, se3, synth

pytestmark = pytest.mark.gpu

T_TILE = _lib.SELECT_TILE
COUNTS = [0, 1, 5, 63, 64, 65, T_TILE - 1, T_TILE, T_TILE + 1, 2 * T_TILE + 1, 5000]  # wave, round and tile edges; several workgroups
FOLDS = [1, 2, 7, 64]
CELL = 0.5


def edge_points(n, seed=1):
    """(n, 4) points for cell = 0.5: a random cloud whose first rows are exact multiples of the cell on every axis (negative ones
    among them), +-0.0, a NaN / +inf / -inf in one coordinate, and cubes just inside and just outside +-2^20"""
    rng = np.random.default_rng(seed)
    pts = np.ones((n, 4))
    pts[:, :3] = rng.normal(size=(n, 3)) * 6
    L = float(1 << 20)
    special = np.array([
        [0.5, -0.5, 1.0], [-1.5, 2.0, -2.5], [-0.5, -0.5, -0.5], [3.0, 0.0, -4.0],
        [0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [-0.0, 0.25, 0.0], [0.0, 0.25, -0.0],
        [np.nan, 1.0, 2.0], [1.0, np.inf, 2.0], [1.0, 2.0, -np.inf],
        [(L - 1) * CELL, 0.1, 0.1], [L * CELL, 0.1, 0.1], [0.1, -L * CELL, 0.1], [0.1, np.nextafter(-L * CELL, -np.inf), 0.1], [0.1, 0.1, np.nextafter(L * CELL, 0.0)],
        [1e300, 0.0, 0.0], [5e-324, -5e-324, 0.3]])
    m = min(n, len(special))
    pts[:m, :3] = special[:m]
    return pts


def test_edge_points_are_what_they_claim():
    k = fo.keys(edge_points(64), CELL)
    own = [int(v) >> 63 for v in k[:18]]
    assert own == [0] * 8 + [1, 1, 1] + [0, 1, 0, 1, 0] + [1, 0]
    assert k[4] == k[5] and k[6] == k[7]  # -0.0 and +0.0 lie in one cube


@pytest.mark.parametrize("n", COUNTS)
def test_fold_ids_and_sizes_equal_the_oracle(n):
    pts = edge_points(n)
    inten = (np.arange(n) % 256) / 256.0
    cloud = nid.Cloud(pts, inten)
    empties = {}
    for K in FOLDS:
        for cell in (0.0, CELL):
            for seed in (0, 0xFFFFFFFFFFFFFFFF, 12345678901234567):
                ids, sizes = cloud.fold_ids(seed, K, cell)
                want_ids, want_sizes = fo.fold_ids(pts, seed, K, cell)
                assert ids.dtype == np.int32 and sizes.dtype == np.int64
                assert np.array_equal(ids, want_ids), (n, K, cell, seed)
                assert np.array_equal(sizes, want_sizes), (n, K, cell, seed)
        empties[K] = int((fo.fold_ids(pts, 0, K)[1] == 0).sum())
    if n == 5:
        assert empties[64] == 59
    if n in (63, 64, 65):
        assert empties[64] in (24, 25)
    assert np.array_equal(cloud.get()[0].view(np.uint64), pts.view(np.uint64))  # the source is untouched
    cloud.close()


@pytest.mark.parametrize("n", COUNTS)
def test_fold_and_complement_equal_the_host_gather(n):
    pts = edge_points(n, seed=2)
    inten = ((np.arange(n) * 7) % 256) / 256.0
    cloud = nid.Cloud(pts, inten)
    seen_empty = False
    for K, k in ((1, 0), (2, 1), (7, 3), (64, 0), (64, 63)):
        for cell in (0.0, CELL):
            seed = 40 + K
            sub, si = cloud.fold(seed, K, k, cell=cell, return_indices=True)
            com, ci = cloud.fold(seed, K, k, complement=True, cell=cell, return_indices=True)
            want_s, want_c = fo.fold_indices(pts, seed, K, k, cell=cell), fo.fold_indices(pts, seed, K, k, True, cell=cell)
            assert si.dtype == np.int32 and np.array_equal(si, want_s) and np.array_equal(ci, want_c), (n, K, k, cell)
            assert (np.diff(si) > 0).all() and (np.diff(ci) > 0).all()
            assert len(np.intersect1d(si, ci)) == 0 and np.array_equal(np.sort(np.concatenate([si, ci])), np.arange(n))
            for c, idx in ((sub, si), (com, ci)):
                assert c.num_points == len(idx) and c.device == cloud.device
                gp, gi = c.get()
                assert gp.tobytes() == pts[idx].tobytes() and gi.tobytes() == inten[idx].tobytes()
                if len(idx) == 0 and not seen_empty:  # an empty fold is a valid empty cloud: its handle builds and evaluates to "not ok"
                    seen_empty = True
                    scene = synth.make_scene("pinhole_vga", num_points=100, seed=7)
                    proj = nid.create_camera(scene.model, scene.intrinsics, scene.distortion)
                    h = nid.NIDCost.from_cloud(proj, scene.image_f64, c, 16, cull=None)
                    assert h.num_points == 0 and not h(scene.T_camera_lidar_init)[0]
                    h.close()
                c.close()
    assert seen_empty  # (K = 1 with the complement, if nothing else)
    gp, gi = cloud.get()
    assert gp.tobytes() == pts.tobytes() and gi.tobytes() == inten.tobytes()  # the source is untouched
    cloud.close()


def test_float32_cloud_folds_like_its_double_twin():
    rng = np.random.default_rng(3)
    xyz = (rng.normal(size=(3000, 3)) * 8).astype(np.float32)
    xyz[:4] = [[0.5, -0.5, 1.0], [-0.0, 0.0, 0.0], [np.nan, 0, 0], [np.inf, 0, 0]]
    inten = (rng.integers(0, 256, 3000) / 256.0).astype(np.float32)
    a = nid.Cloud.from_float32(xyz, inten)
    pts = np.ones((3000, 4))
    pts[:, :3] = xyz.astype(np.float64)
    b = nid.Cloud(pts, inten.astype(np.float64))
    for cell in (0.0, CELL):
        ia, sa = a.fold_ids(9, 7, cell)
        ib, sb = b.fold_ids(9, 7, cell)
        assert np.array_equal(ia, ib) and np.array_equal(sa, sb) and np.array_equal(ia, fo.fold_ids(pts, 9, 7, cell)[0])
        fa, xa = a.fold(9, 7, 2, cell=cell, return_indices=True)
        fb, xb = b.fold(9, 7, 2, cell=cell, return_indices=True)
        assert np.array_equal(xa, xb) and fa.get()[0].tobytes() == fb.get()[0].tobytes() and fa.get()[1].tobytes() == fb.get()[1].tobytes()
        fa.close(), fb.close()
    a.close(), b.close()


@pytest.fixture(scope="module")
def scene():
    return synth.make_scene("pinhole_vga", num_points=12000, seed=7)


def test_a_handle_on_a_fold_cloud_is_the_handle_on_the_host_gathered_points(scene):
    proj = nid.create_camera(scene.model, scene.intrinsics, scene.distortion)
    cloud = nid.Cloud(scene.points, scene.intensities)
    x = scene.T_camera_lidar_init
    for complement, cell in ((False, 1.0), (True, 1.0), (True, 0.0)):
        sub, idx = cloud.fold(5, 4, 1, complement=complement, cell=cell, return_indices=True)
        assert np.array_equal(idx, fo.fold_indices(scene.points, 5, 4, 1, complement, cell)) and 1000 < len(idx) < 11000
        twin = nid.Cloud(np.ascontiguousarray(scene.points[idx]), np.ascontiguousarray(scene.intensities[idx]))
        T = se3.to_matrix(x)
        min_z = math.cos(nid.estimate_camera_fov(proj, (scene.width, scene.height)))
        for cull in (None, (T, min_z, True)):
            a = nid.NIDCost.from_cloud(proj, scene.image_f64, sub, 16, cull=cull)
            b = nid.NIDCost.from_cloud(proj, scene.image_f64, twin, 16, cull=cull)
            ra, rb = a(x), b(x)
            assert a.num_points == b.num_points > 0
            assert ra[0] == rb[0] and ra[1] == rb[1] and np.array_equal(np.asarray(ra[2]), np.asarray(rb[2]))  # ok, cost, gradient: bit for bit
            assert np.array_equal(a.histogram_fixed()[0], b.histogram_fixed()[0])
            a.close(), b.close()
        # nidreg_cloud_select on a fold cloud returns what it returns on the host-gathered cloud
        s1, i1 = sub.select(proj, (scene.width, scene.height), T, min_z, True, min_range=6.0, return_indices=True)
        s2, i2 = twin.select(proj, (scene.width, scene.height), T, min_z, True, min_range=6.0, return_indices=True)
        assert np.array_equal(i1, i2) and 0 < len(i1) < len(idx) and s1.select_counts == s2.select_counts
        assert s1.get()[0].tobytes() == s2.get()[0].tobytes() and s1.get()[1].tobytes() == s2.get()[1].tobytes()
        for c in (s1, s2, sub, twin):
            c.close()
    cloud.close()


def test_refusals_that_need_a_cloud_and_select_counts_on_a_fold_cloud(scene):
    lib = _lib.load()
    cloud = nid.Cloud(scene.points[:100], scene.intensities[:100])
    sizes = (ctypes.c_int64 * 8)()
    assert lib.nidreg_cloud_fold_ids(cloud.c, 0, 0.0, 8, None, sizes) == _lib.NIDREG_ERR_INVALID and "folds_out" in _lib.last_error()
    ids, no_sizes = np.empty(100, dtype=np.int32), None
    assert lib.nidreg_cloud_fold_ids(cloud.c, 0, 0.0, 8, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), no_sizes) == 0  # sizes_out is optional
    assert np.array_equal(ids, fo.fold_ids(scene.points[:100], 0, 8)[0])
    sub = cloud.fold(0, 8, 0)
    c3 = (ctypes.c_int64 * 3)()
    assert lib.nidreg_cloud_select_counts(sub.c, c3) == _lib.NIDREG_ERR_INVALID  # a fold is not a selection
    with pytest.raises(RuntimeError, match="num_folds"):
        cloud.fold_ids(0, 1025)
    with pytest.raises(RuntimeError, match="fold must lie"):
        cloud.fold(0, 8, 8)
    sub.close(), cloud.close()
