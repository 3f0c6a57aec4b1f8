"""GPU tests of the CT-GICP model's LRU eviction (``nidreg_odom_set_lru``, ``k_odom_evict`` and the stamps of ``k_odom_model_insert`` /
``k_odom_linearize`` in csrc/nid_odom_kernels.hpp; ``odometry.DeviceBackend(lru_thresh=..., lru_cycle=...)``; ``preprocess_dynamic
--lru_thresh``).  The yardstick is ``IVoxLRU`` of tests/odometry_lru_oracle.py, a restatement of ivox.cpp:144-178 and :223 that is
unpinned against a compiled reference.  Every comparison with it is exact unless it says otherwise, after EVERY insert."""
import filecmp
import os

import numpy as np
import pytest

import odometry_lru_oracle as lru
import odometry_oracle as oracle
import rosbag1_fixture as fx
from direct_visual_lidar_calibration_amd import odometry, preprocess_dynamic, se3

pytestmark = pytest.mark.gpu
IDENT = odometry.pack_poses(np.eye(4)[None], np.zeros((1, 6, 6)), np.zeros((1, 6, 6)))
IDENT12 = odometry.pack_poses(np.eye(4)[None])


def covs_for(n, seed=0):
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(0.1, 1.0, size=(n, 6)))


def unit_covs(n):
    return np.tile(np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0]), (n, 1))


def assert_model_equals(b, ivox):
    """The surviving voxels, every voxel's ordered list, and the counters the library keeps of them"""
    vox, pts, covs = b.model_points()
    keys, want_pts, want_covs = ivox.flat()
    assert np.array_equal(oracle.pack_key((vox[:, 0], vox[:, 1], vox[:, 2])), keys)
    assert np.array_equal(pts, want_pts) and np.array_equal(covs, want_covs)
    info = b.model_info()
    assert info["points"] == keys.shape[0] and info["voxels"] == len(ivox.voxels)
    assert info["blocks"] == sum(max(1, -(-len(p) // 64)) for p, _ in ivox.voxels.values())  # in use: what the surviving chains hold


def assert_lru_equals(b, ivox, passes=None):
    got = b.lru_info()
    assert got["lru_count"] == ivox.lru_count and got["evicted_voxels"] == sum(len(e) for e in ivox.evicted)
    if passes is not None:
        assert got["passes"] == passes
    return got


def insert_both(b, ivox, pts, covs=None):
    pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 3))
    covs = unit_covs(pts.shape[0]) if covs is None else covs
    b.model_insert(pts, covs)
    ivox.insert(pts, covs)
    assert_model_equals(b, ivox)


def search_both(b, ivox, q, max_dist_sq=1.0):
    """One linearisation at the identity on the device and on the oracle (both stamp what they find); correspondences are exact"""
    q = np.ascontiguousarray(np.asarray(q, dtype=np.float64).reshape(-1, 3))
    tidx = np.zeros(q.shape[0], dtype=np.int32)
    b.set_source(q, unit_covs(q.shape[0]), tidx)
    sums = b.linearize(IDENT, max_dist_sq)
    want = oracle.linearize(q, unit_covs(q.shape[0]), tidx, IDENT, ivox, max_dist_sq)
    found, target, _ = b.correspondences()
    assert np.array_equal(found, want["found"]) and np.array_equal(target, want["target"]) and sums[121] == want["sums"][121]
    return sums, found, target


def centre(v, d=(0.0, 0.0, 0.0)):
    return [v[0] + 0.5 + d[0], v[1] + 0.5 + d[1], v[2] + 0.5 + d[2]]


# ---- 2. the library's own logic ---------------------------------------------------------------------------------------------------------
def test_set_lru_refusals_and_lru_info_of_a_fresh_handle():
    b = odometry.DeviceBackend(0, max_blocks=4)
    try:
        assert b.lru_info() == {"lru_count": 0, "evicted_voxels": 0, "free_blocks": 0, "passes": 0}
        with pytest.raises(ValueError, match="lru_thresh must be >= 0"):
            b.set_lru(-1, 10)
        for cycle in (0, -3):
            with pytest.raises(ValueError, match="lru_cycle must be >= 1"):
                b.set_lru(5, cycle)
        b.set_lru(5, 2)
        b.set_lru(0, 1)  # off again: still before the first insert
        b.set_lru(3, 7)
        b.model_insert(np.zeros((0, 3)), np.zeros((0, 6)))  # an empty call does not reach the device: it neither counts nor closes the door
        b.set_lru(2, 2)
        b.model_insert(np.array([centre((0, 0, 0))]), unit_covs(1))
        assert b.lru_info() == {"lru_count": 1, "evicted_voxels": 0, "free_blocks": 0, "passes": 0}
        for args in ((2, 2), (0, 10)):
            with pytest.raises(ValueError, match="before the first nidreg_odom_model_insert"):
                b.set_lru(*args)
    finally:
        b.close()
    with pytest.raises(ValueError, match="lru_thresh must be >= 0"):
        odometry.DeviceBackend(0, max_blocks=4, lru_thresh=-2)


# ---- 3. the rule's edges ------------------------------------------------------------------------------------------------------------------
def test_rule_edges_on_the_hand_worked_schedule():
    """The schedule of tests/test_odometry_lru_host.py: no pass while the horizon is <= 0 or off the cycle, a voxel AT the horizon stays,
    and a voxel refreshed only by a refused point or only by a search stays"""
    b, ivox = odometry.DeviceBackend(0, max_blocks=16, lru_thresh=lru.RULE_EDGES_THRESH, lru_cycle=lru.RULE_EDGES_CYCLE), lru.IVoxLRU(lru_thresh=2, lru_cycle=3)
    try:
        inserts = 0
        for kind, pts, want in lru.RULE_EDGES:
            if kind == "insert":
                insert_both(b, ivox, pts)
                inserts += 1
            else:
                _, found, target = search_both(b, ivox, pts)
                assert found.tolist() == [1] and np.array_equal(target[0], centre((lru.B, 0, 0)))
                assert_model_equals(b, ivox)
            assert {int(v[0]) for v in b.model_points()[0]} == want  # the voxels written out in the schedule
            got = assert_lru_equals(b, ivox, passes=inserts // 3)
            assert got["free_blocks"] == (3 if inserts == 6 else 0)
        assert b.model_info() == {"voxels": 5, "points": lru.RULE_EDGES_POINTS_AT_END, "blocks": 5, "max_blocks": 16}
        assert b.lru_info() == {"lru_count": 6, "evicted_voxels": 3, "free_blocks": 3, "passes": 2}
    finally:
        b.close()


# ---- 4. touch by search ---------------------------------------------------------------------------------------------------------------------
VA, VB, VC, VD = (0, 0, 0), (1, 0, 0), (10, 1, 0), (1, 1, 0)
PA, PB, PC, PD = [0.9, 0.5, 0.5], [1.5, 0.5, 0.5], [10.5, 1.9, 0.5], [1.5, 1.5, 0.5]
Q1, Q2 = [0.95, 0.5, 0.5], [10.5, 0.5, 0.5]  # Q1 in A: A's point wins, B's (a face neighbour) loses, D is diagonal; Q2 in the absent
#                                              voxel (10, 0, 0): C's point, 1.4 m off in a face neighbour, is the nearest and fails 1 m^2


@pytest.mark.parametrize("search", [True, False])
def test_a_search_stamps_every_face_neighbour_it_finds(search):
    b, ivox = odometry.DeviceBackend(0, max_blocks=16, lru_thresh=1, lru_cycle=3), lru.IVoxLRU(lru_thresh=1, lru_cycle=3)
    try:
        insert_both(b, ivox, [PA, PB, PC, PD])  # 1
        insert_both(b, ivox, [centre((30, 0, 0))])  # 2: elsewhere
        if search:
            _, found, target = search_both(b, ivox, [Q1, Q2])
            assert found.tolist() == [1, 0] and np.array_equal(target[0], PA)
        insert_both(b, ivox, [centre((33, 0, 0))])  # 3: the pass, horizon 2
        left = {tuple(int(c) for c in v) for v in b.model_points()[0]}
        assert left == ({VA, VB, VC} if search else set()) | {(30, 0, 0), (33, 0, 0)}  # D (and, unsearched, all four) is gone
        assert b.lru_info() == {"lru_count": 3, "evicted_voxels": 1 if search else 4, "free_blocks": 1 if search else 4, "passes": 1}
    finally:
        b.close()


# ---- 5. probe chains ----------------------------------------------------------------------------------------------------------------------
def colliding_voxels(mask, want=3):
    """``want`` voxels (x, 0, 0), no two face neighbours, whose probes start at one slot, and a far voxel that starts at least 8 slots off"""
    seen = {}
    for x in range(0, 30000, 3):
        group = seen.setdefault(oracle.home_slot((x, 0, 0), mask), [])
        group.append((x, 0, 0))
        if len(group) == want:
            home = oracle.home_slot(group[0], mask)
            far = next((x2, 7, 0) for x2 in range(0, 3000, 3) if min((oracle.home_slot((x2, 7, 0), mask) - home) & mask, (home - oracle.home_slot((x2, 7, 0), mask)) & mask) >= 8)
            return group, far
    raise AssertionError("no colliding keys")


@pytest.mark.parametrize("victim", [0, 1])  # the chain's head, and a key in its middle
def test_eviction_keeps_the_probe_chains_of_the_keys_that_stay(victim):
    mask = 1023  # max_blocks = 16: a table of 1024 slots
    chain, far = colliding_voxels(mask)
    assert len({oracle.home_slot(v, mask) for v in chain}) == 1 and len(set(chain)) == 3
    keep = [v for i, v in enumerate(chain) if i != victim]
    b, ivox = odometry.DeviceBackend(0, max_blocks=16, lru_thresh=1, lru_cycle=4), lru.IVoxLRU(lru_thresh=1, lru_cycle=4)
    try:
        for v in chain:  # 1, 2, 3: one call each, so the keys take the slots home, home + 1, home + 2 in this order
            insert_both(b, ivox, [centre(v), centre(v, (0.2, 0.0, 0.0))])
        insert_both(b, ivox, [centre(v, (0.0, 0.2, 0.0)) for v in keep] + [centre(far)])  # 4: the others refreshed (and extended); horizon 3: the victim leaves
        assert {tuple(int(c) for c in v) for v in b.model_points()[0]} == set(keep) | {far} and b.lru_info()["evicted_voxels"] == 1
        # the keys behind the victim are still found: a search in each returns its own point
        q = [centre(v, (0.21, 0.0, 0.0)) for v in keep] + [centre(chain[victim], (0.21, 0.0, 0.0))]
        _, found, target = search_both(b, ivox, q)
        assert found.tolist() == [1, 1, 0] and np.array_equal(target[:2], [centre(v, (0.2, 0.0, 0.0)) for v in keep])
        insert_both(b, ivox, [centre(v, (0.0, 0.0, 0.2)) for v in keep])  # 5: the old lists are extended ...
        for v in keep:
            assert len(ivox.voxels[v][0]) == 4
        insert_both(b, ivox, [centre(chain[victim], (0.0, 0.0, -0.2))])  # 6: ... and the evicted key starts an empty voxel
        assert len(ivox.voxels[chain[victim]][0]) == 1
        vox, pts, _ = b.model_points()
        mine = np.all(vox == np.array(chain[victim]), axis=1)
        assert mine.sum() == 1 and np.array_equal(pts[mine][0], centre(chain[victim], (0.0, 0.0, -0.2)))  # the old points are gone
        _, found, target = search_both(b, ivox, q)
        assert found.tolist() == [1, 1, 1]
        assert b.model_info()["blocks"] == 4 and b.lru_info()["free_blocks"] == 0  # the victim's block went to its successor
    finally:
        b.close()


# ---- 6. recycling -------------------------------------------------------------------------------------------------------------------------
def rotation(steps=32, big=10):
    """Per insert one fresh voxel, 10 m from the last; voxel ``big`` receives 130 points, 10 cm apart (three chained blocks)"""
    g = np.stack(np.meshgrid(np.arange(9) * 0.1 + 0.05, np.arange(9) * 0.1 + 0.05, np.arange(2) * 0.1 + 0.05, indexing="ij"), axis=-1).reshape(-1, 3)[:130]
    return [(g if i == big else np.array([[0.5, 0.5, 0.5]])) + [10.0 * i, 0.0, 0.0] for i in range(steps)]


def test_blocks_of_evicted_voxels_are_handed_out_again():
    """max_blocks = 8 and lru_thresh = lru_cycle = 1: after every insert but the first a pass drops what the last two inserts did not
    touch.  34 blocks are requested over the run (31 voxels of one block, one of three), more than 4 x max_blocks."""
    frames = rotation()
    assert sum(max(1, -(-f.shape[0] // 64)) for f in frames) >= 4 * 8
    b, ivox = odometry.DeviceBackend(0, max_blocks=8, lru_thresh=1, lru_cycle=1), lru.IVoxLRU(lru_thresh=1, lru_cycle=1)
    try:
        free, handed_out, rose_by_three = 0, 0, False
        for i, f in enumerate(frames):
            need = max(1, -(-f.shape[0] // 64))
            popped = min(free, need)  # the free stack first, the bump counter for the rest
            handed_out += need - popped
            before = free - popped
            insert_both(b, ivox, f, covs_for(f.shape[0], i))  # (no ModelFullError)
            released = sum(max(1, -(-n // 64)) for _, n in ivox.evicted[-1])
            free = before + released
            info, got = b.model_info(), assert_lru_equals(b, ivox, passes=i)
            assert got["free_blocks"] == free and info["blocks"] == handed_out - free and info["blocks"] <= 8 and info["voxels"] == min(i + 1, 2)
            if [n for _, n in ivox.evicted[-1]] == [130]:
                assert got["free_blocks"] == before + 3  # a chain of three blocks came back
                rose_by_three = True
        assert rose_by_three and handed_out <= 5 and b.lru_info()["evicted_voxels"] == 30
    finally:
        b.close()
    control = odometry.DeviceBackend(0, max_blocks=8, lru_thresh=0, lru_cycle=1)  # the same sequence on a model that only grows
    try:
        with pytest.raises(odometry.ModelFullError, match="exhausted"):
            for i, f in enumerate(frames):
                control.model_insert(np.ascontiguousarray(f), covs_for(f.shape[0], i))
        assert control.model_info()["blocks"] == 8 and control.lru_info()["evicted_voxels"] == 0
    finally:
        control.close()


def test_the_pool_grows_past_its_first_size_while_recycled_blocks_are_in_use():
    """The pool starts at 1024 blocks.  900 voxels are dropped, then 1300 fresh ones arrive in one call: 900 blocks come from the free
    stack and the rest from a pool that has to grow, with the recycled blocks and their links copied over"""
    b, ivox = odometry.DeviceBackend(0, max_blocks=4096, lru_thresh=1, lru_cycle=1), lru.IVoxLRU(lru_thresh=1, lru_cycle=1)
    try:
        grid = np.stack(np.meshgrid(np.arange(40), np.arange(40), [0], indexing="ij"), axis=-1).reshape(-1, 3) + 0.5
        insert_both(b, ivox, grid[:900], covs_for(900, 1))
        insert_both(b, ivox, [centre((100, 0, 5))])
        insert_both(b, ivox, [centre((120, 0, 5))])  # the pass with horizon 2: the 900 leave
        assert b.lru_info()["free_blocks"] == 900 and b.model_info()["blocks"] == 2
        insert_both(b, ivox, grid[:1300] + [0.0, 0.0, 9.0], covs_for(1300, 2))  # (the pass of this insert drops voxel 100)
        assert b.model_info() == {"voxels": 1301, "points": 1301, "blocks": 1301, "max_blocks": 4096} and b.lru_info()["free_blocks"] == 1
        _, found, _ = search_both(b, ivox, grid[:1300:7] + [0.01, 0.0, 9.0])
        assert found.all()
    finally:
        b.close()


# ---- 7. evict everything, then go on --------------------------------------------------------------------------------------------------------
def test_a_pass_that_removes_every_voxel_leaves_a_model_that_works():
    """An insert stamps the voxels it reaches, so a pass can only empty the model after inserts that created nothing: with a pool of two
    blocks, both held, a third voxel is refused (NIDREG_ERR_FULL: the call counts, nothing enters); the oracle, which has no pool, is given
    an empty scan for such a call.  After two of them (lru_thresh = 1, lru_cycle = 3) both voxels are stale and leave."""
    b, ivox = odometry.DeviceBackend(0, max_blocks=2, lru_thresh=1, lru_cycle=3), lru.IVoxLRU(lru_thresh=1, lru_cycle=3)
    try:
        insert_both(b, ivox, [centre((0, 0, 0)), centre((5, 0, 0))])
        for _ in range(2):
            with pytest.raises(odometry.ModelFullError, match="exhausted"):
                b.model_insert(np.array([centre((9, 0, 0))]), unit_covs(1))
            ivox.insert(np.zeros((0, 3)), np.zeros((0, 6)))
            assert_model_equals(b, ivox)
        assert b.model_info() == {"voxels": 0, "points": 0, "blocks": 0, "max_blocks": 2}
        assert b.lru_info() == {"lru_count": 3, "evicted_voxels": 2, "free_blocks": 2, "passes": 1}
        vox, pts, covs = b.model_points()
        assert vox.shape == (0, 3) and pts.shape == (0, 3) and covs.shape == (0, 6)
        sums, found, _ = search_both(b, ivox, [centre((0, 0, 0)), centre((5, 0, 0)), centre((9, 0, 0))])
        assert np.array_equal(sums, np.zeros(122)) and found.sum() == 0 and b.error(IDENT12) == (0.0, 0)
        insert_both(b, ivox, [centre((9, 0, 0)), centre((0, 0, 0), (0.1, 0.0, 0.0))])  # both blocks come from the free stack
        assert b.model_info() == {"voxels": 2, "points": 2, "blocks": 2, "max_blocks": 2} and b.lru_info()["free_blocks"] == 0
        _, found, _ = search_both(b, ivox, [centre((0, 0, 0)), centre((9, 0, 0))])
        assert found.tolist() == [1, 1]
    finally:
        b.close()


# ---- 8. the same bits as a fresh model ----------------------------------------------------------------------------------------------------------
def slab(x0, seed, n=220):
    """A noisy floor and wall over x in [x0, x0 + 3)"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.0, 1.0, size=(n, 2))
    floor = np.stack([x0 + 3.0 * u[: n // 2, 0], -1.0 + 3.0 * u[: n // 2, 1], -0.3 + rng.normal(0.0, 2e-3, n // 2)], axis=1)
    wall = np.stack([x0 + 3.0 * u[n // 2 :, 0], 1.4 + rng.normal(0.0, 2e-3, n - n // 2), -1.0 + 2.5 * u[n // 2 :, 1]], axis=1)
    return np.ascontiguousarray(np.concatenate([floor, wall]))


@pytest.fixture(scope="module")
def evicted_and_fresh():
    """A model after a pass that removed part of it, and a model that only ever received the survivors, voxel by voxel in list order"""
    b, ivox = odometry.DeviceBackend(0, max_blocks=256, lru_thresh=1, lru_cycle=2), lru.IVoxLRU(lru_thresh=1, lru_cycle=2)
    fresh = odometry.DeviceBackend(0, max_blocks=256)
    for i in range(4):  # slabs that overlap by a metre; the pass after the fourth (horizon 3) drops what the last two did not reach
        pts = slab(2.0 * i, 40 + i)
        _, _, covs = b.knn_covariances(pts, 10)
        insert_both(b, ivox, pts, covs)
    assert sum(len(e) for e in ivox.evicted) >= 4 and sum(n for e in ivox.evicted for _, n in e) >= 100 and len(ivox.voxels) >= 8
    _, pts, covs = ivox.flat()
    fresh.model_insert(pts, covs)
    assert all(np.array_equal(x, y) for x, y in zip(fresh.model_points(), b.model_points()))
    yield b, fresh, ivox
    b.close(), fresh.close()


@pytest.mark.parametrize("m", [63, 65])
def test_after_a_pass_results_have_the_bits_of_a_fresh_model_of_the_survivors(evicted_and_fresh, m):
    b, fresh, ivox = evicted_and_fresh
    rng = np.random.default_rng(m)
    T0 = se3.pose3_exp(np.r_[0.02, -0.03, 0.05, 0.1, -0.05, 0.02])
    T1 = T0 @ se3.pose3_exp(np.r_[0.01, 0.02, -0.03, 0.04, 0.03, -0.01])
    poses, d0, d1 = odometry.update_poses(T0, T1, np.linspace(0.0, 1.0, 3))
    _, mpts, _ = ivox.flat()
    land = mpts[rng.integers(0, mpts.shape[0], size=m)] + rng.normal(0.0, 0.02, size=(m, 3))
    land[0] = [0.5, 0.5, -0.3]  # where the evicted part was: nothing is found there any more
    tidx = rng.integers(0, 3, size=m).astype(np.int32)
    P = poses[tidx]
    src = np.ascontiguousarray(np.einsum("nji,nj->ni", P[:, :3, :3], land - P[:, :3, 3]))
    covs = covs_for(m, m) * [1.0, 0.0, 0.0, 1.0, 0.0, 1.0]
    packed, packed12 = odometry.pack_poses(poses, d0, d1), odometry.pack_poses(poses)
    moved = packed12.copy()
    moved[:, 9:] += [0.01, -0.02, 0.005]
    out = []
    for h in (b, fresh):
        h.set_source(src, covs, tidx)
        sums = h.linearize(packed)
        out.append((sums, h.error(packed12), h.error(moved)) + h.correspondences())
    for x, y in zip(*out):
        assert np.array_equal(np.asarray(x), np.asarray(y))  # all 122 sums, both errors, found, targets and Mahalanobis matrices
    sums, found = out[0][0], out[0][3]
    want = oracle.linearize(src, covs, tidx, packed, ivox)
    assert np.array_equal(found, want["found"]) and np.array_equal(out[0][4], want["target"]) and found[0] == 0 and sums[121] >= m - 8


# ---- 9. eviction off is the model that only grows ---------------------------------------------------------------------------------------------
def test_lru_thresh_zero_equals_a_handle_that_was_never_given_set_lru():
    never, off = odometry.DeviceBackend(0, max_blocks=64), odometry.DeviceBackend(0, max_blocks=64, lru_thresh=0, lru_cycle=1)
    try:
        got = []
        for h in (never, off):
            for i in range(3):
                pts = slab(40.0 * i, 70 + i, 150)  # three places far apart: with any threshold and lru_cycle = 1 something would leave
                h.model_insert(pts, covs_for(150, i))
            q = slab(0.0, 70, 150)[:65] + 0.01
            h.set_source(q, unit_covs(65), np.zeros(65, dtype=np.int32))
            got.append((h.linearize(IDENT),) + h.correspondences() + h.model_points() + (h.model_info(), h.lru_info()))
        for x, y in zip(*got[:2]):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
        assert got[0][-1] == {"lru_count": 3, "evicted_voxels": 0, "free_blocks": 0, "passes": 0} and got[0][0][121] >= 60
    finally:
        never.close(), off.close()


# ---- 10. the scan matcher, end to end ---------------------------------------------------------------------------------------------------------
# A sensor that sees 3.5 m, through a window of 140 degrees of azimuth, is carried down a corridor at 0.5 m/s while the window turns by
# 20 degrees per scan (a full turn in 18 scans): what the window leaves falls out of the model, and after a turn it is met again.
CORRIDOR = np.array([[-5.0, -1.5, -1.0], [12.0, 1.5, 1.5]])
# pillars 0.5 m deep on alternating walls every 1.25 m: surfaces that face along the corridor, so the walk can be registered
CORRIDOR_BOXES = np.array([[[x, -1.5, -1.0], [x + 0.5, -0.9, 1.5]] if i % 2 else [[x, 0.9, -1.0], [x + 0.5, 1.5, 0.8]] for i, x in enumerate(np.arange(-4.5, 11.0, 1.25))])
WALK_FRAMES, WALK_RANGE, WINDOW_HALF, WINDOW_TURN, SCAN = 22, 3.5, np.deg2rad(70.0), np.deg2rad(20.0), 0.1
WALK_RINGS, WALK_COLUMNS = 8, 90
# |GPU pose - oracle pose|: the bars of tests/test_odometry_gpu.py (measured there once, x 10); per frame the arithmetic is the same
POSE_TOL_M, POSE_TOL_RAD = 6.5e-11, 1.1e-11


def walk_pose(t):
    T = np.eye(4)
    T[:3, 3] = [0.5 * t, 0.05 * np.sin(2.0 * t), 0.0]
    return T


def cast(origins, dirs, room, boxes):
    """Range of every ray to the nearest surface: the room from inside, the boxes from outside (slab method)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / dirs
        best = np.min(np.maximum((room[0] - origins) * inv, (room[1] - origins) * inv), axis=1)
        for lo_c, hi_c in boxes:
            t0, t1 = (lo_c - origins) * inv, (hi_c - origins) * inv
            near, far = np.max(np.minimum(t0, t1), axis=1), np.min(np.maximum(t0, t1), axis=1)
            hit = (near <= far) & (near > 0.0)
            best = np.where(hit & (near < best), near, best)
    return best


def spinner_scan(f, pose, room, boxes, rings, columns, elevation_deg, max_range=None, window=None):
    """One revolution: ``(points (n, 3) in the sensor frame, times (n,))``, every column cast from where the sensor is at its time;
    returns beyond ``max_range`` and columns further than ``window[1]`` from the azimuth ``window[0]`` are dropped"""
    az = 2.0 * np.pi * np.arange(columns) / columns
    el = np.deg2rad(np.linspace(-elevation_deg, elevation_deg, rings))
    t_col = np.arange(columns) * (SCAN / columns)
    pts, times = [], []
    for j in range(columns):
        if window is not None and abs((az[j] - window[0] + np.pi) % (2.0 * np.pi) - np.pi) > window[1]:
            continue
        T = pose(f * SCAN + t_col[j])
        d = np.stack([np.cos(el) * np.cos(az[j]), np.cos(el) * np.sin(az[j]), np.sin(el)], axis=1)
        r = cast(np.tile(T[:3, 3], (rings, 1)), d @ T[:3, :3].T, room, boxes)
        keep = np.ones(rings, dtype=bool) if max_range is None else r <= max_range
        pts.append((d * r[:, None])[keep])
        times.append(np.full(int(keep.sum()), t_col[j]))
    return np.concatenate(pts), np.concatenate(times)


def pose_delta(A, B):
    D = se3.pose3_inverse(A) @ B
    return float(np.linalg.norm(D[:3, 3])), float(np.linalg.norm(se3.rot3_logmap(D[:3, :3])))


def walk_scans():
    return [spinner_scan(f, walk_pose, CORRIDOR, CORRIDOR_BOXES, WALK_RINGS, WALK_COLUMNS, 35.0, WALK_RANGE, (f * WINDOW_TURN, WINDOW_HALF)) for f in range(WALK_FRAMES)]


def test_scan_matcher_over_a_model_that_forgets_follows_the_oracle():
    scans = walk_scans()
    dev = odometry.DeviceBackend(0, max_blocks=1024, lru_thresh=2, lru_cycle=2)
    cpu = lru.NumpyBackendLRU(lru_thresh=2, lru_cycle=2)
    gpu_matcher, cpu_matcher = odometry.ScanMatcher(dev, 10), odometry.ScanMatcher(cpu, 10)
    dm = dr = 0.0
    try:
        for f, (pts, times) in enumerate(scans):
            got, want = gpu_matcher.insert(pts, times), cpu_matcher.insert(pts, times)
            vox = dev.model_points()[0]
            assert {tuple(int(c) for c in v) for v in vox} == set(cpu.model.voxels), f  # the surviving voxel sets, exactly, after every frame
            assert_lru_equals(dev, cpu.model, passes=(f + 1) // 2 - (1 if f + 1 >= 2 else 0))
            for g, c in zip(got, want):
                dm, dr = max(dm, pose_delta(g, c)[0]), max(dr, pose_delta(g, c)[1])
        truth = walk_pose(WALK_FRAMES * SCAN)
        err = pose_delta(truth, gpu_matcher.last_end)
    finally:
        dev.close()
    # conditions on the input, which the oracle alone decides
    evicted = [(k, n) for e in cpu.model.evicted for k, n in e]
    first_left = {}
    for i, e in enumerate(cpu.model.evicted):
        for k, _ in e:
            first_left.setdefault(k, i)
    again = [k for i, c in enumerate(cpu.model.created) for k in c if k in first_left and first_left[k] < i]
    print(f"walk: |dpose| GPU-oracle {dm:.3e} m {dr:.3e} rad; final T_end error {err[0]:.4f} m {err[1]:.5f} rad; evicted {len(evicted)} voxels "
          f"({sum(n for _, n in evicted)} points), {len(again)} created again; iterations {gpu_matcher.iterations}")
    assert sum(1 for _, n in evicted if n > 0) >= 1 and len(again) >= 1
    assert dm <= POSE_TOL_M and dr <= POSE_TOL_RAD


# ---- 11. the command line ---------------------------------------------------------------------------------------------------------------------
ROOM = np.array([[-10.0, -8.0, -1.5], [10.0, 8.0, 3.0]])
BOXES = np.array([[[3.0, 2.0, -1.5], [5.0, 4.0, 1.0]], [[-6.0, -5.0, -1.5], [-4.0, -2.0, 2.0]], [[-3.0, 4.0, -1.5], [0.0, 6.0, 0.5]]])
SPINNER = np.dtype({"names": ["x", "y", "z", "intensity", "t"], "formats": ["<f4", "<f4", "<f4", "<f4", "<f4"], "offsets": [0, 4, 8, 12, 16], "itemsize": 20})
ARGS = ["--image_topic", "/camera/image", "--points_topic", "/points", "--camera_model", "plumb_bob", "--camera_intrinsics", "60,60,32,24", "--camera_distortion_coeffs", "0,0,0,0,0",
        "--voxel_resolution", "0.02", "--min_distance", "0.5", "--target_num_points", "1000"]


def room_pose(t):
    T = np.eye(4)
    c, s = np.cos(0.2 * t), np.sin(0.2 * t)
    T[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [0.5 * t, 0.0, 0.0]
    return T


def test_the_default_threshold_changes_nothing_on_a_bag_of_twelve_frames(tmp_path, capsys):
    """With the default of 100 nothing can leave before insert 110: ``--lru_thresh 0`` and the default write the same directory"""
    src = tmp_path / "bags"
    src.mkdir()
    image = (np.random.default_rng(3).integers(0, 256, size=(48, 64))).astype(np.uint8)
    msgs = [(0, (50, 0), fx.image((50, 0), image, "mono8"))]
    for f in range(12):
        pts, times = spinner_scan(f, room_pose, ROOM, BOXES, 8, 256, 15.0)
        rec = np.zeros(pts.shape[0], dtype=SPINNER)
        rec["x"], rec["y"], rec["z"], rec["t"], rec["intensity"] = pts[:, 0], pts[:, 1], pts[:, 2], times, 40.0 + 100.0 * np.abs(np.sin(np.arange(pts.shape[0])))
        stamp = (100 + (f * 100000000) // 1000000000, (f * 100000000) % 1000000000)
        msgs.append((1, stamp, fx.cloud_from_struct(stamp, rec)))
    fx.write_bag(src / "run.bag", [(0, "/camera/image", "sensor_msgs/Image"), (1, "/points", "sensor_msgs/PointCloud2")], msgs, chunk_size=4, index=True)
    assert preprocess_dynamic.main([str(src), str(tmp_path / "default")] + ARGS) == 0
    assert preprocess_dynamic.main([str(src), str(tmp_path / "off"), "--lru_thresh", "0"] + ARGS) == 0
    names = sorted(os.listdir(tmp_path / "default"))
    assert names == sorted(os.listdir(tmp_path / "off")) and "run.bag.ply" in names and "calib.json" in names
    match, mismatch, errors = filecmp.cmpfiles(tmp_path / "default", tmp_path / "off", names, shallow=False)
    assert sorted(match) == names and not mismatch and not errors
    assert os.path.getsize(tmp_path / "default" / "run.bag.ply") > 100000
    capsys.readouterr()
    assert preprocess_dynamic.main([str(src), str(tmp_path / "bad"), "--lru_thresh", "-1"] + ARGS) == 1
    assert "--lru_thresh -1" in capsys.readouterr().err and not os.path.exists(tmp_path / "bad" / "run.bag.ply")
