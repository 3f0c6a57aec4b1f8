"""CPU tests of the LRU eviction's yardstick (tests/odometry_lru_oracle.py: ``IVoxLRU``, a restatement of ivox.cpp:144-178 and :223)
and of the command line's ``--lru_thresh``.  No GPU: the device side is tests/test_odometry_lru_gpu.py, which also holds the tests of
``nidreg_odom_set_lru`` / ``nidreg_odom_lru_info`` -- a handle cannot be created without a device."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import odometry_lru_oracle as lru  # noqa: E402
import odometry_oracle as oracle  # noqa: E402
from direct_visual_lidar_calibration_amd import preprocess_dynamic  # noqa: E402


def covs_for(n):
    return np.tile(np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0]), (n, 1))


def test_the_oracle_follows_the_hand_worked_schedule():
    """lru_thresh = 2, lru_cycle = 3, six inserts; voxels named by their x index (they lie 3 m apart: a search in one finds no other).
    The voxels that exist after each INSERT, worked by hand from ivox.cpp:169-178:

      1  A B H enter (stamps 1)                                        horizon -1           {0, 3, 6}
      2  C enters (2)                                                  horizon  0: no pass  {0, 3, 6, 9}
      3  D enters (3)                                                  horizon  1, 3 % 3 == 0: the pass runs; A, B, H are stamped 1,
                                                                       exactly the horizon, and stay                {0, 3, 6, 9, 12}
      4  E enters (4); a point 3 cm from A's is refused, A restamped 4 horizon  2, B and H are stale, but 4 % 3 != 0 {0, 3, 6, 9, 12, 15}
         a search in B's voxel restamps B (4)
      5  F enters (5)                                                  horizon  3, H and C are stale, 5 % 3 != 0    {0, 3, 6, 9, 12, 15, 18}
      6  G enters (6)                                                  horizon  4, 6 % 3 == 0: H (1), C (2), D (3) leave; A (4, by
                                                                       the refused point), B (4, by the search) and E (4) sit at the
                                                                       horizon and stay                             {0, 3, 15, 18, 21}
    """
    after_insert = [{0, 3, 6}, {0, 3, 6, 9}, {0, 3, 6, 9, 12}, {0, 3, 6, 9, 12, 15}, {0, 3, 6, 9, 12, 15, 18}, {0, 3, 15, 18, 21}]
    assert [s[2] for s in lru.RULE_EDGES if s[0] == "insert"] == after_insert  # (the schedule the GPU test runs is this one)
    ivox = lru.IVoxLRU(lru_thresh=lru.RULE_EDGES_THRESH, lru_cycle=lru.RULE_EDGES_CYCLE)
    assert (ivox.lru_thresh, ivox.lru_cycle) == (2, 3)
    for kind, pts, want in lru.RULE_EDGES:
        pts = np.array(pts)
        if kind == "insert":
            ivox.insert(pts, covs_for(pts.shape[0]))
        else:
            index, dist = ivox.nearest(pts)
            assert index[0] >= 0 and abs(dist[0] - 0.01) < 1e-12  # B's point, 10 cm away
        assert {k[0] for k in ivox.voxels} == want and all(k[1:] == (0, 0) for k in ivox.voxels)
    assert ivox.lru_count == 6
    assert [len(e) for e in ivox.evicted] == [0, 0, 0, 0, 0, 3] and sorted(k[0] for k, _ in ivox.evicted[5]) == [6, 9, 12]
    assert ivox.stamps == {(0, 0, 0): 4, (3, 0, 0): 4, (15, 0, 0): 4, (18, 0, 0): 5, (21, 0, 0): 6}
    assert ivox.flat()[1].shape[0] == lru.RULE_EDGES_POINTS_AT_END and len(ivox.voxels[(0, 0, 0)][0]) == 1  # the refused point never entered


def test_without_the_refreshes_the_same_voxels_leave():
    """The schedule again without the refused point and without the search: A and B then leave with the others"""
    ivox = lru.IVoxLRU(lru_thresh=2, lru_cycle=3)
    for kind, pts, _ in lru.RULE_EDGES:
        if kind == "insert":
            pts = np.array(pts[:1] if len(pts) == 2 else pts)
            ivox.insert(pts, covs_for(pts.shape[0]))
    assert {k[0] for k in ivox.voxels} == {15, 18, 21}


def test_a_search_stamps_only_present_face_neighbours_inside_the_key_range():
    ivox = lru.IVoxLRU(lru_thresh=5, lru_cycle=1)
    L = oracle.AXIS_LIMIT
    pts = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [1.5, 1.5, 0.5], [L - 0.5, 0.5, 0.5], [40.5, 0.5, 0.5]])
    ivox.insert(pts, covs_for(5))
    ivox.insert(np.array([[90.5, 0.5, 0.5]]), covs_for(1))
    q = np.array([[0.6, 0.5, 0.5],  # finds (0,0,0) and its face neighbour (1,0,0); (1,1,0) is diagonal
                  [L - 0.4, 0.5, 0.5],  # its +x neighbour lies outside the key range: skipped, not looked up
                  [np.nan, 0.0, 0.0], [41.5, 0.5, 3.5]])  # a non-finite query and one with no neighbour stamp nothing
    index, _ = ivox.nearest(q)
    assert index[0] >= 0 and index[1] >= 0 and index[2] == -1 and index[3] == -1
    assert ivox.stamps == {(0, 0, 0): 2, (1, 0, 0): 2, (1, 1, 0): 1, (L - 1, 0, 0): 2, (40, 0, 0): 1, (90, 0, 0): 2}


def test_lru_thresh_zero_never_erases_and_equals_the_plain_oracle():
    rng = np.random.default_rng(2)
    a, b = lru.IVoxLRU(lru_thresh=0, lru_cycle=1), oracle.IVox()
    for i in range(5):
        pts = rng.uniform(0.0, 4.0, size=(30, 3)) + [10.0 * i, 0.0, 0.0]
        a.insert(pts, covs_for(30))
        b.insert(pts, covs_for(30))
    assert all(np.array_equal(x, y) for x, y in zip(a.flat(), b.flat())) and a.lru_count == 5 and not any(a.evicted)


def test_the_command_line_refuses_a_negative_lru_thresh(tmp_path, capsys):
    assert preprocess_dynamic.build_parser().parse_args(["a", "b"]).lru_thresh == 100  # the reference's iVox(1.0, 0.05, 100)
    assert preprocess_dynamic.main([str(tmp_path), str(tmp_path / "out"), "--lru_thresh", "-1"]) == 1
    assert "--lru_thresh -1" in capsys.readouterr().err
    assert "extension" in preprocess_dynamic.build_parser().format_help().split("--lru_thresh")[-1]  # the option's own help text
