"""CPU tests of the host side of the dynamic integrator (odometry.py, the Pose3 helpers of se3.py, TimeKeeper.process_times, the
preprocess_dynamic command line).  No GPU: the device side is tests/test_odometry_gpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import odometry_oracle as oracle  # noqa: E402
from direct_visual_lidar_calibration_amd import odometry, preprocess, preprocess_dynamic, preprocess_ros1, se3  # noqa: E402

AXIS = np.array([1.0, 2.0, -1.0]) / np.sqrt(6.0)
XIS = {
    "zero_rotation": np.r_[0.0, 0.0, 0.0, 0.3, -0.2, 0.1],
    "tiny_rotation": np.r_[1e-9, 0.0, 0.0, 0.3, -0.2, 0.1],
    "series_edge": np.r_[6e-5, 8e-5, 0.0, 0.3, -0.2, 0.1],
    "generic": np.r_[0.4, -0.7, 0.2, 1.0, 2.0, -0.5],
    "near_pi": np.r_[AXIS * (np.pi - 0.05), 0.3, 0.2, 0.1],
}
H = 1e-6
# central differences with step 1e-6 of functions whose third derivatives are O(1) (O(1 / 0.05^2) next to pi): truncation h^2 / 6 times
# that, rounding 1e-16 / h
TOL = {"zero_rotation": 1e-8, "tiny_rotation": 1e-8, "series_edge": 1e-8, "generic": 1e-8, "near_pi": 1e-6}


def local(T, T2):
    return se3.pose3_logmap(se3.pose3_inverse(T) @ T2)


def numeric(f, at, n=6):
    """d Logmap(f(at)^-1 f(at + d)) / d d by central differences; ``f`` takes the 6-vector perturbation"""
    J = np.zeros((6, n))
    for i in range(n):
        d = np.zeros(n)
        d[i] = H
        J[:, i] = (local(at, f(d)) - local(at, f(-d))) / (2.0 * H)
    return J


@pytest.mark.parametrize("name", list(XIS))
def test_expmap_and_logmap_derivatives_match_central_differences(name):
    xi = XIS[name]
    T, J = se3.pose3_expmap_with_derivative(xi)
    assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-12)
    assert np.allclose(se3.pose3_logmap(T), xi, atol=1e-8 if name == "near_pi" else 1e-12)
    assert np.allclose(T, se3.pose3_expmap(xi), atol=1e-12)  # the same map as the helper the Nelder-Mead path uses
    assert np.abs(J - numeric(lambda d: se3.pose3_exp(xi + d), T)).max() < TOL[name]
    JL = se3.pose3_logmap_derivative(xi)
    num = np.zeros((6, 6))
    for i in range(6):
        d = np.zeros(6)
        d[i] = H
        num[:, i] = (se3.pose3_logmap(T @ se3.pose3_exp(d)) - se3.pose3_logmap(T @ se3.pose3_exp(-d))) / (2.0 * H)
    assert np.abs(JL - num).max() < TOL[name] * (100.0 if name == "near_pi" else 1.0)  # (Logmap's own curvature next to pi)
    assert np.allclose(JL @ J, np.eye(6), atol=1e-9)


def test_between_and_compose_jacobians_match_central_differences():
    A, B = se3.pose3_exp(XIS["generic"]), se3.pose3_exp(np.r_[-0.3, 0.2, 0.9, -1.0, 0.5, 2.0])
    D, H1, H2 = se3.pose3_between(A, B)
    assert np.allclose(D, np.linalg.inv(A) @ B)
    assert np.abs(H1 - numeric(lambda d: se3.pose3_between(se3.pose3_retract(A, d), B)[0], D)).max() < 1e-8
    assert np.abs(H2 - numeric(lambda d: se3.pose3_between(A, se3.pose3_retract(B, d))[0], D)).max() < 1e-8
    C, G1, G2 = se3.pose3_compose(A, B)
    assert np.abs(G1 - numeric(lambda d: se3.pose3_compose(se3.pose3_retract(A, d), B)[0], C)).max() < 1e-8
    assert np.abs(G2 - numeric(lambda d: se3.pose3_compose(A, se3.pose3_retract(B, d))[0], C)).max() < 1e-8


@pytest.mark.parametrize("case", ["generic", "identical_poses", "tiny_motion"])
def test_pose_derivatives_of_update_poses_match_central_differences(case):
    T0 = se3.pose3_exp(np.r_[0.1, -0.2, 0.3, 1.0, -2.0, 0.5])
    delta = {"generic": np.r_[0.02, -0.01, 0.03, 0.05, 0.01, -0.02], "identical_poses": np.zeros(6), "tiny_motion": np.r_[1e-9, 0.0, 0.0, 1e-9, 0.0, 0.0]}[case]
    T1 = T0 @ se3.pose3_exp(delta)
    table = np.array([0.0, 0.37, 1.0])
    poses, d0, d1 = odometry.update_poses(T0, T1, table)
    for i, t in enumerate(table):
        assert np.allclose(poses[i], T0 @ se3.pose3_exp(t * delta), atol=1e-12)
        n0 = numeric(lambda d: odometry.update_poses(se3.pose3_retract(T0, d), T1, table, derivatives=False)[0][i], poses[i])
        n1 = numeric(lambda d: odometry.update_poses(T0, se3.pose3_retract(T1, d), table, derivatives=False)[0][i], poses[i])
        assert np.abs(d0[i] - n0).max() < 1e-7 and np.abs(d1[i] - n1).max() < 1e-7
    assert np.allclose(d0[0], np.eye(6), atol=1e-12) and np.allclose(d1[0], 0.0, atol=1e-12)  # t = 0: pose 0 itself
    assert np.allclose(d0[2], 0.0, atol=1e-7) and np.allclose(d1[2], np.eye(6), atol=1e-7)  # t = 1: pose 1 itself
    packed = odometry.pack_poses(poses, d0, d1)
    assert packed.shape == (3, 84) and np.array_equal(packed[1, :9], poses[1][:3, :3].reshape(9)) and np.array_equal(packed[1, 48:], d1[1].reshape(36))


def test_interpolate_rt_meets_both_ends():
    A, B = se3.pose3_exp(XIS["generic"]), se3.pose3_exp(np.r_[-0.3, 0.2, 0.9, -1.0, 0.5, 2.0])
    assert np.allclose(se3.pose3_interpolate_rt(A, B, 0.0), A, atol=1e-15) and np.allclose(se3.pose3_interpolate_rt(A, B, 1.0), B, atol=1e-12)
    mid = se3.pose3_interpolate_rt(A, B, 0.5)
    assert np.allclose(mid[:3, 3], 0.5 * (A[:3, 3] + B[:3, 3])) and np.allclose(mid[:3, :3] @ mid[:3, :3].T, np.eye(3), atol=1e-12)


def test_time_table_groups_by_time_eps_and_normalises():
    table, idx = odometry.time_table(np.array([0.0, 0.0005, 0.001, 0.0011, 0.0030, 0.1]))
    assert idx.tolist() == [0, 0, 0, 1, 2, 3] and np.allclose(table, np.array([0.0, 0.0011, 0.003, 0.1]) / 0.1)
    table, idx = odometry.time_table(np.zeros(4))
    assert idx.tolist() == [0, 0, 0, 0] and table.tolist() == [0.0]


# ---- the time keeper's affine map against the oracle's full per-point column, one case per branch of replace_points_stamp
def _frames(case):
    n = 7
    rel = np.linspace(0.0, 0.09, n)
    if case == "relative":
        return [(100.0 + 0.1 * f, rel.copy(), 1.0) for f in range(3)]
    if case == "absolute_near_stamp":
        return [(1700000000.0 + 0.1 * f, 1700000000.02 + 0.1 * f + rel, 1.0) for f in range(3)]
    if case == "absolute_far_from_stamp":
        return [(1700000000.0 + 0.1 * f, 5000.0 + 0.1 * f + rel, 1.0) for f in range(3)]
    if case == "livox_nanoseconds":
        return [(1700000000.0 + 0.1 * f, (1700000000.0 + 0.1 * f + rel) * 1e9 * 1e9, 1.0) for f in range(2)]  # > 1e16 after the column's own unit
    if case == "negative":
        return [(100.0 + 0.1 * f, rel - 0.03, 1.0) for f in range(2)]
    if case == "uint32_nanoseconds":
        return [(100.0 + 0.1 * f, (rel * 1e9).astype(np.uint32), 1e-9) for f in range(2)]
    if case == "no_time_field":
        return [(100.0 + 0.1 * f, None, 1.0) for f in range(4)]
    raise AssertionError(case)


@pytest.mark.parametrize("case", ["relative", "absolute_near_stamp", "absolute_far_from_stamp", "livox_nanoseconds", "negative", "uint32_nanoseconds", "no_time_field"])
def test_process_times_map_reproduces_the_oracles_per_point_times(case):
    keeper, plain, ref = preprocess.TimeKeeper(log=lambda m: None), preprocess.TimeKeeper(log=lambda m: None), oracle.TimeKeeperOracle()
    n = 7
    for stamp, raw, raw_scale in _frames(case):
        if raw is None:
            keep, scale, shift = keeper.process_times(stamp)
            assert plain.process(stamp) == keep
            _, want = ref.replace(stamp, None, n)
            got = (scale * np.arange(n, dtype=np.float64)) / n
            assert np.array_equal(got, want)
        else:
            col = raw.astype(np.float64) / 1e9 if raw.dtype == np.uint32 else raw.astype(np.float64)  # extract_raw_points: uint32 is nanoseconds
            keep, scale, shift = keeper.process_times(stamp, col[0], col[-1], lambda: col.min(), raw_scale=raw_scale)
            assert plain.process(stamp, col[0], col[-1], lambda: col.min()) == keep
            want_stamp, want = ref.replace(stamp, col, n)
            got = raw.astype(np.float64) * scale + shift
            # one affine map of the raw column against the reference's chain of subtractions: a few roundings of the largest
            # intermediate, max(|raw * scale|, |shift|) * 2^-52 each
            bound = 4.0 * 2.0**-52 * max(np.abs(raw.astype(np.float64) * scale).max(), abs(shift), 1.0)
            assert np.abs(got - want).max() <= bound, (np.abs(got - want).max(), bound)
            assert keeper.stamp == plain.stamp == want_stamp
        assert keep
    assert keeper.last_points_stamp == plain.last_points_stamp  # process itself is untouched by the new method


def test_process_times_first_frame_without_times_is_all_zero():
    keeper = preprocess.TimeKeeper(log=lambda m: None)
    assert keeper.process_times(5.0) == (True, 0.0, 0.0)
    assert keeper.process_times(5.1)[1] == pytest.approx(0.1)
    assert keeper.process_times(5.0)[0] is False  # a rewinding stamp is still refused


# ---- sampling
def test_randomgrid_sampling_rules():
    rng = np.random.Generator(np.random.MT19937(0))
    pts = np.random.default_rng(1).uniform(-4.0, 4.0, size=(6000, 3))
    pts[:2000] = pts[:2000] * 0.05 + 1.2  # one crowded cell
    rate = 0.1
    idx = odometry.randomgrid_sampling(pts, 0.5, rate, rng)
    cells = np.floor(pts / 0.5).astype(np.int64)
    n_vox = np.unique(cells, axis=0).shape[0]
    quota = int(np.ceil(rate * 6000 / n_vox))
    assert np.all(np.diff(idx) > 0) and idx.dtype == np.int64  # sorted, no duplicates
    _, counts = np.unique(cells[idx], axis=0, return_counts=True)
    assert counts.max() <= quota and idx.shape[0] <= int(6000 * rate * 1.2)
    # the cap: few cells, so every cell fills its quota and the total exceeds 1.2 rate n
    flat = np.random.default_rng(2).uniform(0.0, 0.999, size=(1000, 3)) + np.array([[0.0, 0.0, 0.0]]) + np.repeat(np.arange(3.0), 334)[:1000, None] * np.array([[0.5, 0.0, 0.0]])
    idx = odometry.randomgrid_sampling(flat, 0.5, 0.0101, rng)
    assert idx.shape[0] == int(1000 * 0.0101 * 1.2) and np.all(np.diff(idx) > 0)
    assert np.array_equal(odometry.randomgrid_sampling(pts, 0.5, 0.99, rng), np.arange(6000))
    assert np.array_equal(odometry.randomgrid_sampling(pts, 0.5, 5.0, rng), np.arange(6000))
    a = odometry.randomgrid_sampling(pts, 0.5, rate, np.random.Generator(np.random.MT19937(3)))
    b = odometry.randomgrid_sampling(pts, 0.5, rate, np.random.Generator(np.random.MT19937(3)))
    assert np.array_equal(a, b)  # a seed fixes the draw


def test_sort_and_sample_is_a_stable_sort_by_time():
    times = np.array([0.2, 0.0, 0.2, 0.1, 0.0])
    order, sampled = odometry.sort_and_sample(np.zeros((5, 3)), times, 10000, np.random.Generator(np.random.MT19937(0)))
    assert order.tolist() == [1, 4, 3, 0, 2] and sampled.tolist() == [0, 1, 2, 3, 4]


# ---- the optimiser
def test_levenberg_marquardt_on_a_fixed_quadratic():
    A = np.diag([1.0, 10.0, 100.0]) + 0.5
    b = np.array([1.0, -2.0, 3.0])
    xs = np.linalg.solve(A, b)
    f = lambda x: 0.5 * x @ A @ x - b @ x  # noqa: E731
    calls = []

    def linearize(x):
        calls.append(x.copy())
        return A, A @ x - b, f(x)

    x, e, its = odometry.levenberg_marquardt(np.zeros(3), linearize, f, lambda x, d: x + d)
    # lambda = 1e-5 against eigenvalues >= 1: the first step lands within 1e-5 of the minimiser, the second finds no decrease > 1e-5
    assert np.abs(x - xs).max() < 1e-4 and its == 2 and len(calls) == 2 and e == pytest.approx(f(xs), abs=1e-8)
    # a model that over-promises (the true error rises): lambda grows past its upper bound and the start is returned
    x, e, its = odometry.levenberg_marquardt(np.ones(3), lambda x: (np.eye(3) * 1e-9, np.ones(3), 0.0), lambda x: 1.0, lambda x, d: x + d)
    assert np.array_equal(x, np.ones(3)) and e == 0.0 and its == 1


# ---- the command line
def test_preprocess_dynamic_parser_defaults():
    args = preprocess_dynamic.build_parser().parse_args(["bags", "dst"])
    assert (args.k_neighbors, args.target_num_points, args.seed) == (20, 10000, 0)
    assert (args.voxel_resolution, args.min_distance, args.device, args.intensity_channel, args.camera_model) == (0.002, 1.0, 0, "auto", "auto")
    args = preprocess_dynamic.build_parser().parse_args(["bags", "dst", "-a", "--k_neighbors", "10", "--target_num_points", "2000", "--seed", "7", "-d"])
    assert (args.k_neighbors, args.target_num_points, args.seed, args.auto_topic) == (10, 2000, 7, True)
    assert preprocess_dynamic.main([]) == 0  # the usage


def test_preprocess_dynamic_refuses_bad_options_before_touching_a_bag(tmp_path, capsys):
    assert preprocess_dynamic.main([str(tmp_path), str(tmp_path / "out"), "--k_neighbors", "40"]) == 1
    assert "k_neighbors" in capsys.readouterr().err
    assert preprocess_dynamic.main([str(tmp_path), str(tmp_path / "out")]) == 1  # an empty directory, as preprocess_ros1
    assert "no input bags" in capsys.readouterr().err and not (tmp_path / "out").exists()


def test_preprocess_ros1_still_refuses_dynamic_integration(tmp_path, capsys):
    assert preprocess_ros1.main([str(tmp_path), str(tmp_path / "out"), "-d"]) == 1
    err = capsys.readouterr().err
    assert "dynamic LiDAR integration" in err and "preprocess_dynamic" in err and not (tmp_path / "out").exists()


# ---- the oracle's own pins (tests/odometry_oracle.py is the yardstick of the GPU tests) ----------------------------------------------
def test_oracle_knn_orders_by_distance_then_index_under_ties():
    """A shuffled 5 x 5 x 3 integer lattice, k = 8: exact distances, so ties are true ties, at the k / k + 1 boundary too; a partition
    before the sort (the earlier oracle) kept an arbitrary subset of a tied boundary group and differed here in 35 of 75 rows"""
    g = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    pts = g[np.random.default_rng(0).permutation(75)]
    nbr, dist = oracle.knn(pts, 8)
    assert nbr.shape == (75, 8) and nbr.dtype == np.int32 and dist.shape == (75, 9)
    tied = 0
    for i in range(75):
        d = [float(np.sum((pts[j] - pts[i]) ** 2)) for j in range(75)]
        order = sorted(range(75), key=lambda j: (d[j], j))
        assert nbr[i].tolist() == order[:8] and dist[i].tolist() == [d[j] for j in order[:9]]
        tied += d[order[7]] == d[order[8]]
    assert tied >= 19  # a tie decides the set in a quarter of the rows at least
    nbr, dist = oracle.knn(pts[:8], 8)  # m == k: everything, and no next distance
    assert np.array_equal(np.sort(nbr, axis=1), np.tile(np.arange(8), (8, 1))) and np.all(np.isinf(dist[:, 8]))


def test_oracle_hash_is_splitmix64_and_home_slot_takes_the_packed_key_plus_one():
    assert oracle.vox_mix(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF  # splitmix64's first output from seed 0
    assert oracle.vox_mix(0) == 0 and oracle.vox_mix((1 << 64) + 5) == oracle.vox_mix(5)
    key = int(oracle.pack_key((3, -2, 7))) + 1
    assert key == ((3 + (1 << 20)) | ((-2 + (1 << 20)) << 21) | ((7 + (1 << 20)) << 42)) + 1
    assert oracle.home_slot((3, -2, 7), 1023) == oracle.vox_mix(key) & 1023 and oracle.home_slot((3, -2, 7), (1 << 25) - 1) == oracle.vox_mix(key) & ((1 << 25) - 1)
    homes = [oracle.home_slot(v, 1023) for v in np.ndindex(12, 12, 12)]
    assert min(homes) >= 0 and max(homes) <= 1023 and len(set(homes)) > 800  # spread over the table


def test_oracle_nearest_honours_the_resolution_and_never_packs_a_voxel_outside_the_key_range(monkeypatch):
    top = 2.0**20
    packed = []
    real = oracle.pack_key
    monkeypatch.setattr(oracle, "pack_key", lambda v: packed.append(np.stack([np.asarray(c, dtype=np.int64) for c in v])) or real(v))
    for res in (1.0, 0.5, 0.3):
        ivox = oracle.IVox(resolution=res, insertion_dist_thresh=0.01)
        model = np.array([[top - 0.25, 0.5, 0.5], [-top + 0.25, 0.5, 0.5], [0.5, 0.5, 0.5], [1.25, 2.5, 0.5]]) * res
        ivox.insert(model, np.ones((4, 6)))
        assert sorted(ivox.voxels) == sorted([(2**20 - 1, 0, 0), (-(2**20), 0, 0), (0, 0, 0), (1, 2, 0)])  # floor(p / res)
        q = np.array([[top - 0.75, 0.5, 0.5], [top + 0.5, 0.5, 0.5], [top + 1.5, 0.5, 0.5], [-top - 0.5, 0.5, 0.5], [-top - 1.5, 0.5, 0.5], [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5],
                      [0.75, 2.5, 0.5], [1.25, 3.5, 0.5], [0.75, 3.5, 0.5]]) * res  # the last three: the -x face neighbour, the -y one, an edge-diagonal voxel
        index, dist = ivox.nearest(q)
        _, pts, _ = ivox.flat()
        assert (index >= 0).tolist() == [True, True, False, True, False, False, False, True, True, False]
        assert np.array_equal(pts[index[[0, 1, 3, 7, 8]]], model[[0, 0, 1, 3, 3]])
        assert np.allclose(dist[[0, 1, 3]], np.array([0.25, 0.5625, 0.5625]) * res * res, rtol=1e-9, atol=0.0) and np.all(dist[index < 0] == oracle.DBL_MAX)
    every = np.concatenate([p.reshape(3, -1) for p in packed], axis=1)
    assert every.min() >= -(2**20) and every.max() < 2**20


def test_the_eigen_fixture_regenerates_identically():
    import make_odometry_golden as golden

    stored = np.load(golden.PATH)
    assert os.path.getsize(golden.PATH) < 64 * 1024 and stored["k"].max() <= golden.MAX_POINTS and 24 <= stored["names"].shape[0] <= 48
    cases = golden.build_cases()  # the inputs need numpy only: always compared
    assert [c[0] for c in cases] == stored["names"].tolist() and [c[1] for c in cases] == stored["groups"].tolist()
    for i, (_, _, pts, lst) in enumerate(cases):
        k = pts.shape[0]
        assert np.array_equal(stored["points"][i, :k], pts) and np.array_equal(stored["lists"][i, :k], lst) and stored["k"][i] == k
    try:
        import mpmath  # noqa: F401
    except ImportError:
        pytest.skip("mpmath is not installed: the exact normals of tests/golden/odometry_eigen_cases.npz are not regenerated here")
    fresh = golden.generate()
    assert sorted(fresh) == sorted(stored.files)
    for name in stored.files:
        assert np.array_equal(fresh[name], stored[name]), name
