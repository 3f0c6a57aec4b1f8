"""GPU tests of the dynamic integrator's device side (``nidreg_odom_*``, csrc/nid_odom_kernels.hpp) and of the preprocess_dynamic
command end to end.  The yardstick is the CPU restatement of tests/odometry_oracle.py -- written from the reference's sources -- and a
synthetic ground truth: the reference's own integrator cannot be compiled for these tests (it needs gtsam, PCL and ROS)."""
import numpy as np
import pytest

import odometry_oracle as oracle
import rosbag1_fixture as fx
from direct_visual_lidar_calibration_amd import dataset, odometry, preprocess, preprocess_dynamic, preprocess_ros1, se3

pytestmark = pytest.mark.gpu
EPS = 2.0**-53


@pytest.fixture(scope="module")
def backend():
    b = odometry.DeviceBackend(0)
    yield b
    b.close()


# ---- 1. kNN and covariances -------------------------------------------------------------------------------------------------------
def noisy_planes(m, seed):
    """Points on three planes a few metres from the origin, 1 mm of noise across them"""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-1.0, 1.0, size=(m, 2))
    which = rng.integers(0, 3, size=m)
    origins = np.array([[4.0, 0.0, 0.5], [0.0, -3.0, 1.0], [1.0, 2.0, -1.2]])
    frames = np.array([[[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]], [[1.0, 0.0, 0.2], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0], [0.0, 1.0, 0.1], [0.0, 0.0, 1.0]]])
    pts = origins[which] + uv[:, :1] * frames[which, 0] + uv[:, 1:] * frames[which, 1] + rng.normal(0.0, 1e-3, size=(m, 1)) * frames[which, 2]
    return np.ascontiguousarray(pts)


# |GPU - oracle| of the covariance entries and of the normals (up to sign) on these inputs, rows with an eigen-gap above 1e-6 lambda_2:
# measured once at 8.3e-15 (the largest over the cases below: the normals at M = 65, k = 20; the covariances there 7.9e-15); the bar
# is 10 x that.  A closed-form solver and LAPACK's iteration legitimately differ by more than rounding: the covariance of points 4 m
# from the origin carries ~1e-14 of cancellation error, against a smallest eigenvalue of 1e-6.
COV_TOL = 8.3e-14


@pytest.mark.parametrize("m,k", [(20, 20), (64, 20), (65, 20), (257, 20), (1025, 20), (257, 5)])
def test_knn_sets_normals_and_covariances_match_the_oracle(backend, m, k):
    pts = noisy_planes(m, 100 + m + k)
    want_nbr, dist = oracle.knn(pts, k)
    assert np.all(dist[:, k - 1] < dist[:, k])  # no tie decides a set (m == k: the next distance is inf)
    assert np.all(np.diff(dist[:, :k], axis=1) > 0) or m == k  # ... nor an order inside it
    nbr, normals, covs = backend.knn_covariances(pts, k)
    if m == k:
        assert np.array_equal(np.sort(nbr, axis=1), np.tile(np.arange(m, dtype=np.int32), (m, 1)))  # every point neighbours all
    assert np.array_equal(np.sort(nbr, axis=1), np.sort(want_nbr, axis=1))
    if np.all(np.diff(dist[:, :k], axis=1) > 0):
        assert np.array_equal(nbr, want_nbr)  # ascending (d^2, index)
    assert np.all(nbr[:, 0] == np.arange(m))  # itself first, at distance 0
    want_n, want_c, lam = oracle.covariances(pts, want_nbr)
    rows = (lam[:, 1] - lam[:, 0]) > 1e-6 * lam[:, 2]
    assert rows.mean() >= 0.98  # (oracle alone: these inputs stay under the 2 % cap)
    sign = np.sign(np.sum(normals * want_n, axis=1))[:, None]
    dn, dc = np.abs(normals * sign - want_n)[rows].max(), np.abs(covs - want_c)[rows].max()
    print(f"knn/cov m={m} k={k}: |dn|max {dn:.3e} |dcov|max {dc:.3e} rows {int(rows.sum())}/{m}")
    assert np.allclose(np.linalg.norm(normals, axis=1), 1.0, atol=1e-12)
    assert dn <= COV_TOL and dc <= COV_TOL
    # the second entry: the same covariances from the GIVEN lists, bit for bit
    n2, c2 = backend.covariances(pts, nbr)
    assert np.array_equal(n2, normals) and np.array_equal(c2, covs)


def test_knn_refuses_fewer_points_than_neighbours_and_bad_lists(backend):
    pts = noisy_planes(19, 1)
    with pytest.raises(ValueError, match="fewer points"):
        backend.knn_covariances(pts, 20)
    with pytest.raises(ValueError, match="k must lie"):
        backend.knn_covariances(pts, 33)
    bad = np.zeros((19, 5), dtype=np.int32)
    bad[3, 2] = 19
    with pytest.raises(ValueError, match="neighbour index"):
        backend.covariances(pts, bad)


def test_coincident_and_collinear_neighbourhoods_give_finite_output(backend):
    same = np.tile(np.array([[1.5, -2.0, 0.25]]), (24, 1))
    line = np.array([1.0, 2.0, 3.0])[None] + np.linspace(0.0, 1.0, 40)[:, None] * np.array([[0.6, 0.0, 0.8]])
    for pts in (same, line):
        nbr, normals, covs = backend.knn_covariances(np.ascontiguousarray(pts), 20)
        assert np.all(np.isfinite(normals)) and np.all(np.isfinite(covs)) and np.all((nbr >= 0) & (nbr < pts.shape[0]))
        assert np.allclose(np.linalg.norm(normals, axis=1), 1.0, atol=1e-12)
    _, normals, _ = backend.knn_covariances(np.ascontiguousarray(line), 20)
    assert np.abs(normals @ np.array([0.6, 0.0, 0.8])).max() < 1e-6  # orthogonal to the line


# ---- 2. the model -------------------------------------------------------------------------------------------------------------------
def covs_for(n, seed):
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(0.1, 1.0, size=(n, 6)))


def assert_model_equals(b, ivox):
    vox, pts, covs = b.model_points()
    keys, want_pts, want_covs = ivox.flat()
    assert np.array_equal(oracle.pack_key((vox[:, 0], vox[:, 1], vox[:, 2])), keys)  # every voxel, and how many points it holds
    assert np.array_equal(pts, want_pts) and np.array_equal(covs, want_covs)  # every voxel's ordered list
    info = b.model_info()
    assert info["points"] == keys.shape[0] and info["voxels"] == np.unique(keys).shape[0]


def test_model_insert_keeps_the_sequential_rule_exactly():
    b, ivox = odometry.DeviceBackend(0), oracle.IVox()
    try:
        pairs = np.array([[0.5, 0.5, 0.5], [0.549, 0.5, 0.5],  # 0.049 m apart: the second is refused
                          [3.5, 0.5, 0.5], [3.551, 0.5, 0.5],  # 0.051 m: both enter
                          [1.0, 0.2, 0.2], [-1.0, 0.2, 0.2], [-0.0, 0.2, 0.2], [-1e-300, 0.2, 0.2],  # voxels 1, -1, 0 and -1 (floor on negatives)
                          [0.999, 0.2, 0.2], [1.03, 0.2, 0.2]])  # 0.031 m apart across a voxel face: both enter (the test is per voxel)
        rng = np.random.default_rng(5)
        cloud = np.concatenate([pairs, rng.uniform(-3.0, 3.0, size=(700, 3)), rng.uniform(-3.0, 3.0, size=(300, 3)) * [1.0, 1.0, 0.01]])
        for frame, seed in ((cloud, 1), (cloud[::-1] + 0.02, 2)):  # the second frame: the same places, 3.5 cm off, in reverse order
            frame, covs = np.ascontiguousarray(frame), covs_for(frame.shape[0], seed)
            b.model_insert(frame, covs)
            ivox.insert(frame, covs)
            assert_model_equals(b, ivox)
        lists = ivox.lists()
        assert len(lists[(0, 0, 0)][0]) >= 2 and len(lists[(3, 0, 0)][0]) >= 2 and (-1, 0, 0) in lists and (1, 0, 0) in lists
    finally:
        b.close()


def test_model_insert_chains_a_second_and_third_block():
    b, ivox = odometry.DeviceBackend(0), oracle.IVox()
    try:
        g = np.stack(np.meshgrid(np.arange(9) * 0.1 + 0.05, np.arange(8) * 0.1 + 0.05, [0.2], indexing="ij"), axis=-1).reshape(-1, 3)[:65] + [7.0, -3.0, 2.0]
        assert np.unique(np.floor(g), axis=0).shape[0] == 1  # ONE voxel receives one point more than a block holds ...
        b.model_insert(np.ascontiguousarray(g), covs_for(65, 3))
        ivox.insert(g, covs_for(65, 3))
        assert_model_equals(b, ivox)
        assert b.model_info()["blocks"] == 2 and b.model_info()["points"] == 65
        later = np.concatenate([g[:64] + [0.0, 0.0, 0.3], g[:10] + [0.01, 0.0, 0.0]])  # ... then a second block's worth, and ten that are too close
        b.model_insert(np.ascontiguousarray(later), covs_for(74, 4))
        ivox.insert(later, covs_for(74, 4))
        assert_model_equals(b, ivox)
        assert b.model_info() == {"voxels": 1, "points": 129, "blocks": 3, "max_blocks": 1 << 18}
    finally:
        b.close()


def test_model_insert_refuses_a_key_outside_the_range_and_reports_an_exhausted_pool():
    b = odometry.DeviceBackend(0, max_blocks=2)
    try:
        ok = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5]])
        for bad in ([2.0**20 + 0.5, 0.0, 0.0], [0.0, -(2.0**20) - 0.5, 0.0], [0.0, np.nan, 0.0]):
            with pytest.raises(ValueError, match="packed-key limit"):
                b.model_insert(np.ascontiguousarray(np.concatenate([ok, [bad]])), covs_for(3, 0))
            assert b.model_info()["points"] == 0  # nothing was inserted
        b.model_insert(np.ascontiguousarray(ok), covs_for(2, 0))
        assert b.model_info()["points"] == 2 and b.model_info()["blocks"] == 2
        for _ in range(2):  # a third voxel needs a third block; a repeated call errors again
            with pytest.raises(odometry.ModelFullError, match="exhausted"):
                b.model_insert(np.array([[2.5, 0.5, 0.5]]), covs_for(1, 0))
            assert b.model_info() == {"voxels": 2, "points": 2, "blocks": 2, "max_blocks": 2}  # a voxel without a block is not in the table
        b.model_insert(np.array([[0.6, 0.5, 0.5]]), covs_for(1, 0))  # the voxels that have a block still take points
        assert b.model_info()["points"] == 3
    finally:
        b.close()


def test_more_new_voxels_than_free_blocks_in_one_call_is_an_error_not_a_hang_or_a_silent_drop():
    b = odometry.DeviceBackend(0, max_blocks=4)  # a table of 1024 slots
    try:
        g = np.stack(np.meshgrid(np.arange(40), np.arange(40), [0], indexing="ij"), axis=-1).reshape(-1, 3) + 0.5  # 1600 new voxels, more than slots
        for _ in range(2):
            with pytest.raises(odometry.ModelFullError, match="exhausted"):
                b.model_insert(np.ascontiguousarray(g), covs_for(1600, 0))
            info = b.model_info()
            assert info["voxels"] == info["points"] == info["blocks"] == 4  # four voxels got a block and their point; nothing else is in the table
        vox, pts, _ = b.model_points()
        assert pts.shape == (4, 3) and np.array_equal(np.floor(pts).astype(np.int32), vox)
        src = np.ascontiguousarray(np.concatenate([pts, g[:126]]) + 0.01)
        b.set_source(src, covs_for(130, 1) * [1.0, 0.0, 0.0, 1.0, 0.0, 1.0], np.zeros(130, dtype=np.int32))
        ident = odometry.pack_poses(np.eye(4)[None], np.zeros((1, 6, 6)), np.zeros((1, 6, 6)))
        assert b.linearize(ident)[121] >= 4  # the lookups end on a table that refused most of what it was offered
    finally:
        b.close()


# ---- 3. linearise and error ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lin_model():
    """A model of two noisy planes around the origin (negative coordinates included) and three lone points, on both sides"""
    rng = np.random.default_rng(11)
    uv = rng.uniform(-2.5, 2.5, size=(900, 2))
    wall = np.stack([uv[:450, 0], np.full(450, 1.3) + rng.normal(0, 2e-3, 450), uv[:450, 1]], axis=1)
    floor = np.stack([uv[450:, 0], uv[450:, 1], np.full(450, -0.7) + rng.normal(0, 2e-3, 450)], axis=1)
    lone = np.array([[-0.02, 20.5, 0.5],  # reached from voxel (0, 20, 0) across the face x = 0
                     [-0.01, 31.01, 0.5],  # voxel (-1, 31, 0): edge-diagonal to (0, 30, 0)
                     [40.5, 40.5, 40.5]])
    pts = np.ascontiguousarray(np.concatenate([wall, floor, lone]))
    b, ivox = odometry.DeviceBackend(0), oracle.IVox()
    _, _, covs = b.knn_covariances(pts, 10)
    b.model_insert(pts, covs)
    ivox.insert(pts, covs)
    yield b, ivox
    b.close()


def lin_case(ivox, m, k_entries, seed, unmatched=False):
    """m source points, their covariances, time indices and the packed pose table; the points are given where they must LAND"""
    rng = np.random.default_rng(seed)
    T0 = se3.pose3_exp(np.r_[0.02, -0.03, 0.05, 0.1, -0.05, 0.02])
    T1 = T0 @ se3.pose3_exp(np.r_[0.01, 0.02, -0.03, 0.04, 0.03, -0.01])
    table = np.linspace(0.0, 1.0, k_entries) if k_entries > 1 else np.array([0.0])
    poses, d0, d1 = odometry.update_poses(T0, T1, table)
    _, mpts, _ = ivox.flat()
    land = mpts[rng.integers(0, mpts.shape[0], size=m)] + rng.normal(0.0, 0.02, size=(m, 3))
    special = np.array([[50.0, 50.0, 50.0],  # nothing within 1 m
                        [0.03, 20.5, 0.5],  # its nearest lies across a negative voxel boundary
                        [0.01, 30.99, 0.5]])  # its only neighbour is in an edge-diagonal voxel: not found
    if unmatched:
        land = special[[0] * m] + rng.normal(0.0, 0.3, size=(m, 3))
    elif m >= 63:
        land[:3] = special
    else:
        land[0] = special[1]
    tidx = rng.integers(0, k_entries, size=m).astype(np.int32)
    P = poses[tidx]
    src = np.einsum("nji,nj->ni", P[:, :3, :3], land - P[:, :3, 3])  # R^T (q - t)
    covs = oracle.covariances(land, np.tile(np.arange(min(m, 3)), (m, 1)))[1] if m >= 3 else covs_for(m, seed) * [1.0, 0.0, 0.0, 1.0, 0.0, 1.0]
    return np.ascontiguousarray(src), np.ascontiguousarray(covs), tidx, odometry.pack_poses(poses, d0, d1), odometry.pack_poses(poses)


def assert_no_nearest_tie(ivox, q):
    _, mpts, _ = ivox.flat()
    mvox, centre = np.floor(mpts), np.floor(q)
    for i in range(q.shape[0]):
        near = np.abs(mvox - centre[i]).sum(axis=1) <= 1  # the 7 face-neighbour voxels
        d = np.sort(oracle.sq_dists(mpts[near], q[i]))
        assert d.shape[0] < 2 or d[0] < d[1]


@pytest.mark.parametrize("k_entries", [1, 3])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_linearize_and_error_match_the_oracle(lin_model, m, k_entries):
    b, ivox = lin_model
    src, covs, tidx, packed, packed12 = lin_case(ivox, m, k_entries, 1000 + m)
    want = oracle.linearize(src, covs, tidx, packed, ivox)
    q = np.stack(oracle._transform(packed[tidx], src, np.zeros((m, 3))), axis=1)
    assert_no_nearest_tie(ivox, q)
    b.set_source(src, covs, tidx)
    sums = b.linearize(packed)
    found, target, mahal = b.correspondences()
    assert np.array_equal(found, want["found"]) and np.array_equal(target, want["target"])  # correspondences are exact
    if m >= 63:
        assert found[:3].tolist() == [0, 1, 0] and np.array_equal(target[1], [-0.02, 20.5, 0.5])
    else:
        assert found[0] == 1 and np.array_equal(target[0], [-0.02, 20.5, 0.5])
    assert np.allclose(mahal.reshape(m, 9), want["mahal"], rtol=1e-9, atol=0.0)
    # every term is computed with the oracle's expression tree; what differs is the order of the sum: a wave's tree and the
    # partials in wave order against math.fsum -- each of at most m additions, 2^-53 relative each, of partial sums bounded by
    # the sum of the magnitudes; 4 m 2^-53 sum|terms| covers both orders with a factor of two to spare
    bound = 4.0 * m * EPS * want["abs"]
    print(f"linearize m={m} K={k_entries}: matched {int(sums[121])}, max |d| / bound {np.max(np.abs(sums - want['sums']) / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(np.abs(sums - want["sums"]) <= bound)
    assert sums[121] == found.sum() == want["sums"][121] and sums[121] >= m - 3
    assert np.array_equal(b.linearize(packed), sums)  # bit-identical from run to run
    err, matched = b.error(packed12)
    assert err == sums[120] and matched == int(sums[121])  # error() at the linearisation point IS the linearisation's error
    moved = packed12.copy()
    moved[:, 9:] += [0.01, -0.02, 0.005]
    want_err, want_abs, _ = oracle.error(src, tidx, moved, want["found"], want["target"], want["mahal"])
    err2, _ = b.error(moved)
    assert abs(err2 - want_err) <= 4.0 * m * EPS * want_abs and err2 != err


def test_an_all_unmatched_frame_gives_zeros(lin_model):
    b, ivox = lin_model
    src, covs, tidx, packed, packed12 = lin_case(ivox, 70, 3, 7, unmatched=True)
    assert oracle.linearize(src, covs, tidx, packed, ivox)["found"].sum() == 0
    b.set_source(src, covs, tidx)
    assert np.array_equal(b.linearize(packed), np.zeros(122))
    assert b.error(packed12) == (0.0, 0) and b.correspondences()[0].sum() == 0
    with pytest.raises(ValueError, match="time index"):
        b.linearize(packed[:1])  # the source refers to entries the table does not have


# ---- 4. deskewed insert ---------------------------------------------------------------------------------------------------------------
RES = 0.05
T_BEGIN = se3.pose3_exp(np.r_[0.02, -0.01, 0.3, 1.0, -0.5, 0.2])
T_END = T_BEGIN @ se3.pose3_exp(np.r_[0.01, 0.02, 0.15, 0.4, 0.1, -0.05])


def cloud_dtype(time_type, step):
    names, formats, offsets = ["x", "y", "z", "intensity"], ["<f4", "<f4", "<f4", "<f4"], [1, 5, 9, 13] if step == 29 else [0, 4, 8, 12]
    if time_type is not None:
        names, formats, offsets = names + ["t"], formats + [time_type], offsets + [offsets[-1] + 4]
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": step})


def make_cloud(n, time_type, step, seed, max_time=0.1):
    """``(message dict, float64 points, times [s], (time_field, scale, shift))``: random points, times in random order"""
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, dtype=cloud_dtype(time_type, step))
    xyz = rng.uniform(-8.0, 8.0, size=(n, 3)).astype(np.float32)
    rec["x"], rec["y"], rec["z"], rec["intensity"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], rng.uniform(0.0, 255.0, n).astype(np.float32)
    frac = rng.permutation(n) / max(1, n - 1)  # 0 and 1 both occur
    field = None
    if time_type == "<u4":
        rec["t"] = np.rint(frac * max_time * 1e9).astype(np.uint32)
        scale, times = 1e-9, rec["t"].astype(np.float64) * 1e-9
    elif time_type is not None:
        rec["t"] = (frac * max_time).astype(time_type)
        scale, times = 1.0, rec["t"].astype(np.float64)
    else:
        scale, times = max_time, (max_time * np.arange(n, dtype=np.float64)) / n
    if time_type is not None:
        field = (rec.dtype.fields["t"][1], fx.DATATYPE[time_type[1:]])
    msg = {"fields": [(k, rec.dtype.fields[k][1], fx.DATATYPE[rec.dtype.fields[k][0].str[1:]]) for k in rec.dtype.names], "point_step": step, "data": rec.tobytes(), "num_points": n,
           "is_bigendian": False}
    return msg, xyz.astype(np.float64), times, (field, scale, 0.0), rec


def records_by_seq(grid):
    rec = grid.get_records()
    return {int(s): rec[i] for i, s in enumerate(grid.last_seq)}


def test_deskew_insert_with_identity_poses_is_insert_cloud2_bit_for_bit():
    msg, _, times, (field, scale, shift), rec = make_cloud(5000, "<f4", 24, 21)
    rec = rec.copy()
    rec["x"][17], rec["y"][4000], rec["z"][4999] = np.nan, np.inf, -np.inf
    msg["data"] = rec.tobytes()
    a, b = preprocess.StaticPointCloudIntegrator(RES, 0.0), preprocess.StaticPointCloudIntegrator(RES, 0.0)
    try:
        for _ in range(2):  # two frames: the bases rise alike
            sa = a.insert_cloud2(msg, "intensity")
            sb = odometry.deskew_insert(b, preprocess.cloud2_layout(msg, "intensity"), "intensity", field, scale, shift, float(times.max()), np.eye(4), np.eye(4))
            assert sa == sb == 3
        ra, rb = a.get_records(), b.get_records()
        assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32)) and np.array_equal(a.last_seq, b.last_seq) and a.info() == b.info()
        assert a.last_seq.min() >= 5000  # the second frame's points overwrote the first's
    finally:
        a.close(), b.close()


@pytest.mark.parametrize("time_type,step,max_time", [("<u4", 24, 0.1), ("<f4", 29, 0.1), ("<f8", 29, 0.1), ("<f8", 32, 0.1), (None, 16, 0.1), ("<f4", 20, 0.0)])
def test_deskew_insert_moves_every_point_by_the_pose_of_its_time(time_type, step, max_time):
    n, min_distance = 3000, 2.0
    grid = preprocess.StaticPointCloudIntegrator(RES, min_distance)
    try:
        expected, base = {}, 0
        for seed in (31, 32):  # two frames with rising bases
            msg, pts, times, (field, scale, shift), rec = make_cloud(n, time_type, step, seed, max_time)
            rec = rec.copy()
            rec["y"][5] = np.nan
            pts[5, 1] = np.nan
            msg["data"] = rec.tobytes()
            tmax = float(times.max())
            moved = oracle.deskew(pts, times, tmax, T_BEGIN, T_END)
            cell = moved[np.all(np.isfinite(moved), axis=1)] / RES
            assert np.min(np.minimum(cell - np.floor(cell), np.ceil(cell) - cell)) * RES >= 1e-9  # no oracle coordinate near a cell face: none excluded
            norms = np.linalg.norm(moved, axis=1)
            assert np.nanmin(np.abs(norms - min_distance)) > 1e-9 and np.sum(norms < min_distance) > 5  # the gate acts, in the odometry frame ...
            assert np.sum((np.linalg.norm(pts, axis=1) >= min_distance) & (norms < min_distance)) > 0  # ... on points it would pass in the sensor frame
            skipped = odometry.deskew_insert(grid, preprocess.cloud2_layout(msg, "intensity"), "intensity", field, scale, shift, tmax, T_BEGIN, T_END)
            assert skipped == 1
            winners = oracle.voxel_winners(moved, RES, min_distance, base)
            expected.update({v: (s, moved[s - base], rec["intensity"][s - base]) for v, s in winners.items()})
            if tmax > 0.0:
                first, last = int(np.argmin(times)), int(np.argmax(times))
                assert times[first] == 0.0 and np.allclose(moved[first], T_BEGIN[:3, :3] @ pts[first] + T_BEGIN[:3, 3], atol=1e-12)
                assert np.allclose(moved[last], T_END[:3, :3] @ pts[last] + T_END[:3, 3], atol=1e-12)
            else:
                assert np.allclose(moved[6:], pts[6:] @ T_BEGIN[:3, :3].T + T_BEGIN[:3, 3], atol=1e-12)  # max_time = 0: every point at t = 0
            base += n
        got = records_by_seq(grid)
        assert sorted(got) == sorted(s for s, _, _ in expected.values())  # the voxel set, and every voxel's winner
        for s, p, inten in expected.values():
            want = p.astype(np.float32)
            assert np.all(np.abs(got[s][:3] - want) <= np.spacing(np.abs(want))) and got[s][3] == inten  # within 1 float32 ulp of the stored value
        assert grid.info()["offered"] == 2 * n
    finally:
        grid.close()


def test_deskew_insert_refuses_bad_arguments():
    msg, _, times, (field, scale, shift), _ = make_cloud(10, "<f4", 24, 1)
    grid = preprocess.StaticPointCloudIntegrator(RES, 0.0)
    try:
        layout = preprocess.cloud2_layout(msg, "intensity")
        with pytest.raises(ValueError, match="time field lies outside"):
            odometry.deskew_insert(grid, layout, "intensity", (22, 7), scale, shift, 0.1, np.eye(4), np.eye(4))
        with pytest.raises(ValueError, match="time field must be"):
            odometry.deskew_insert(grid, layout, "intensity", (16, 4), scale, shift, 0.1, np.eye(4), np.eye(4))
        far = np.eye(4)
        far[0, 3] = 2.0**20 * RES
        with pytest.raises(ValueError, match="packed-key limit"):
            odometry.deskew_insert(grid, layout, "intensity", field, scale, shift, 0.1, far, far)
        assert grid.info()["offered"] == 0 and grid.size() == 0
    finally:
        grid.close()


def test_a_frame_with_fewer_finite_points_than_neighbours_is_inserted_at_the_last_pose():
    integ = odometry.DynamicPointCloudIntegrator(RES, 0.0, 0, k_neighbors=20, target_num_points=500)
    try:
        full, _, _, (field, scale, shift), _ = make_cloud(600, "<f4", 24, 41)
        integ.insert_cloud2_timed(full, "intensity", field, scale, shift)
        before = integ.info()
        for keep in (7, 0):  # 7 finite points, then none
            msg, _, _, _, rec = make_cloud(50, "<f4", 24, 42 + keep)
            rec = rec.copy()
            rec["x"][keep:] = np.nan
            msg["data"] = rec.tobytes()
            assert integ.insert_cloud2_timed(msg, "intensity", field, scale, shift) == 50 - keep
            assert np.array_equal(integ.poses()[-1][0], np.eye(4)) and np.array_equal(integ.poses()[-1][1], np.eye(4))
        after = integ.info()
        assert after["model"] == before["model"] and after["frames"] == 3 and after["offered"] == 700 and after["voxels"] == before["voxels"] + 7
    finally:
        integ.close()


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------------
ROOM = np.array([[-10.0, -8.0, -1.5], [10.0, 8.0, 3.0]])
BOXES = np.array([[[3.0, 2.0, -1.5], [5.0, 4.0, 1.0]], [[-6.0, -5.0, -1.5], [-4.0, -2.0, 2.0]], [[-3.0, 4.0, -1.5], [0.0, 6.0, 0.5]]])
RINGS, COLUMNS, FRAMES, SCAN = 16, 512, 12, 0.1
VELOCITY, YAW_RATE = np.array([0.5, 0.0, 0.0]), 0.2
SPINNER = np.dtype({"names": ["x", "y", "z", "intensity", "t"], "formats": ["<f4", "<f4", "<f4", "<f4", "<f4"], "offsets": [0, 4, 8, 12, 16], "itemsize": 20})


def true_pose(t):
    T = np.eye(4)
    c, s = np.cos(YAW_RATE * t), np.sin(YAW_RATE * t)
    T[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = VELOCITY * t
    return T


def cast(origins, dirs):
    """Range of every ray to the nearest surface: the room from inside, the boxes from outside (slab method)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / dirs
        hi = np.maximum((ROOM[0] - origins) * inv, (ROOM[1] - origins) * inv)
        best = np.min(hi, axis=1)
        for lo_c, hi_c in BOXES:
            t0, t1 = (lo_c - origins) * inv, (hi_c - origins) * inv
            near, far = np.max(np.minimum(t0, t1), axis=1), np.min(np.maximum(t0, t1), axis=1)
            hit = (near <= far) & (near > 0.0)
            best = np.where(hit & (near < best), near, best)
    return best


def surface_distance(p):
    d = np.min(np.concatenate([p - ROOM[0], ROOM[1] - p], axis=1), axis=1)
    for lo_c, hi_c in BOXES:
        outside = np.linalg.norm(np.maximum(np.maximum(lo_c - p, p - hi_c), 0.0), axis=1)
        inside = np.min(np.concatenate([p - lo_c, hi_c - p], axis=1), axis=1)
        d = np.minimum(d, np.where(outside > 0.0, outside, np.abs(inside)))
    return np.abs(d)


def spinner_frames():
    az = 2.0 * np.pi * np.arange(COLUMNS) / COLUMNS
    el = np.deg2rad(np.linspace(-15.0, 15.0, RINGS))
    frames = []
    for f in range(FRAMES):
        t_col = np.arange(COLUMNS) * (SCAN / COLUMNS)
        rec = np.zeros(RINGS * COLUMNS, dtype=SPINNER)
        for j in range(COLUMNS):  # the columns are stamped: every column is cast from where the sensor is at its time
            T = true_pose(f * SCAN + t_col[j])
            d = np.stack([np.cos(el) * np.cos(az[j]), np.cos(el) * np.sin(az[j]), np.sin(el)], axis=1)
            r = cast(np.tile(T[:3, 3], (RINGS, 1)), d @ T[:3, :3].T)
            sl = slice(j * RINGS, (j + 1) * RINGS)
            rec["x"][sl], rec["y"][sl], rec["z"][sl] = (d * r[:, None]).T
            rec["t"][sl] = t_col[j]
            rec["intensity"][sl] = 40.0 + 10.0 * np.arange(RINGS) + 50.0 * np.sin(az[j])
        frames.append(rec)
    return frames


@pytest.fixture(scope="module")
def bag_dir(tmp_path_factory):
    src = tmp_path_factory.mktemp("dynamic_bags")
    frames = spinner_frames()
    image = (np.random.default_rng(3).integers(0, 256, size=(48, 64))).astype(np.uint8)
    msgs = [(0, (50, 0), fx.image((50, 0), image, "mono8"))]
    for f, rec in enumerate(frames):
        stamp = (100 + (f * 100000000) // 1000000000, (f * 100000000) % 1000000000)
        msgs.append((1, stamp, fx.cloud_from_struct(stamp, rec)))
    fx.write_bag(src / "run.bag", [(0, "/camera/image", "sensor_msgs/Image"), (1, "/points", "sensor_msgs/PointCloud2")], msgs, chunk_size=4, index=True)
    return src, frames


ARGS = ["--image_topic", "/camera/image", "--points_topic", "/points", "--camera_model", "plumb_bob", "--camera_intrinsics", "60,60,32,24", "--camera_distortion_coeffs", "0,0,0,0,0",
        "--voxel_resolution", "0.02", "--min_distance", "0.5"]
# |GPU pose - oracle pose| over the 12 frames, translation [m] and rotation [rad] of begin and end poses: measured once at
# 6.5e-12 m and 1.1e-12 rad; the bars are 10 x those.  It cannot be derived: a correspondence may flip on a last-place difference.
POSE_TOL_M, POSE_TOL_RAD = 6.5e-11, 1.1e-11


def pose_delta(A, B):
    D = se3.pose3_inverse(A) @ B
    return float(np.linalg.norm(D[:3, 3])), float(np.linalg.norm(se3.rot3_logmap(D[:3, :3])))


def test_preprocess_dynamic_end_to_end(bag_dir, tmp_path, capsys):
    src, frames = bag_dir
    dst = str(tmp_path / "data")
    # (a) the command writes a directory the calibration reads
    assert preprocess_dynamic.main([str(src), dst, "--target_num_points", "2000"] + ARGS) == 0
    data = dataset.VisualLiDARData(dst, "run.bag")
    assert data.image.shape == (48, 64) and data.points.shape[0] > 20000
    out = np.asarray(data.points)[:, :3]

    # the same frames through the integrator directly, to see its poses and sampled indices
    integ = odometry.DynamicPointCloudIntegrator(0.02, 0.5, 0, target_num_points=2000, seed=0)
    keeper = preprocess.TimeKeeper(log=lambda m: None)
    cpu = odometry.ScanMatcher(oracle.NumpyBackend(), 20)
    cpu_poses = []
    try:
        for f, rec in enumerate(frames):
            msg = {"fields": [(k, SPINNER.fields[k][1], 7) for k in SPINNER.names], "point_step": 20, "data": rec.tobytes(), "num_points": rec.shape[0], "is_bigendian": False}
            keep, scale, shift = keeper.process_times(100.0 + f * SCAN, float(rec["t"][0]), float(rec["t"][-1]), lambda: float(rec["t"].min()))
            assert keep and (scale, shift) == (1.0, 0.0)
            integ.insert_cloud2_timed(msg, "intensity", (16, 7), scale, shift)
            idx = integ.sampled[-1]
            pts = np.stack([rec["x"][idx], rec["y"][idx], rec["z"][idx]], axis=1).astype(np.float64)
            cpu_poses.append(cpu.insert(pts, rec["t"][idx].astype(np.float64)))
        records = integ.get_records()
        poses = integ.poses()
    finally:
        integ.close()
    assert np.array_equal(np.sort(records[:, :3].astype(np.float64), axis=0), np.sort(out, axis=0))  # the command ran this integrator

    # (b) per-frame poses against the oracle on the same sampled points
    dm = max(pose_delta(g, c)[0] for gp, cp in zip(poses, cpu_poses) for g, c in zip(gp, cp))
    dr = max(pose_delta(g, c)[1] for gp, cp in zip(poses, cpu_poses) for g, c in zip(gp, cp))
    # (c) against the truth
    truth_end = true_pose(FRAMES * SCAN - SCAN / COLUMNS)
    err_gpu, err_cpu = pose_delta(truth_end, poses[-1][1]), pose_delta(truth_end, cpu_poses[-1][1])
    # (d) sharper than the static integrator on the same bag
    static_dst = str(tmp_path / "static")
    assert preprocess_ros1.main([str(src), static_dst] + ARGS) == 0
    smeared = np.asarray(dataset.VisualLiDARData(static_dst, "run.bag").points)[:, :3]
    share_dyn, share_static = float(np.mean(surface_distance(out) < 0.03)), float(np.mean(surface_distance(smeared) < 0.03))
    print(f"end to end: |dpose| GPU-oracle {dm:.3e} m {dr:.3e} rad; final T_end error GPU {err_gpu[0]:.4f} m {err_gpu[1]:.5f} rad, oracle {err_cpu[0]:.4f} m {err_cpu[1]:.5f} rad; "
          f"within 3 cm: dynamic {share_dyn:.3f} static {share_static:.3f}; iterations {integ._matcher.iterations}")
    assert dm <= POSE_TOL_M and dr <= POSE_TOL_RAD
    assert err_gpu[0] <= 2.0 * err_cpu[0] and err_gpu[1] <= 2.0 * err_cpu[1]
    assert share_dyn > share_static
