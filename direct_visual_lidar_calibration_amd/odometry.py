"""``vlcal::DynamicPointCloudIntegrator`` (src/vlcal/preprocess/dynamic_point_cloud_integrator.cpp): the integrator of
``preprocess -d``.  The LiDAR moves; every scan is registered against a running model with continuous-time GICP -- two poses per
scan, the begin and the end of the sweep, every point transformed by the pose interpolated at its own time --, deskewed, and ALL
its raw points go into the voxel grid.

==========================================  ==================================================================================
here                                        reference
==========================================  ==================================================================================
``sort_and_sample``                         ``sort_by_time`` + ``randomgrid_sampling`` (src/vlcal/common/frame_cpu.cpp:443-507)
``time_table`` / ``update_poses``           ``IntegratedCT_ICPFactor_`` constructor and ``update_poses``
                                            (include/vlcal/common/integrated_ct_icp_factor_impl.hpp:34-45, :154-182)
``levenberg_marquardt``                     ``gtsam::LevenbergMarquardtOptimizer`` with default parameters (NOT in the reference tree)
``ScanMatcher.insert``                      ``DynamicPointCloudIntegrator::insert_points`` (:50-121)
``DeviceBackend``                           the GPU side behind ``include/nidreg.h`` (``nidreg_odom_*``, csrc/nid_odom_kernels.hpp): kNN and
                                            covariances, the iVox model, the CT-GICP linearisation and error
``DynamicPointCloudIntegrator``             the class, with ``StaticPointCloudIntegrator``'s surface; ``voxelgrid_task`` (:123-155) is
                                            ``nidreg_odom_deskew_insert``
==========================================  ==================================================================================

The host does what touches four columns of ~10^5 points once (decode, finite filter, sort, sample) and the 12-unknown optimiser; the
device does the rest.  Differences from the reference, all deliberate:

* sampling draws from ``numpy.random.Generator(MT19937(seed))`` (the reference's ``std::sample`` over an ``unordered_map``'s
  iteration order is not reproducible across standard libraries); its rules are kept;
* the optimiser restates gtsam's Levenberg-Marquardt from its documented defaults; gtsam itself is not available, so it is
  UNPINNED against it;
* iVox's LRU eviction (``lru_thresh`` = 100 scans, looked at on every 10th insert; ivox.cpp:144-178, :223) runs on the device and
  is checked against a restatement of that rule (tests/odometry_lru_oracle.py) that is itself UNPINNED against a compiled
  ``ivox.cpp``; its "too many voxels" branch (2^32 - 1 voxels) is not built, and ``lru_thresh=0`` keeps a model that only grows;
* the voxel insert evaluates ``interpolateRt`` per point (the reference refreshes the pose every 1e-4 of normalised time), and
  within a frame the point with the highest message index wins a voxel (the reference: the latest in time);
* where the reference divides by zero: a frame whose largest time is <= 0 uses t = 0 for every point, a scan duration <= 0 gives
  a zero velocity prediction, and a linearisation without a correspondence keeps the prediction;
* a frame with fewer finite points than ``k_neighbors`` (the reference would read past its short neighbour lists) is not
  registered: it is inserted at the last pose, and neither the model nor the velocity changes.
"""
import ctypes
import math

import numpy as np

from . import _lib, preprocess, se3

UINT32, FLOAT32, FLOAT64 = 6, 7, 8  # sensor_msgs/PointField datatypes a time field may have
_FIELD_DTYPES = {UINT32: "<u4", FLOAT32: "<f4", FLOAT64: "<f8"}
SUMS = 122  # nidreg_odom_linearize: H_00 H_01 H_11 b_0 b_1 error count


# ---- host steps -------------------------------------------------------------------------------------------------------------
def randomgrid_sampling(points, voxel_resolution, sampling_rate, rng):
    """``randomgrid_sampling`` (frame_cpu.cpp:443-498): ascending indices of the sampled points.  ``rate >= 0.99`` keeps everything;
    else at most ``ceil(rate n / voxels)`` per ``voxel_resolution`` cell (cells in ascending key order, a cell's surplus drawn
    without replacement), capped at ``int(1.2 rate n)`` by a second draw."""
    n = points.shape[0]
    if sampling_rate >= 0.99 or n == 0:
        return np.arange(n, dtype=np.int64)
    cells = np.floor(points[:, :3] / voxel_resolution).astype(np.int64)
    _, inverse, counts = np.unique(cells, axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    per_voxel = int(math.ceil((sampling_rate * n) / counts.shape[0]))
    max_num = int(n * sampling_rate * 1.2)
    order = np.argsort(inverse, kind="stable")
    starts = np.concatenate([[0], np.cumsum(counts)])
    chosen = []
    for v in range(counts.shape[0]):
        members = order[starts[v] : starts[v + 1]]
        chosen.append(members if members.shape[0] <= per_voxel else rng.choice(members, size=per_voxel, replace=False))
    indices = np.concatenate(chosen)
    if indices.shape[0] > max_num:
        indices = rng.choice(indices, size=max_num, replace=False)
    return np.sort(indices).astype(np.int64)


def sort_and_sample(points, times, target_num_points, rng):
    """``sort_by_time`` (stable) then ``randomgrid_sampling(0.5 m, target / n)``: ``(order, sampled)`` -- ``order`` sorts the frame
    by time, ``sampled`` indexes the sorted frame"""
    order = np.argsort(times, kind="stable")
    n = order.shape[0]
    sampled = randomgrid_sampling(points[order], 0.5, (float(target_num_points) / n) if n else 1.0, rng)
    return order, sampled


def time_table(times, time_eps=1e-3):
    """The factor's constructor (:34-45): ``(table normalised by max(1e-9, last), index per point)``"""
    table, indices = [], np.empty(len(times), dtype=np.int32)
    for i, t in enumerate(times):
        if not table or t - table[-1] > time_eps:
            table.append(float(t))
        indices[i] = len(table) - 1
    table = np.asarray(table, dtype=np.float64)
    if table.shape[0]:
        table = table / max(1e-9, table[-1])
    return table, indices


def _hat_batch(w):
    W = np.zeros(w.shape[:-1] + (3, 3))
    W[..., 0, 1], W[..., 0, 2], W[..., 1, 0] = -w[..., 2], w[..., 1], w[..., 2]
    W[..., 1, 2], W[..., 2, 0], W[..., 2, 1] = -w[..., 0], -w[..., 1], w[..., 0]
    return W


def _expmap_batch(xis, derivatives):
    """``se3.pose3_exp`` and ``se3.pose3_expmap_derivative`` for the rows of ``xis`` (K, 6) at once, with the same branches:
    ``(poses (K, 4, 4), derivatives (K, 6, 6) or None)``"""
    K = xis.shape[0]
    w, v = xis[:, :3], xis[:, 3:]
    th2 = np.einsum("ki,ki->k", w, w)
    W = _hat_batch(w)
    W2 = W @ W
    eye = np.eye(3)[None]
    col = lambda a: a[:, None, None]  # noqa: E731
    big = th2 > np.finfo(float).eps  # rot3_expmap: I + hat(omega) at and below
    t2 = np.where(big, th2, 1.0)
    th = np.sqrt(t2)
    R = eye + col(np.where(big, np.sin(th) / th, 1.0)) * W + col(np.where(big, (1.0 - np.cos(th)) / t2, 0.0)) * W2
    series = th2 <= 1e-4  # se3._series_b_c
    t2 = np.where(series, 1.0, th2)
    th = np.sqrt(t2)
    sb, sc = se3._series_b_c(th2)
    b, c = np.where(series, sb, (1.0 - np.cos(th)) / t2), np.where(series, sc, (th - np.sin(th)) / (t2 * th))
    poses = np.zeros((K, 4, 4))
    poses[:, :3, :3], poses[:, 3, 3] = R, 1.0
    poses[:, :3, 3] = np.einsum("kij,kj->ki", eye + col(b) * W + col(c) * W2, v)
    if not derivatives:
        return poses, None
    J = np.zeros((K, 6, 6))
    J[:, :3, :3] = J[:, 3:, 3:] = eye - col(b) * W + col(c) * W2
    p4 = th2 * th2
    qb = np.where(series, -1.0 / 24.0 + th2 / 720.0 - p4 / 40320.0, (1.0 - 0.5 * t2 - np.cos(th)) / (t2 * t2))  # se3._pose3_q
    qd = np.where(series, -1.0 / 120.0 + th2 / 5040.0 - p4 / 362880.0, (th - np.sin(th) - t2 * th / 6.0) / (t2 * t2 * th))
    qa = np.where(series, 1.0 / 6.0 - th2 / 120.0 + p4 / 5040.0, c)
    qc = qb - 3.0 * qd
    Wn, Vn = -W, _hat_batch(-v)
    WV, VW = Wn @ Vn, Vn @ Wn
    WVW = WV @ Wn
    J[:, 3:, :3] = 0.5 * Vn + col(qa) * (WV + VW + WVW) - col(qb) * (Wn @ WV + VW @ Wn - 3.0 * WVW) - 0.5 * col(qc) * (WVW @ Wn + Wn @ WVW)
    return poses, J


def update_poses(T0, T1, table, derivatives=True):
    """``update_poses`` (:154-182): per table entry the pose ``T0 Expmap(t Logmap(T0^-1 T1))`` (K, 4, 4) and, with
    ``derivatives``, d pose / d T0 and d pose / d T1 (K, 6, 6 each; right-hand increments, [omega; v]); all entries at once."""
    D, H_delta_0, H_delta_1 = se3.pose3_between(T0, T1)
    vel = se3.pose3_logmap(D)
    table = np.asarray(table, dtype=np.float64)
    inc, H_inc_vel = _expmap_batch(table[:, None] * vel[None, :], derivatives)
    poses = T0[None] @ inc
    if not derivatives:
        return poses, None, None
    Rt = np.transpose(inc[:, :3, :3], (0, 2, 1))
    H_pose_0 = np.zeros((table.shape[0], 6, 6))  # Ad(inc^-1); d compose / d inc is the identity
    H_pose_0[:, :3, :3] = H_pose_0[:, 3:, 3:] = Rt
    H_pose_0[:, 3:, :3] = _hat_batch(-np.einsum("kij,kj->ki", Rt, inc[:, :3, 3])) @ Rt
    H_pose_delta = (H_inc_vel @ se3.pose3_logmap_derivative(vel)[None]) * table[:, None, None]
    return poses, H_pose_0 + H_pose_delta @ H_delta_0[None], H_pose_delta @ H_delta_1[None]


def pack_poses(poses, d0=None, d1=None):
    """The table as the device reads it: per entry R (9, row-major) t (3) [and the two 6 x 6 derivatives]"""
    K = poses.shape[0]
    out = np.empty((K, 12 if d0 is None else 84))
    out[:, :9] = poses[:, :3, :3].reshape(K, 9)
    out[:, 9:12] = poses[:, :3, 3]
    if d0 is not None:
        out[:, 12:48] = d0.reshape(K, 36)
        out[:, 48:84] = d1.reshape(K, 36)
    return np.ascontiguousarray(out)


def levenberg_marquardt(x0, linearize, error, retract, max_iterations=10, lambda_initial=1e-5, lambda_factor=10.0, lambda_upper=1e5, rel_tol=1e-5, abs_tol=1e-5,
                        min_model_fidelity=1e-3):
    """gtsam's ``LevenbergMarquardtOptimizer::optimize`` with its default parameters, diagonal damping off: ``linearize(x)`` ->
    ``(H, g, error)`` of the quadratic model ``error + g^T d + d^T H d / 2``; a trial step solves ``(H + lambda I) d = -g`` and is
    evaluated with ``error(retract(x, d))``; it is accepted when the gain ratio exceeds ``min_model_fidelity`` (lambda /= factor),
    else lambda *= factor until it passes ``lambda_upper``.  Stops after ``max_iterations``, or when an accepted step lowers the
    error by <= ``abs_tol`` or relatively by <= ``rel_tol``.  Returns ``(x, error, iterations)``."""
    x, lam = x0, lambda_initial
    current = None
    for it in range(max_iterations):
        H, g, lin_error = linearize(x)
        if current is None:
            current = lin_error
        n = g.shape[0]
        accepted = False
        while True:
            try:
                d = np.linalg.solve(H + lam * np.eye(n), -g)
            except np.linalg.LinAlgError:
                d = None
            if d is not None and np.all(np.isfinite(d)):
                model_change = -(g @ d + 0.5 * d @ H @ d)  # the linearised decrease
                trial = retract(x, d)
                new = error(trial)
                cost_change = current - new
                if model_change > 0.0 and np.isfinite(new) and cost_change / model_change > min_model_fidelity:
                    accepted = True
                    lam = lam / lambda_factor
                    break
            lam *= lambda_factor
            if lam > lambda_upper:
                break
        if not accepted:
            return x, current, it + 1
        x, previous, current = trial, current, new
        decrease = previous - current
        if decrease <= abs_tol or (previous > 0.0 and decrease / previous <= rel_tol):
            return x, current, it + 1
    return x, current, max_iterations


# ---- the device ---------------------------------------------------------------------------------------------------------------
def _dp(a):
    return a.ctypes.data_as(_lib.c_double_p)


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


class ModelFullError(RuntimeError):
    """``NIDREG_ERR_FULL``: the model's pool of point blocks (``max_blocks``) is exhausted; points of the scan are missing from it"""


def _check(rc, what):
    if rc == _lib.NIDREG_ERR_FULL:
        raise ModelFullError(f"{what}: {_lib.last_error()}")
    return preprocess._check(rc, what)


class DeviceBackend:
    """The ``nidreg_odom_*`` handle: the model and the current scan on the GPU.  No CPU implementation stands behind it."""

    def __init__(self, device=0, voxel_resolution=1.0, insertion_dist_thresh=0.05, max_blocks=1 << 18, lru_thresh=0, lru_cycle=10):
        """``lru_thresh`` > 0: a voxel neither inserted into nor found by a search for more than ``lru_thresh`` inserts leaves the model
        on the next insert whose count is a multiple of ``lru_cycle`` (iVox's rule); 0: the model only grows"""
        self._lib = _lib.load()
        self._h = None
        h = ctypes.c_void_p()
        _check(self._lib.nidreg_odom_create(int(device), float(voxel_resolution), float(insertion_dist_thresh), int(max_blocks), ctypes.byref(h)), "nidreg_odom_create")
        self._h = h
        self._m = 0
        if (int(lru_thresh), int(lru_cycle)) != (0, 10):
            self.set_lru(lru_thresh, lru_cycle)

    def set_lru(self, lru_thresh, lru_cycle=10):
        """``nidreg_odom_set_lru``: before the first ``model_insert`` only"""
        _check(self._lib.nidreg_odom_set_lru(self._h, int(lru_thresh), int(lru_cycle)), "nidreg_odom_set_lru")

    def lru_info(self):
        v = (ctypes.c_int64 * 4)()
        _check(self._lib.nidreg_odom_lru_info(self._h, v), "nidreg_odom_lru_info")
        return {"lru_count": int(v[0]), "evicted_voxels": int(v[1]), "free_blocks": int(v[2]), "passes": int(v[3])}

    def knn_covariances(self, points, k):
        """``(neighbors (m, k) int32, normals (m, 3), covs (m, 6))``"""
        points = np.ascontiguousarray(points, dtype=np.float64)
        m = points.shape[0]
        nbr, normals, covs = np.empty((m, max(k, 0)), dtype=np.int32), np.empty((m, 3)), np.empty((m, 6))
        _check(self._lib.nidreg_odom_knn_covariances(self._h, _dp(points), m, int(k), _ip(nbr), _dp(normals), _dp(covs)), "nidreg_odom_knn_covariances")
        return nbr, normals, covs

    def covariances(self, points, neighbors):
        """``(normals, covs)`` from a given neighbour list"""
        points = np.ascontiguousarray(points, dtype=np.float64)
        neighbors = np.ascontiguousarray(neighbors, dtype=np.int32)
        m = points.shape[0]
        normals, covs = np.empty((m, 3)), np.empty((m, 6))
        _check(self._lib.nidreg_odom_covariances(self._h, _dp(points), m, int(neighbors.shape[1]), _ip(neighbors), _dp(normals), _dp(covs)), "nidreg_odom_covariances")
        return normals, covs

    def model_insert(self, points, covs):
        points, covs = np.ascontiguousarray(points, dtype=np.float64), np.ascontiguousarray(covs, dtype=np.float64)
        _check(self._lib.nidreg_odom_model_insert(self._h, _dp(points), _dp(covs), points.shape[0]), "nidreg_odom_model_insert")

    def model_info(self):
        v = (ctypes.c_int64 * 4)()
        _check(self._lib.nidreg_odom_model_info(self._h, v), "nidreg_odom_model_info")
        return {"voxels": int(v[0]), "points": int(v[1]), "blocks": int(v[2]), "max_blocks": int(v[3])}

    def model_points(self):
        """``(voxels (n, 3) int32, points (n, 3), covs (n, 6))``: voxels in ascending key order, a voxel's points in list order"""
        n = self.model_info()["points"]
        vox, pts, covs = np.empty((n, 3), dtype=np.int32), np.empty((n, 3)), np.empty((n, 6))
        _check(self._lib.nidreg_odom_model_get(self._h, _ip(vox), _dp(pts), _dp(covs)), "nidreg_odom_model_get")
        return vox, pts, covs

    def set_source(self, points, covs, time_index):
        points, covs = np.ascontiguousarray(points, dtype=np.float64), np.ascontiguousarray(covs, dtype=np.float64)
        time_index = np.ascontiguousarray(time_index, dtype=np.int32)
        _check(self._lib.nidreg_odom_set_source(self._h, _dp(points), _dp(covs), _ip(time_index), points.shape[0]), "nidreg_odom_set_source")
        self._m = points.shape[0]

    def linearize(self, packed_poses, max_correspondence_dist_sq=1.0):
        """The 122 sums of ``nidreg_odom_linearize`` at the packed (K, 84) table"""
        out = np.empty(SUMS)
        _check(self._lib.nidreg_odom_linearize(self._h, _dp(packed_poses), packed_poses.shape[0], float(max_correspondence_dist_sq), _dp(out)), "nidreg_odom_linearize")
        return out

    def error(self, packed_poses):
        """``(error, matched points)`` at the packed (K, 12) table, on the correspondences of the last ``linearize``"""
        out = np.empty(2)
        _check(self._lib.nidreg_odom_error(self._h, _dp(packed_poses), packed_poses.shape[0], _dp(out)), "nidreg_odom_error")
        return float(out[0]), int(out[1])

    def correspondences(self):
        """``(found (m,) int32, target (m, 3), mahalanobis (m, 3, 3))`` of the last ``linearize``"""
        found, target, mahal = np.empty(self._m, dtype=np.int32), np.empty((self._m, 3)), np.empty((self._m, 3, 3))
        _check(self._lib.nidreg_odom_correspondences(self._h, _ip(found), _dp(target), _dp(mahal)), "nidreg_odom_correspondences")
        return found, target, mahal

    def close(self):
        if getattr(self, "_h", None):
            self._lib.nidreg_odom_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the scan matcher -----------------------------------------------------------------------------------------------------------
class ScanMatcher:
    """``DynamicPointCloudIntegrator::insert_points`` (:50-121) without the voxel grid: scans in, ``(T_begin, T_end)`` out.
    ``backend`` does the per-point work (``DeviceBackend``; the tests' CPU restatement has the same methods)."""

    PRIOR_PRECISION, BETWEEN_PRECISION, PREDICTION_FACTOR, RESTARTS = 1e3, 1e5, 0.75, 3

    def __init__(self, backend, k_neighbors=20):
        self.backend, self.k = backend, int(k_neighbors)
        self.last_begin, self.last_end = np.eye(4), np.eye(4)
        self.has_model = False
        self.iterations = []

    def insert(self, points, times):
        """``points`` (m, 3) and ``times`` (m,) of the sampled scan, sorted by time; returns ``(T_begin, T_end)``"""
        points = np.ascontiguousarray(points[:, :3], dtype=np.float64)
        neighbors, _, covs = self.backend.knn_covariances(points, self.k)
        if not self.has_model:  # :70-75
            self.backend.model_insert(points, covs)
            self.has_model = True
            return np.eye(4), np.eye(4)
        scan_duration = float(times[-1])
        if scan_duration > 0.0:  # :77-80
            velocity = se3.pose3_logmap(se3.pose3_between(self.last_begin, self.last_end)[0]) / scan_duration
        else:
            velocity = np.zeros(6)
        begin, end = self.last_end.copy(), self.last_end @ se3.pose3_exp(self.PREDICTION_FACTOR * velocity * scan_duration)
        table, indices = time_table(times)
        self.backend.set_source(points, covs, indices)
        x = (begin, end)
        prior = begin.copy()

        def priors(x, jacobians):
            r0 = se3.pose3_logmap(se3.pose3_inverse(prior) @ x[0])
            D, Hd0, _ = se3.pose3_between(x[0], x[1])
            r1 = se3.pose3_logmap(D)
            e = 0.5 * self.PRIOR_PRECISION * (r0 @ r0) + 0.5 * self.BETWEEN_PRECISION * (r1 @ r1)
            if not jacobians:
                return e
            H, g = np.zeros((12, 12)), np.zeros(12)
            J0 = se3.pose3_logmap_derivative(r0)
            H[:6, :6] += self.PRIOR_PRECISION * (J0.T @ J0)
            g[:6] += self.PRIOR_PRECISION * (J0.T @ r0)
            JL = se3.pose3_logmap_derivative(r1)
            J = np.hstack([JL @ Hd0, JL])
            H += self.BETWEEN_PRECISION * (J.T @ J)
            g += self.BETWEEN_PRECISION * (J.T @ r1)
            return e, H, g

        matched = [0]

        def linearize(x):
            poses, d0, d1 = update_poses(x[0], x[1], table)
            s = self.backend.linearize(pack_poses(poses, d0, d1))
            matched[0] = int(s[121])
            e, H, g = priors(x, True)
            H[:6, :6] += s[0:36].reshape(6, 6)
            H[:6, 6:] += s[36:72].reshape(6, 6)
            H[6:, :6] += s[36:72].reshape(6, 6).T
            H[6:, 6:] += s[72:108].reshape(6, 6)
            g[:6] += s[108:114]
            g[6:] += s[114:120]
            return H, g, e + float(s[120])

        def error(x):
            poses, _, _ = update_poses(x[0], x[1], table, derivatives=False)
            return priors(x, False) + self.backend.error(pack_poses(poses))[0]

        def retract(x, d):
            return se3.pose3_retract(x[0], d[:6]), se3.pose3_retract(x[1], d[6:])

        total = 0
        for _ in range(self.RESTARTS):  # :100-102
            x, _, its = levenberg_marquardt(x, linearize, error, retract)
            total += its
        self.iterations.append(total)
        if matched[0] == 0:  # nothing to register against: the prediction stands
            x = (begin, end)
        self.last_begin, self.last_end = x
        poses, _, _ = update_poses(x[0], x[1], table, derivatives=False)
        P = poses[indices]
        deskewed = np.einsum("nij,nj->ni", P[:, :3, :3], points) + P[:, :3, 3]  # :107-110
        _, covs = self.backend.covariances(deskewed, neighbors)
        self.backend.model_insert(deskewed, covs)
        return x


def decode_columns(data, n, step, table, time_field):
    """x, y, z (and the raw time column, or None) of a frame as strided views of its bytes"""
    def column(offset, datatype):
        if offset < 0 or offset + np.dtype(_FIELD_DTYPES[datatype]).itemsize > step:
            raise ValueError(f"insert_cloud2_timed: a field at offset {offset} lies outside the {step}-byte record")
        return np.ndarray(shape=(n,), dtype=np.dtype(_FIELD_DTYPES[datatype]), buffer=data, offset=offset, strides=(step,))

    xyz = [column(table[c][0], table[c][1]) for c in ("x", "y", "z")]
    raw = None if time_field is None else column(time_field[0], time_field[1])
    return xyz, raw


def deskew_insert(grid, layout, intensity_channel, time_field, scale, shift, max_time, T_begin, T_end):
    """``voxelgrid_task`` (:123-155) for one raw frame into ``grid`` (a ``StaticPointCloudIntegrator``): ``layout`` =
    ``preprocess.cloud2_layout``'s result, the time column as ``insert_cloud2_timed`` takes it, ``max_time`` the frame's largest time
    (<= 0: every point at t = 0).  Returns the number of points skipped for a non-finite coordinate."""
    data, n, step, table = layout
    begin12 = np.ascontiguousarray(np.concatenate([T_begin[:3, :3].reshape(9), T_begin[:3, 3]]), dtype=np.float64)
    rotvec = np.ascontiguousarray(se3.rot3_logmap(T_begin[:3, :3].T @ T_end[:3, :3]), dtype=np.float64)
    dtrans = np.ascontiguousarray(T_end[:3, 3] - T_begin[:3, 3], dtype=np.float64)
    skipped = ctypes.c_int64()
    ch = table[intensity_channel]
    rc = grid._lib.nidreg_odom_deskew_insert(grid._h, data.ctypes.data if n else None, n, step, table["x"][0], table["y"][0], table["z"][0], table["x"][1], ch[0], ch[1],
                                             0 if time_field is None else int(time_field[0]), 0 if time_field is None else int(time_field[1]), float(scale), float(shift), float(max_time),
                                             _dp(begin12), _dp(rotvec), _dp(dtrans), ctypes.byref(skipped))
    _check(rc, "nidreg_odom_deskew_insert")
    return int(skipped.value)


class DynamicPointCloudIntegrator:
    """``vlcal::DynamicPointCloudIntegrator`` with ``StaticPointCloudIntegrator``'s surface (``insert_cloud2``, ``get_records``,
    ``info``, ``close``) and ``poses()``.  Defaults as the reference's (:22-30).  Unlike the static integrator of
    ``preprocess_ros1`` it applies ``min_distance`` -- in the odometry frame, as the reference does (:149)."""

    def __init__(self, voxel_resolution=0.05, min_distance=1.0, device=0, k_neighbors=20, target_num_points=10000, seed=0, max_blocks=1 << 18, lru_thresh=100):
        self._grid = preprocess.StaticPointCloudIntegrator(voxel_resolution, min_distance, device)
        self._backend = DeviceBackend(device, max_blocks=max_blocks, lru_thresh=lru_thresh)  # iVox(1.0, 0.05, 100): lru_cycle stays 10
        self._matcher = ScanMatcher(self._backend, k_neighbors)
        self._lib = self._grid._lib
        self.target_num_points = int(target_num_points)
        self.rng = np.random.Generator(np.random.MT19937(seed))
        self._poses = []
        self.sampled = []  # per frame: indices into the message of the sampled points, in time order (what a CPU restatement needs to follow)
        self.last_seq = None

    def insert_cloud2(self, msg_or_fields, intensity_channel):
        """A frame without per-point times: every point at t = 0"""
        return self.insert_cloud2_timed(msg_or_fields, intensity_channel, None, 0.0, 0.0)

    def insert_cloud2_timed(self, msg_or_fields, intensity_channel, time_field, scale, shift):
        """One PointCloud2 frame with its per-point times: ``time_field`` = ``(offset, datatype)`` of the time column (UINT32,
        FLOAT32 or FLOAT64) and ``time = raw * scale + shift``, or ``None`` and ``time = scale * index / n``
        (``preprocess.TimeKeeper.process_times``).  Registers the frame, then inserts all its raw points deskewed.  Returns the number
        of points skipped for a non-finite coordinate."""
        data, n, step, table = preprocess.cloud2_layout(msg_or_fields, intensity_channel, who="insert_cloud2_timed")
        if table["x"][1] not in (FLOAT32, FLOAT64):
            raise ValueError(f"insert_cloud2_timed: x, y and z must be FLOAT32 or FLOAT64, got datatype {table['x'][1]}")
        if time_field is not None and time_field[1] not in _FIELD_DTYPES:
            raise ValueError(f"insert_cloud2_timed: unsupported time datatype {time_field[1]}")
        (x, y, z), raw = decode_columns(data, n, step, table, time_field)
        if raw is None:
            times = (float(scale) * np.arange(n, dtype=np.float64)) / n if n else np.zeros(0)
        else:
            times = raw.astype(np.float64) * float(scale) + float(shift)
        finite = np.flatnonzero(np.isfinite(x) & np.isfinite(y) & np.isfinite(z))  # preprocess.cpp:457
        points = np.stack([x[finite], y[finite], z[finite]], axis=1).astype(np.float64)
        order, sampled = sort_and_sample(points, times[finite], self.target_num_points, self.rng)
        sorted_times = times[finite][order]
        max_time = float(sorted_times[-1]) if sorted_times.shape[0] else 0.0
        if sampled.shape[0] < self._matcher.k:  # too few finite points for a neighbourhood (none at all included): not registered
            begin, end = self._matcher.last_end.copy(), self._matcher.last_end.copy()
        else:
            t = sorted_times[sampled] if max_time > 0.0 else np.zeros(sampled.shape[0])
            begin, end = self._matcher.insert(points[order][sampled], t)
        self.sampled.append(finite[order][sampled])
        self._poses.append((begin, end))
        return deskew_insert(self._grid, (data, n, step, table), intensity_channel, time_field, scale, shift, max_time, begin, end)

    def poses(self):
        """Per inserted frame ``(T_odom_lidar_begin, T_odom_lidar_end)`` (4 x 4 each)"""
        return list(self._poses)

    def info(self):
        """The voxel grid's ``info()`` plus ``{"model": the model's voxels / points / blocks, "lru": the eviction's totals, "frames"}``"""
        out = self._grid.info()
        out["model"] = self._backend.model_info()
        out["lru"] = self._backend.lru_info()
        out["frames"] = len(self._poses)
        return out

    def size(self):
        return self._grid.size()

    def get_records(self):
        rec = self._grid.get_records()
        self.last_seq = self._grid.last_seq
        return rec

    def get_points(self):
        return self._grid.get_points()

    def close(self):
        self._backend.close()
        self._grid.close()
