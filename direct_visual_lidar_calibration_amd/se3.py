"""Small numpy SE(3) toolbox in the conventions the reference's callers use.

* pose storage = Sophus ``SE3d::data()`` order ``[qx qy qz qw tx ty tz]`` -- the 7 numbers Ceres
  hands to ``NIDCost::operator()`` (nid_cost.hpp:38, visual_camera_calibration.cpp:215-229);
* ``plus(x, delta)`` = ``T * exp(delta)``, delta = [upsilon; omega] -- ``Sophus::Manifold<SE3>::Plus``
  (visual_camera_calibration.cpp:216);
* ``plus_jacobian(x)`` = ``Dx_this_mul_exp_x_at_0`` (7x6), which Ceres right-multiplies onto the
  ambient gradient;
* ``pose3_expmap(xi)`` = GTSAM ``Pose3::Expmap``, xi = [omega; v] (Nelder-Mead path,
  visual_camera_calibration.cpp:104,129);
* TUM order ``[tx ty tz qx qy qz qw]`` for ``calib.json`` (calibrate.cpp:72-76,128-133).
"""
import numpy as np


def quat_mul(a, b):
    """Hamilton product, storage [x y z w]."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array(
        [
            aw * bx + ax * bw + ay * bz - az * by,
            aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw,
            aw * bw - ax * bx - ay * by - az * bz,
        ]
    )


def quat_to_rot(q):
    x, y, z, w = q
    return np.array(
        [
            [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)],
        ]
    )


def rot_to_quat(R):
    """Rotation matrix -> unit quaternion [x y z w] (Shepperd's method)."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        w = 0.25 * s
        x = (R[2, 1] - R[1, 2]) / s
        y = (R[0, 2] - R[2, 0]) / s
        z = (R[1, 0] - R[0, 1]) / s
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        w = (R[2, 1] - R[1, 2]) / s
        x = 0.25 * s
        y = (R[0, 1] + R[1, 0]) / s
        z = (R[0, 2] + R[2, 0]) / s
    elif R[1, 1] > R[2, 2]:
        s = np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        w = (R[0, 2] - R[2, 0]) / s
        x = (R[0, 1] + R[1, 0]) / s
        y = 0.25 * s
        z = (R[1, 2] + R[2, 1]) / s
    else:
        s = np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        w = (R[1, 0] - R[0, 1]) / s
        x = (R[0, 2] + R[2, 0]) / s
        y = (R[1, 2] + R[2, 1]) / s
        z = 0.25 * s
    q = np.array([x, y, z, w])
    return q / np.linalg.norm(q)


def hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def so3_exp_quat(omega):
    theta = np.linalg.norm(omega)
    if theta < 1e-10:
        half = 0.5 - theta * theta / 48.0
        w = 1.0 - theta * theta / 8.0
    else:
        half = np.sin(0.5 * theta) / theta
        w = np.cos(0.5 * theta)
    q = np.array([half * omega[0], half * omega[1], half * omega[2], w])
    return q / np.linalg.norm(q)


def _left_jacobian(omega):
    theta = np.linalg.norm(omega)
    W = hat(omega)
    if theta < 1e-8:
        return np.eye(3) + 0.5 * W + W @ W / 6.0
    return np.eye(3) + (1 - np.cos(theta)) / theta**2 * W + (theta - np.sin(theta)) / theta**3 * (W @ W)


def se3_exp(delta):
    """Sophus SE3::exp, delta = [upsilon(3); omega(3)] -> 7-vector."""
    ups, omega = np.asarray(delta[:3], float), np.asarray(delta[3:], float)
    q = so3_exp_quat(omega)
    t = _left_jacobian(omega) @ ups
    return np.concatenate([q, t])


def compose(a, b):
    """a * b for 7-vectors."""
    qa, ta = a[:4], a[4:]
    qb, tb = b[:4], b[4:]
    q = quat_mul(qa, qb)
    q = q / np.linalg.norm(q)
    t = quat_to_rot(qa) @ tb + ta
    return np.concatenate([q, t])


def inverse(a):
    q = np.array([-a[0], -a[1], -a[2], a[3]])
    t = -(quat_to_rot(q) @ a[4:])
    return np.concatenate([q, t])


def plus(x, delta):
    """Sophus::Manifold<SE3>::Plus: x * exp(delta)."""
    return compose(np.asarray(x, float), se3_exp(delta))


def plus_jacobian(x):
    """Sophus ``SE3::Dx_this_mul_exp_x_at_0`` (7x6): d(x * exp(delta))/d(delta) at 0, rows in
    storage order [qx qy qz qw tx ty tz], columns [upsilon; omega]."""
    qx, qy, qz, qw = x[:4]
    J = np.zeros((7, 6))
    J[0:4, 3:6] = 0.5 * np.array([[qw, -qz, qy], [qz, qw, -qx], [-qy, qx, qw], [-qx, -qy, -qz]])
    J[4:7, 0:3] = quat_to_rot(x[:4])
    return J


def to_matrix(x):
    T = np.eye(4)
    T[:3, :3] = quat_to_rot(x[:4])
    T[:3, 3] = x[4:]
    return T


def from_matrix(T):
    return np.concatenate([rot_to_quat(T[:3, :3]), T[:3, 3]])


def pose3_expmap(xi):
    """GTSAM Pose3::Expmap, xi = [omega(3); v(3)] -> 4x4 matrix (full SE(3) exponential)."""
    omega, v = np.asarray(xi[:3], float), np.asarray(xi[3:], float)
    T = np.eye(4)
    T[:3, :3] = quat_to_rot(so3_exp_quat(omega))
    T[:3, 3] = _left_jacobian(omega) @ v
    return T


def from_tum(v):
    """calib.json order [tx ty tz qx qy qz qw] -> 7-vector (quaternion normalised as
    calibrate.cpp:74 does)."""
    v = np.asarray(v, float)
    q = v[3:7] / np.linalg.norm(v[3:7])
    return np.concatenate([q, v[0:3]])


def to_tum(x):
    return np.concatenate([x[4:7], x[0:4]])


def delta_trans_rot(a, b):
    """|translation| and rotation angle of a^-1 * b (the convergence / parity measures)."""
    d = compose(inverse(a), b)
    ang = 2.0 * np.arctan2(np.linalg.norm(d[:3]), abs(d[3]))
    return float(np.linalg.norm(d[4:])), float(ang)


# ---- gtsam Pose3 on 4x4 matrices, xi = [omega; v], right-hand increments (what the CT-GICP factor of the dynamic integrator uses) ----
def rot3_expmap(omega):
    """gtsam ``SO3::Expmap`` (Rodrigues; ``I + hat(omega)`` where ``|omega|^2 <= eps``)"""
    omega = np.asarray(omega, float)
    theta2 = float(omega @ omega)
    W = hat(omega)
    if theta2 <= np.finfo(float).eps:
        return np.eye(3) + W
    theta = np.sqrt(theta2)
    return np.eye(3) + np.sin(theta) / theta * W + (1.0 - np.cos(theta)) / theta2 * (W @ W)


def rot3_logmap(R):
    """gtsam ``SO3::Logmap``: the rotation vector of R, with its branches near 0 and near pi"""
    tr = float(np.trace(R))
    if tr + 1.0 < 1e-10:  # angle pi: the axis from the largest diagonal entry
        i = int(np.argmax(np.diag(R)))
        e = np.zeros(3)
        e[i] = 1.0
        return np.pi / np.sqrt(2.0 + 2.0 * R[i, i]) * (R[:, i] + e)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    tr_3 = tr - 3.0
    if tr_3 < -1e-7:
        theta = np.arccos(min(1.0, max(-1.0, 0.5 * (tr - 1.0))))
        magnitude = theta / (2.0 * np.sin(theta))
    else:  # first-order Taylor around 0
        magnitude = 0.5 - tr_3 / 12.0
    return magnitude * v


def _series_b_c(theta2):
    """``(1 - cos theta) / theta^2`` and ``(theta - sin theta) / theta^3`` to theta^6 (exact to rounding for ``theta <= 1e-2``)"""
    b = 0.5 - theta2 * (1.0 / 24.0 - theta2 * (1.0 / 720.0 - theta2 / 40320.0))
    c = 1.0 / 6.0 - theta2 * (1.0 / 120.0 - theta2 * (1.0 / 5040.0 - theta2 / 362880.0))
    return b, c


def rot3_expmap_derivative(omega):
    """Right Jacobian of SO(3): ``Expmap(omega + d) ~ Expmap(omega) Expmap(J d)``"""
    omega = np.asarray(omega, float)
    theta2 = float(omega @ omega)
    W = hat(omega)
    if theta2 <= 1e-4:  # (the closed forms subtract nearly equal numbers below)
        b, c = _series_b_c(theta2)
        return np.eye(3) - b * W + c * (W @ W)
    theta = np.sqrt(theta2)
    return np.eye(3) - (1.0 - np.cos(theta)) / theta2 * W + (theta - np.sin(theta)) / (theta2 * theta) * (W @ W)


def rot3_logmap_derivative(omega):
    """Inverse of ``rot3_expmap_derivative``"""
    omega = np.asarray(omega, float)
    theta2 = float(omega @ omega)
    W = hat(omega)
    if theta2 <= 1e-8:
        return np.eye(3) + 0.5 * W + (1.0 / 12.0 + theta2 / 720.0) * (W @ W)
    theta = np.sqrt(theta2)
    return np.eye(3) + 0.5 * W + (1.0 / theta2 - (1.0 + np.cos(theta)) / (2.0 * theta * np.sin(theta))) * (W @ W)


def _pose3_q(xi):
    """The off-diagonal block of the right Jacobian of SE(3) (Barfoot's Q, eq. 7.86b, at -xi; gtsam ``computeQforExpmapDerivative``);
    series of the three coefficients below ``|omega| = 1e-2``"""
    w, v = -np.asarray(xi[:3], float), -np.asarray(xi[3:], float)
    W, V = hat(w), hat(v)
    phi2 = float(w @ w)
    phi = np.sqrt(phi2)
    if phi < 1e-2:  # (the closed forms subtract nearly equal numbers: b has no correct digit left at phi = 1e-4)
        p4 = phi2 * phi2
        a = 1.0 / 6.0 - phi2 / 120.0 + p4 / 5040.0
        b = -1.0 / 24.0 + phi2 / 720.0 - p4 / 40320.0
        c = b - 3.0 * (-1.0 / 120.0 + phi2 / 5040.0 - p4 / 362880.0)
    else:
        a = (phi - np.sin(phi)) / (phi2 * phi)
        b = (1.0 - 0.5 * phi2 - np.cos(phi)) / (phi2 * phi2)
        c = b - 3.0 * (phi - np.sin(phi) - phi2 * phi / 6.0) / (phi2 * phi2 * phi)
    WV, VW, WVW = W @ V, V @ W, W @ V @ W
    return 0.5 * V + a * (WV + VW + WVW) - b * (W @ WV + VW @ W - 3.0 * WVW) - 0.5 * c * (WVW @ W + W @ WVW)


def pose3_expmap_derivative(xi):
    """gtsam ``Pose3::ExpmapDerivative`` (6x6): ``Expmap(xi + d) ~ Expmap(xi) Expmap(J d)``"""
    J = np.zeros((6, 6))
    Jw = rot3_expmap_derivative(xi[:3])
    J[:3, :3] = Jw
    J[3:, 3:] = Jw
    J[3:, :3] = _pose3_q(xi)
    return J


def pose3_logmap(T):
    """gtsam ``Pose3::Logmap``: 4x4 -> xi = [omega; v]"""
    w = rot3_logmap(T[:3, :3])
    t = np.asarray(T[:3, 3], float)
    theta = np.linalg.norm(w)
    if theta < 1e-10:
        return np.concatenate([w, t])
    W = hat(w / theta)
    Wt = W @ t
    u = t - (0.5 * theta) * Wt + (1.0 - theta / (2.0 * np.tan(0.5 * theta))) * (W @ Wt)
    return np.concatenate([w, u])


def pose3_logmap_derivative(xi):
    """gtsam ``Pose3::LogmapDerivative`` at xi = Logmap(T): d Logmap(T Expmap(d)) / d d"""
    J = np.zeros((6, 6))
    Jw = rot3_logmap_derivative(xi[:3])
    J[:3, :3] = Jw
    J[3:, 3:] = Jw
    J[3:, :3] = -Jw @ _pose3_q(xi) @ Jw
    return J


def pose3_exp(xi):
    """``Pose3::Expmap`` as ``pose3_expmap`` above, with the series of the translation's coefficients below ``|omega| = 1e-2``
    (where ``(1 - cos) / theta^2`` has lost half its digits) and gtsam's first-order rotation at ``|omega|^2 <= eps``"""
    omega, v = np.asarray(xi[:3], float), np.asarray(xi[3:], float)
    theta2 = float(omega @ omega)
    W = hat(omega)
    if theta2 <= 1e-4:
        b, c = _series_b_c(theta2)
        V = np.eye(3) + b * W + c * (W @ W)
    else:
        theta = np.sqrt(theta2)
        V = np.eye(3) + (1.0 - np.cos(theta)) / theta2 * W + (theta - np.sin(theta)) / (theta2 * theta) * (W @ W)
    T = np.eye(4)
    T[:3, :3] = rot3_expmap(omega)
    T[:3, 3] = V @ v
    return T


def pose3_expmap_with_derivative(xi):
    """``(Pose3::Expmap(xi), its 6x6 derivative)``"""
    return pose3_exp(xi), pose3_expmap_derivative(xi)


def pose3_adjoint(T):
    """``Pose3::AdjointMap`` in [omega; v] order"""
    R, t = T[:3, :3], T[:3, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, 3:] = R
    A[3:, :3] = hat(t) @ R
    return A


def pose3_inverse(T):
    Ti = np.eye(4)
    Ti[:3, :3] = T[:3, :3].T
    Ti[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return Ti


def pose3_between(T1, T2):
    """``T1.between(T2, H1, H2)`` = ``(T1^-1 T2, -Ad(result^-1), I)``"""
    D = pose3_inverse(T1) @ T2
    return D, -pose3_adjoint(pose3_inverse(D)), np.eye(6)


def pose3_compose(T1, T2):
    """``T1.compose(T2, H1, H2)`` = ``(T1 T2, Ad(T2^-1), I)``"""
    return T1 @ T2, pose3_adjoint(pose3_inverse(T2)), np.eye(6)


def pose3_retract(T, xi):
    """``T * Expmap(xi)``: the increment the optimiser of the dynamic integrator applies"""
    return T @ pose3_exp(xi)


def pose3_interpolate_rt(T0, T1, t):
    """``Pose3::interpolateRt``: the rotation ``R0 Expmap(t Logmap(R0^T R1))``, the translation interpolated linearly"""
    T = np.eye(4)
    T[:3, :3] = T0[:3, :3] @ rot3_expmap(t * rot3_logmap(T0[:3, :3].T @ T1[:3, :3]))
    T[:3, 3] = T0[:3, 3] + t * (T1[:3, 3] - T0[:3, 3])
    return T
