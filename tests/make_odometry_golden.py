"""Writes tests/golden/odometry_eigen_cases.npz: the neighbourhoods of tests/test_odometry_edges.py's covariance cases with their
EXACT smallest-eigenvalue unit normal and eigenvalues (test infrastructure, not a test).

The float64 inputs are taken as exact rationals; mpmath at 50 digits computes the two-pass covariance (mean first, then the centred
products, divided by k - 1) and ``eigsy``.  The GPU test reads the file and does not need mpmath; an unmarked test regenerates the
cases in memory where mpmath imports and compares them with the file.  Deterministic: ``python tests/make_odometry_golden.py``.

Per case: ``points`` (k, 3), ``lists`` (k,) -- the neighbour list, a fixed permutation of the points --, ``normal`` (3,) with its
largest component positive, ``eigenvalues`` (3,) ascending.  Arrays are padded to ``MAX_POINTS`` rows (lists with -1).
"""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "odometry_eigen_cases.npz")
MAX_POINTS = 32
DISTANCES = (0.0, 4.0, 100.0, 1000.0)  # the translation cases: the same patch this far from the origin
AWAY = np.array([2.0, -1.0, 2.0]) / 3.0  # ... along this unit vector
LINES = {"x": (np.array([1.0, 0.0, 0.0]), 0.25), "z": (np.array([0.0, 0.0, 1.0]), 0.25), "345": (np.array([3.0, 0.0, 4.0]), 0.0625), "111": (np.array([1.0, 1.0, 1.0]), 0.125)}


def _dyadic(rng, shape, span, bits=6):
    """Multiples of 2^-bits in [-span, span)"""
    return rng.integers(-span * 2**bits, span * 2**bits, size=shape).astype(np.float64) / 2.0**bits


def _patch(rng, k, extent=0.2, noise=1e-3):
    """A noisy planar patch (normal about (1, 2, 2) / 3) of the given extent around the origin"""
    n = np.array([1.0, 2.0, 2.0]) / 3.0
    u = np.array([2.0, 1.0, -2.0]) / 3.0
    v = np.cross(n, u)
    ab = rng.uniform(-0.5 * extent, 0.5 * extent, size=(k, 2))
    return ab[:, :1] * u + ab[:, 1:] * v + rng.normal(0.0, noise, size=(k, 1)) * n


def build_cases():
    """``[(name, group, points (k, 3), list (k,))]`` in a fixed order"""
    cases = []

    def add(name, group, pts, seed):
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        assert pts.shape[0] <= MAX_POINTS
        cases.append((name, group, pts, np.random.default_rng(seed).permutation(pts.shape[0]).astype(np.int32)))

    for k in (5, 20):
        rng = np.random.default_rng(900 + k)
        # exact planes, dyadic coordinates (every product and sum of the one-pass covariance is exact)
        ab = _dyadic(rng, (k, 2), 4)
        add(f"plane_z_k{k}", "plane", np.stack([ab[:, 0], ab[:, 1], np.full(k, 1.5)], axis=1), 1)
        add(f"plane_x_k{k}", "plane", np.stack([np.full(k, -2.25), ab[:, 0], ab[:, 1]], axis=1), 2)
        add(f"plane_xy_k{k}", "plane", np.stack([ab[:, 0], 3.0 - ab[:, 0], ab[:, 1]], axis=1), 3)  # x + y = 3
        # a ring of k points (lambda_1 ~ lambda_2) and two strips (lambda_2 >> lambda_1), tilted, 2 m from the origin
        n = np.array([1.0, 2.0, 2.0]) / 3.0
        u = np.array([2.0, 1.0, -2.0]) / 3.0
        v = np.cross(n, u)
        centre = np.array([1.0, -1.5, 0.8])
        ang = 2.0 * np.pi * np.arange(k) / k + 0.1
        add(f"disc_k{k}", "disc", centre + 0.3 * np.cos(ang)[:, None] * u + 0.3 * np.sin(ang)[:, None] * v + rng.normal(0.0, 1e-3, size=(k, 1)) * n, 4)
        for aspect in (30, 1000):  # points along 2 m, alternating between the strip's two edges; 1 um across the plane
            s = np.linspace(-1.0, 1.0, k)
            w = (1.0 / aspect) * np.where(np.arange(k) % 2 == 0, 1.0, -1.0)
            add(f"strip{aspect}_k{k}", f"strip{aspect}", centre + s[:, None] * u + w[:, None] * v + rng.normal(0.0, 1e-6, size=(k, 1)) * n, 5)
        # exact lines with dyadic steps
        for tag, (direction, step) in LINES.items():
            add(f"line_{tag}_k{k}", "line", np.array([0.5, -1.25, 2.0]) + (step * rng.permutation(np.arange(-k, k))[:k])[:, None] * direction, 6)
        add(f"coincident_k{k}", "identity", np.tile(np.array([[1.5, -2.0, 0.25]]), (k, 1)), 7)
        # the same noisy patch (1 mm, 0.2 m) ever farther from the origin; and one patch at three power-of-two scales
        patch = _patch(rng, k)
        for dist in DISTANCES:
            add(f"translate{int(dist)}_k{k}", f"translate{int(dist)}", patch + dist * AWAY, 8)
        patch = _patch(rng, k)
        for e in (-20, 0, 20):
            add(f"scale{e:+d}_k{k}", "scale", patch * 2.0**e, 9)
    tetra = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    add("tetrahedron_k4", "identity", 0.5 * tetra + [2.0, -1.0, 0.5], 10)
    cube = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
    add("cube_k8", "identity", 0.25 * cube + [-1.0, 3.0, 0.5], 11)
    return cases


def exact(points, digits=50):
    """``(unit normal (3,), eigenvalues (3,) ascending)`` of the covariance of ``points``: two passes in mpmath"""
    import mpmath

    with mpmath.workdps(digits):
        k = points.shape[0]
        p = [[mpmath.mpf(float(c)) for c in row] for row in points]
        mean = [sum(row[a] for row in p) / k for a in range(3)]
        cov = mpmath.matrix(3, 3)
        for a in range(3):
            for b in range(3):
                cov[a, b] = sum((row[a] - mean[a]) * (row[b] - mean[b]) for row in p) / (k - 1)
        values, vectors = mpmath.eigsy(cov)
        order = sorted(range(3), key=lambda i: values[i])
        n = [vectors[a, order[0]] for a in range(3)]
        norm = mpmath.sqrt(sum(c * c for c in n))
        big = max(range(3), key=lambda a: abs(n[a]))
        sign = -1 if n[big] < 0 else 1
        return np.array([float(sign * c / norm) for c in n]), np.array([float(values[i]) for i in order])


def generate():
    """The file's arrays as a dict"""
    cases = build_cases()
    c = len(cases)
    out = {"names": np.array([name for name, _, _, _ in cases]), "groups": np.array([g for _, g, _, _ in cases]), "k": np.array([p.shape[0] for _, _, p, _ in cases], dtype=np.int32),
           "points": np.zeros((c, MAX_POINTS, 3)), "lists": np.full((c, MAX_POINTS), -1, dtype=np.int32), "normal": np.zeros((c, 3)), "eigenvalues": np.zeros((c, 3))}
    for i, (_, _, pts, lst) in enumerate(cases):
        k = pts.shape[0]
        out["points"][i, :k], out["lists"][i, :k] = pts, lst
        out["normal"][i], out["eigenvalues"][i] = exact(pts)
    return out


if __name__ == "__main__":
    arrays = generate()
    np.savez_compressed(PATH, **arrays)
    print(f"wrote {PATH}: {arrays['names'].shape[0]} cases, {os.path.getsize(PATH)} bytes")
