"""Host oracle of the voxel integrator (test infrastructure): the loop of StaticPointCloudIntegrator::insert_points as described
in include/nidreg.h -- a Python dict keyed by ``tuple(floor(p / res))``, overwritten in input order, behind the
``norm < min_distance`` gate --, plus the sequence numbers the GPU side orders its output by."""
import numpy as np


class Integrator:
    def __init__(self, voxel_resolution, min_distance):
        self.res, self.min_distance = float(voxel_resolution), float(min_distance)
        self.grid = {}  # voxel -> (sequence number, x, y, z, intensity)
        self.offered = 0

    def insert(self, points, intensities):
        """points (n, >= 3) and intensities (n,) of any float type; computed in float64"""
        pts = np.asarray(points, dtype=np.float64)[:, :3]
        inten = np.asarray(intensities, dtype=np.float64)
        x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
        keep = ~(np.sqrt(x * x + y * y + z * z) < self.min_distance)
        vox = np.floor(pts / self.res)
        for i in np.flatnonzero(keep):
            self.grid[(vox[i, 0], vox[i, 1], vox[i, 2])] = (self.offered + int(i), pts[i, 0], pts[i, 1], pts[i, 2], inten[i])
        self.offered += pts.shape[0]
        return int(keep.sum())

    def size(self):
        return len(self.grid)

    def winners(self):
        """``(records (m, 4) float32, seq (m,) int64, voxels (m, 3) int64)`` in ascending sequence number: what
        nidreg_integrator_get returns, and the voxels the entries stand for"""
        items = sorted(self.grid.items(), key=lambda kv: kv[1][0])
        rec = np.array([v[1:] for _, v in items], dtype=np.float64).reshape(-1, 4).astype(np.float32)
        seq = np.array([v[0] for _, v in items], dtype=np.int64)
        vox = np.array([k for k, _ in items], dtype=np.float64).reshape(-1, 3).astype(np.int64)
        return rec, seq, vox


def parity_input():
    """The parity case of tests/test_voxel_gpu.py: 5000 points uniform in [-2, 2)^3 with random intensities"""
    rng = np.random.default_rng(0)
    points = rng.uniform(-2, 2, (5000, 3))
    intensities = rng.uniform(0, 1, 5000)
    return points, intensities
