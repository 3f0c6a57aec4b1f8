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


def winners_numpy(frames, voxel_resolution, min_distance):
    """The dict oracle restated in numpy for the large cases: ``frames`` is a sequence of ``(points, intensities)`` inserted in
    that order.  The same gate and the same ``floor(p / res)`` in float64; the winner of a voxel is its LAST occurrence (the first
    row ``np.unique`` meets in the reversed array).  Returns ``(records, seq, voxels, offered)``, the first three as
    ``Integrator.winners()``.  (Voxel rows are compared as int64, so -0.0 and +0.0 are one voxel as they are one dict key; the
    quotients of an accepted frame are far inside int64.)"""
    pts = np.concatenate([np.asarray(p, dtype=np.float64)[:, :3] for p, _ in frames])
    inten = np.concatenate([np.asarray(w, dtype=np.float64).reshape(-1) for _, w in frames])
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    seq = np.flatnonzero(~(np.sqrt(x * x + y * y + z * z) < float(min_distance)))
    vox = np.floor(pts[seq] / float(voxel_resolution)).astype(np.int64)
    if len(seq):
        # one int64 per voxel row, row-major inside the bounding box of the occupied voxels (a 1-D unique sorts several times
        # faster than a row-wise one); a box too large for that goes through the row-wise unique
        lo, ext = vox.min(axis=0), [int(e) for e in vox.max(axis=0) - vox.min(axis=0) + 1]
        if ext[0] * ext[1] * ext[2] < 2**62:
            d = vox - lo
            rows = ((d[:, 0] * ext[1] + d[:, 1]) * ext[2] + d[:, 2])[::-1]
            _, first = np.unique(rows, return_index=True)
        else:
            _, first = np.unique(vox[::-1], axis=0, return_index=True)
        win = np.sort(len(seq) - 1 - first)
    else:
        win = np.zeros(0, dtype=np.int64)
    seq = seq[win].astype(np.int64)
    rec = np.concatenate([pts[seq], inten[seq, None]], axis=1).astype(np.float32)
    return rec, seq, vox[win].reshape(-1, 3), int(pts.shape[0])


# ---- the table of csrc/nid_voxel_kernels.hpp restated (white-box tests of the probing): the packed key and where probing starts


def packed_key(vox):
    """``vox_classify``'s key of integer voxels (m, 3): 21 bits per axis, index + 2^20, x lowest, stored + 1 (0 = empty slot)"""
    v = (np.asarray(vox, dtype=np.int64) + (1 << 20)).astype(np.uint64)
    return (v[:, 0] | (v[:, 1] << np.uint64(21)) | (v[:, 2] << np.uint64(42))) + np.uint64(1)


def vox_mix(key):
    """``vox_mix``: splitmix64's finaliser WITHOUT the additive constant (``pose_mix`` of the RANSAC sampler has it), mod 2^64"""
    z = np.asarray(key, dtype=np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def home_slot(vox, capacity):
    """where ``vox_find_or_claim`` starts probing in a table of ``capacity`` (a power of two) slots"""
    return ((vox_mix(packed_key(vox)) & np.uint64(0xFFFFFFFF)) & np.uint64(capacity - 1)).astype(np.int64)


def linear_probe(homes, capacity):
    """Final slot of every key (distinct keys, inserted in the given order) under ``h = (h + 1) & mask`` probing"""
    used = np.zeros(capacity, dtype=bool)
    out = np.empty(len(homes), dtype=np.int64)
    for n, h in enumerate(homes.tolist()):
        while used[h]:
            h = (h + 1) & (capacity - 1)
        used[h] = True
        out[n] = h
    return out


def parity_input():
    """The parity case of tests/test_voxel_gpu.py: 5000 points uniform in [-2, 2)^3 with random intensities"""
    rng = np.random.default_rng(0)
    points = rng.uniform(-2, 2, (5000, 3))
    intensities = rng.uniform(0, 1, 5000)
    return points, intensities
