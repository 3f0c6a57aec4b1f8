"""The LRU eviction of iVox (src/vlcal/common/ivox.cpp:144-178, :223) on top of the CPU restatement of tests/odometry_oracle.py (test
infrastructure, not a test).  ``IVoxLRU`` adds to ``IVox`` the insert count, the stamp a voxel gets when a scan offers it a point and
when a search finds it, and the erase rule; ``NumpyBackendLRU`` is ``NumpyBackend`` over it, for ``odometry.ScanMatcher``.

It is the yardstick of tests/test_odometry_lru_gpu.py.  Like the rest of that module it is written from the reference's sources;
UNLIKE the NID oracle it is UNPINNED against a compiled ``ivox.cpp`` (no recipe under oracle/ builds it).  Not restated: the "too
many voxels" branch (:181-197), which takes 2^32 - 1 voxels.
"""
import numpy as np

from odometry_oracle import AXIS_LIMIT, OFFSETS, IVox, NumpyBackend


class IVoxLRU(IVox):
    """``iVox(resolution, insertion_dist_thresh, lru_thresh)`` with ``lru_cycle`` (ivox.cpp:55: 10): ``lru_thresh=0`` never erases"""

    def __init__(self, resolution=1.0, insertion_dist_thresh=0.05, lru_thresh=100, lru_cycle=10):
        super().__init__(resolution, insertion_dist_thresh)
        self.lru_thresh, self.lru_cycle = int(lru_thresh), int(lru_cycle)
        self.lru_count = 0
        self.stamps = {}  # voxel -> LinearContainer::last_lru_count
        self.evicted = []  # per insert: the voxels it erased, with the number of points each held
        self.created = []  # per insert: the voxels it created

    def insert(self, points, covs):
        self.lru_count += 1  # :144
        created = []
        for i in range(points.shape[0]):  # :147
            key = tuple(int(v) for v in np.floor(points[i] / self.res))  # :149
            if key not in self.voxels:  # :151-154
                self.voxels[key] = ([], [])
                created.append(key)
            pts, cvs = self.voxels[key]
            self.stamps[key] = self.lru_count  # :164 -- before the point is tested: a refused point refreshes its voxel too
            if pts:  # :165, LinearContainer::insert :29-50
                d = np.asarray(pts) - points[i]
                if ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).min() <= self.thresh_sq:
                    continue
            pts.append(points[i].copy())
            cvs.append(covs[i].copy())
        erased = []
        horizon = self.lru_count - self.lru_thresh  # :169
        if self.lru_thresh > 0 and horizon > 0 and self.lru_count % self.lru_cycle == 0:  # :170 (lru_thresh = 0: the project's "off")
            for key in list(self.voxels):  # :171
                if self.stamps[key] < horizon:  # :172 -- strictly: a voxel at the horizon stays
                    erased.append((key, len(self.voxels[key][0])))
                    del self.voxels[key], self.stamps[key]  # :173
        self.created.append(created)
        self.evicted.append(erased)
        self._flat = None

    def nearest(self, q):
        """``IVox.nearest``, and every voxel among the 7 that is inside the key range and present is stamped (:217-223) -- whether
        or not one of its points becomes the nearest, and whatever the caller then does with the distance"""
        out = super().nearest(q)
        with np.errstate(invalid="ignore"):
            fc = np.floor(q / self.res)  # :209
        sane = np.all(np.isfinite(fc) & (fc >= -AXIS_LIMIT - 1) & (fc <= AXIS_LIMIT), axis=1)
        centre = fc[sane].astype(np.int64)
        for off in OFFSETS:  # :215
            v = centre + np.asarray(off, dtype=np.int64)[None]  # :216
            v = v[np.all((v >= -AXIS_LIMIT) & (v < AXIS_LIMIT), axis=1)]
            for key in {tuple(int(c) for c in row) for row in np.unique(v, axis=0)} if v.shape[0] else ():
                if key in self.voxels:  # :217-220
                    self.stamps[key] = self.lru_count  # :223
        return out


class NumpyBackendLRU(NumpyBackend):
    """``odometry.DeviceBackend(lru_thresh=..., lru_cycle=...)``'s methods on the CPU"""

    def __init__(self, lru_thresh=100, lru_cycle=10):
        super().__init__()
        self.model = IVoxLRU(lru_thresh=lru_thresh, lru_cycle=lru_cycle)


# ---- a hand-worked schedule, shared by the host test of this module and the GPU test of the device ---------------------------------
# lru_thresh = 2, lru_cycle = 3: a pass runs after inserts 3 and 6, with horizons 1 and 4.  Voxels lie 3 m apart on the x axis, so a
# search in one finds no other.  Per step: ("insert", points) or ("search", queries), and the voxels (x index) that exist after it.
def _at(x, dx=0.5):
    return [x + dx, 0.5, 0.5]


A, B, H, C, D, E, F, G = 0, 3, 6, 9, 12, 15, 18, 21
RULE_EDGES_THRESH, RULE_EDGES_CYCLE = 2, 3
RULE_EDGES = [
    ("insert", [_at(A), _at(B), _at(H)], {A, B, H}),  # 1: stamps A1 B1 H1
    ("insert", [_at(C)], {A, B, H, C}),  # 2: C2; the horizon is 0: no pass looks
    ("insert", [_at(D)], {A, B, H, C, D}),  # 3: D3; the pass runs with horizon 1: A, B and H sit exactly AT it and stay
    ("insert", [_at(E), _at(A, 0.53)], {A, B, H, C, D, E}),  # 4: E4, and A4 by a point 3 cm from A's, which is refused; horizon 2, B and
    #                                                             H are stale, but 4 % 3 != 0: no pass
    ("search", [_at(B, 0.4)], {A, B, H, C, D, E}),  # B4 by a search alone
    ("insert", [_at(F)], {A, B, H, C, D, E, F}),  # 5: F5; horizon 3, 5 % 3 != 0: no pass, with H and C stale
    ("insert", [_at(G)], {A, B, E, F, G}),  # 6: G6; the pass runs with horizon 4: H1 C2 D3 leave, A4 B4 E4 (at the horizon) F5 G6 stay
]
RULE_EDGES_POINTS_AT_END = 5  # one point per surviving voxel: A's refused point never entered
