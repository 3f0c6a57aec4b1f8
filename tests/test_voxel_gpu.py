"""GPU tests of the voxel integrator (nidreg_integrator_*, csrc/nid_voxel_kernels.hpp) against the dict oracle of
tests/preprocess_oracle.py.  Every comparison is EXACT: the same set of voxels, the same float32 record per voxel, the same winner
sequence numbers, the records in ascending sequence number.  The inputs are chosen so that the oracle is unambiguous whatever the
division or FMA choices (the CPU test below says how far every decision is from its boundary)."""
import ctypes

import numpy as np
import pytest

import preprocess_oracle
from direct_visual_lidar_calibration_amd import _lib, preprocess

RES, MIN_D = 0.25, 1.0
_parity = {}


def parity_oracle():
    if not _parity:
        points, intensities = preprocess_oracle.parity_input()
        o = preprocess_oracle.Integrator(RES, MIN_D)
        kept = o.insert(points, intensities)
        _parity.update(points=points, intensities=intensities, kept=kept, oracle=o, winners=o.winners())
    return _parity


def assert_equals_oracle(integ, oracle):
    rec_o, seq_o, _ = oracle.winners()
    assert integ.size() == oracle.size()
    rec = integ.get_records()
    assert rec.dtype == np.float32 and rec.shape == rec_o.shape
    assert np.array_equal(integ.last_seq, seq_o)
    assert np.array_equal(rec.view(np.uint32), rec_o.view(np.uint32))
    return rec


def test_the_parity_input_is_unambiguous():
    """(CPU) The oracle keeps 4654 points in 2716 voxels; no point is within 1.3e-3 of the distance gate and no quotient within
    3e-6 of an integer, so neither the association of the norm's sum nor a last-place difference in the division moves a point."""
    c = parity_oracle()
    p = c["points"]
    assert c["kept"] == 4654 and c["oracle"].size() == 2716
    gate = np.abs(np.linalg.norm(p, axis=1) - MIN_D).min()
    q = p / RES
    frac = np.abs(q - np.rint(q)).min()
    print(f"closest to the gate {gate:.3e}, closest quotient to an integer {frac:.3e}")
    assert gate > 1.3e-3 and frac > 3e-6


@pytest.mark.gpu
def test_parity_with_the_oracle_double_and_float_routes():
    c = parity_oracle()
    integ = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
    integ.insert_points(c["points"], c["intensities"])
    rec = assert_equals_oracle(integ, c["oracle"])
    _, _, vox_o = c["winners"]
    assert np.array_equal(np.floor(c["points"][integ.last_seq] / RES).astype(np.int64), vox_o)  # the same set of voxels
    pts, inten = integ.get_points()
    assert pts.shape == (2716, 3) and inten.shape == (2716,) and np.array_equal(pts, rec[:, :3]) and np.array_equal(inten, rec[:, 3])
    # homogeneous (n, 4) points take the same route
    i4 = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
    i4.insert_points(np.concatenate([c["points"], np.ones((5000, 1))], axis=1), c["intensities"])
    assert np.array_equal(i4.get_records().view(np.uint32), rec.view(np.uint32))
    i4.close()
    integ.close()

    # the float32 route fed float32(points) == the double route fed those values widened == the oracle on them
    p32, w32 = c["points"].astype(np.float32), c["intensities"].astype(np.float32)
    o32 = preprocess_oracle.Integrator(RES, MIN_D)
    o32.insert(p32, w32)
    results = []
    records16 = np.concatenate([p32, w32[:, None]], axis=1)  # the stored 16-byte record: uploaded as it lies
    for points, intensities in ((p32, w32), (records16[:, :3], records16[:, 3]), (p32.astype(np.float64), w32.astype(np.float64))):
        g = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
        g.insert_points(points, intensities)
        results.append((assert_equals_oracle(g, o32), g.last_seq))
        g.close()
    for rec_k, seq_k in results[1:]:
        assert np.array_equal(rec_k.view(np.uint32), results[0][0].view(np.uint32)) and np.array_equal(seq_k, results[0][1])


@pytest.mark.gpu
def test_floor_not_truncation():
    pts = np.array([[sx * 0.1, sy * 0.1, sz * 0.1] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    integ = preprocess.StaticPointCloudIntegrator(0.25, 0.0, device=0)
    integ.insert_points(pts, np.arange(8.0))
    o = preprocess_oracle.Integrator(0.25, 0.0)
    o.insert(pts, np.arange(8.0))
    rec = assert_equals_oracle(integ, o)
    assert integ.size() == 8  # (truncation would merge all eight into voxel 0 0 0)
    assert np.array_equal(o.winners()[2], np.where(pts < 0, -1, 0))
    assert np.array_equal(rec[:, 3], np.arange(8, dtype=np.float32))
    integ.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 65, 257])
def test_one_wave_one_voxel_the_last_point_wins(n):
    rng = np.random.default_rng(n)
    pts = np.array([2.0, 3.0, -1.0]) + 0.25 * rng.uniform(0.01, 0.99, (n, 3))  # all inside voxel (8, 12, -4)
    inten = np.arange(n, dtype=np.float64) + 0.5
    integ = preprocess.StaticPointCloudIntegrator(0.25, 0.0, device=0)
    integ.insert_points(pts, inten)
    rec = integ.get_records()
    assert integ.size() == 1 and integ.last_seq.tolist() == [n - 1]
    assert np.array_equal(rec[0], np.append(pts[-1], inten[-1]).astype(np.float32))
    integ.close()


@pytest.mark.gpu
def test_full_key_identity_on_axis_aligned_and_diagonal_voxels():
    """Voxels (+-k, 0, 0), (0, +-k, 0), (0, 0, +-k) and (k, k, -k), k = 1..300, one point at the centre of each: 2100 voxels.  A
    table that compares hashes (or a key that folds the axes together) merges some of them."""
    res = 0.05
    k = np.arange(1, 301)
    z = np.zeros(300, dtype=np.int64)
    vox = np.concatenate([np.stack(c, axis=1) for c in ((k, z, z), (z, k, z), (z, z, k), (-k, z, z), (z, -k, z), (z, z, -k), (k, k, -k))])
    pts = (vox + 0.5) * res
    inten = np.arange(len(pts), dtype=np.float64) / 4096.0
    perm = np.random.default_rng(3).permutation(len(pts))
    pts, inten, vox = pts[perm], inten[perm], vox[perm]
    o = preprocess_oracle.Integrator(res, 0.0)
    o.insert(pts, inten)
    assert o.size() == 2100 and np.array_equal(o.winners()[2], vox)
    integ = preprocess.StaticPointCloudIntegrator(res, 0.0, device=0)
    integ.insert_points(pts, inten)
    assert_equals_oracle(integ, o)
    integ.close()


@pytest.mark.gpu
def test_ragged_frames_growth_and_revisits():
    res, min_d = 0.05, 0.5
    rng = np.random.default_rng(5)
    o = preprocess_oracle.Integrator(res, min_d)
    integ = preprocess.StaticPointCloudIntegrator(res, min_d, device=0)
    cap0 = integ.info()["capacity"]
    for n in (0, 1, 63, 64, 65, 4097):
        pts, inten = rng.uniform(-1.5, 1.5, (n, 3)), rng.uniform(0, 1, n)
        integ.insert_points(pts, inten)
        o.insert(pts, inten)
        assert integ.size() == o.size(), n
    _, _, early_vox = o.winners()
    # 200 000 points on a lattice of 60 x 60 x 42 voxel centres (151 200 voxels, 48 800 of them visited twice), 4 m away
    i = np.arange(200000) % (60 * 60 * 42)
    vox = np.stack([i % 60 + 80, (i // 60) % 60 - 30, i // 3600 - 21], axis=1)
    pts, inten = (vox + 0.5) * res, rng.uniform(0, 1, 200000)
    integ.insert_points(pts, inten)
    o.insert(pts, inten)
    assert integ.size() == o.size() and o.size() > 150000
    info = integ.info()
    assert info["capacity"] > cap0 and info["capacity"] >= 2 * info["voxels"] and info["offered"] == o.offered
    # revisit 1000 of the earliest voxels (at their centres) with new intensities
    pick = early_vox[np.linalg.norm((early_vox + 0.5) * res, axis=1) > min_d + 0.1][:1000]
    assert len(pick) == 1000
    pts, inten = (pick + 0.5) * res, 2.0 + rng.uniform(0, 1, 1000)
    assert (np.linalg.norm(pts, axis=1) > min_d + 1e-3).all()
    size_before = integ.size()
    integ.insert_points(pts, inten)
    o.insert(pts, inten)
    assert integ.size() == o.size() == size_before
    rec = assert_equals_oracle(integ, o)
    assert np.array_equal(rec[-1000:, 3], inten.astype(np.float32)) and (rec[:-1000, 3] < 2.0).all()
    integ.close()


@pytest.mark.gpu
def test_refusals_leave_the_integrator_unchanged():
    lib = _lib.load()
    c = parity_oracle()
    integ = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
    integ.insert_points(c["points"][:1000], c["intensities"][:1000])
    size, rec, seq = integ.size(), integ.get_records(), integ.last_seq
    far = c["points"][1000:1100].copy()
    far[57, 1] = 2.0**20 * RES + 1.0
    nan = c["points"][1000:1100].copy()
    nan[3, 2] = np.nan
    for bad in (far, nan, far.astype(np.float32), nan.astype(np.float32)):
        inten = np.zeros(100, dtype=bad.dtype)
        with pytest.raises(ValueError, match="1048576"):
            integ.insert_points(bad, inten)
        assert "1048576" in _lib.last_error() and "nothing was inserted" in _lib.last_error()
        assert integ.size() == size and np.array_equal(integ.get_records().view(np.uint32), rec.view(np.uint32)) and np.array_equal(integ.last_seq, seq)
    # the status itself, through the C ABI
    inten = np.zeros(100)
    assert lib.nidreg_integrator_insert(integ._h, far.ctypes.data, 24, inten.ctypes.data, 100) == _lib.NIDREG_ERR_INVALID
    assert lib.nidreg_integrator_insert(integ._h, nan.ctypes.data, 24, inten.ctypes.data, 100) == _lib.NIDREG_ERR_INVALID
    assert lib.nidreg_integrator_insert(integ._h, far.ctypes.data, 24, inten.ctypes.data, -1) == _lib.NIDREG_ERR_INVALID
    assert lib.nidreg_integrator_insert_f32(integ._h, far.ctypes.data, 12, inten.ctypes.data, 4, -1) == _lib.NIDREG_ERR_INVALID
    # the last voxel inside the limit is accepted, and a refused frame does not advance the sequence numbers
    edge = np.array([[(2.0**20 - 0.5) * RES, 0.0, -(2.0**20) * RES]])
    integ.insert_points(edge, np.array([7.0]))
    assert integ.size() == size + 1
    integ.get_records()
    assert integ.last_seq[-1] == 1000
    integ.close()
    for res in (0.0, -0.25, float("nan"), float("inf")):
        h = ctypes.c_void_p()
        assert lib.nidreg_integrator_create(0, res, 1.0, ctypes.byref(h)) == _lib.NIDREG_ERR_INVALID and not h.value
        with pytest.raises(ValueError):
            preprocess.StaticPointCloudIntegrator(res, 1.0, device=0)


@pytest.mark.gpu
def test_run_to_run_identical_bytes():
    c = parity_oracle()
    out = []
    for _ in range(2):
        integ = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
        integ.insert_points(c["points"], c["intensities"])
        out.append(integ.get_records().tobytes() + integ.last_seq.tobytes())
        integ.close()
    assert out[0] == out[1]
