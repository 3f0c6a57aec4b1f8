"""GPU tests of the raw sensor_msgs/PointCloud2 ingest (nidreg_integrator_insert_cloud2, k_vox_decode_cloud2 of
csrc/nid_voxel_kernels.hpp) against the oracle of tests/preprocess_oracle.py, which is fed a numpy structured-dtype decode of the
same bytes with the finite filter applied.  Every comparison is EXACT: the same float32 records in the same order, and the winners'
sequence numbers equal to the RAW index of the point in the frames (skipped points take a number)."""
import ctypes

import numpy as np
import pytest

import preprocess_oracle
from direct_visual_lidar_calibration_amd import _lib, preprocess

RES, MIN_D = 0.25, 1.0
DATATYPE = {"u1": 2, "u2": 4, "u4": 6, "f4": 7, "f8": 8, "i1": 1, "i2": 3, "i4": 5}


def _dt(names, formats, offsets, itemsize):
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": itemsize})


# name -> (record dtype, intensity channel).  Records of up to 128 bytes are decoded from LDS, longer ones from global memory.
LAYOUTS = {
    "xyzi16": (_dt(["x", "y", "z", "intensity"], ["<f4"] * 4, [0, 4, 8, 12], 16), "intensity"),
    "u16_at_13_step18": (_dt(["x", "y", "z", "intensity", "ring"], ["<f4", "<f4", "<f4", "<u2", "<u2"], [1, 5, 9, 13, 15], 18), "intensity"),
    "u8_at_13_step22": (_dt(["x", "y", "z", "intensity", "timestamp"], ["<f4", "<f4", "<f4", "<u1", "<f8"], [0, 4, 8, 13, 14], 22), "intensity"),
    "ouster48": (_dt(["x", "y", "z", "intensity", "t", "reflectivity", "ring", "ambient", "range"], ["<f4", "<f4", "<f4", "<f4", "<u4", "<u2", "<u2", "<u2", "<u4"],
                     [0, 4, 8, 16, 20, 24, 26, 28, 32], 48), "reflectivity"),
    "f64_step40": (_dt(["x", "y", "z", "intensity"], ["<f8"] * 4, [0, 8, 16, 24], 40), "intensity"),
    "u32_intensity": (_dt(["x", "y", "z", "intensity"], ["<f4", "<f4", "<f4", "<u4"], [0, 4, 8, 12], 16), "intensity"),
    "step128_fields_at_both_ends": (_dt(["x", "y", "z", "intensity"], ["<f4"] * 4, [0, 60, 120, 124], 128), "intensity"),
    "step129_from_global": (_dt(["x", "y", "z", "intensity"], ["<f4", "<f4", "<f4", "<u1"], [113, 117, 121, 128], 129), "intensity"),
    "step300_from_global": (_dt(["intensity", "x", "y", "z"], ["<f8", "<f8", "<f8", "<f8"], [3, 11, 150, 292], 300), "intensity"),
}
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 4097]
_cache = {}


def make_records(layout, n, seed=0):
    """n records of the layout: points uniform in [-3, 3)^3 (13824 voxels of 0.25), intensities over the channel's whole range (a uint32 channel mostly
    above 2^24, where float32 no longer holds every integer), every other byte of the record random"""
    key = (layout, n, seed)
    if key not in _cache:
        dt, channel = LAYOUTS[layout]
        rng = np.random.default_rng([seed, n, sorted(LAYOUTS).index(layout)])
        rec = np.frombuffer(rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).tobytes(), dtype=dt).copy()
        for k in "xyz":
            rec[k] = rng.uniform(-3, 3, n)
        kind = dt.fields[channel][0]
        if kind.kind == "u":
            rec[channel] = rng.integers(0, 2 ** (8 * kind.itemsize), n, dtype=np.uint64)
            if kind.itemsize == 4 and n > 2:
                rec[channel][:3] = [2**24 + 1, 2**31 + 129, 2**32 - 1]
        else:
            rec[channel] = rng.uniform(0, 255, n)
        _cache[key] = rec
    return _cache[key].copy()


def message(rec, **over):
    dt = rec.dtype
    fields = [(name, dt.fields[name][1], DATATYPE[dt.fields[name][0].str[1:]], 1) for name in dt.names]
    msg = {"fields": fields, "point_step": dt.itemsize, "data": rec.tobytes(), "width": len(rec), "height": 1, "is_bigendian": 0}
    msg.update(over)
    return msg


def decode(rec, channel):
    """The host's decode: ``(points (n, 3) float64, intensities (n,) float64, finite mask)``"""
    pts = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float64)
    return pts, rec[channel].astype(np.float64), np.isfinite(pts).all(axis=1)


def expected(frames, res=RES, min_d=MIN_D):
    """``(records, raw sequence numbers, points skipped per frame)`` of ``frames`` = [(records, channel)]: the oracle on the decoded,
    filtered points; its sequence numbers count filtered points and are mapped back to raw indices over all frames"""
    filtered, masks = [], []
    for rec, channel in frames:
        pts, inten, ok = decode(rec, channel)
        filtered.append((pts[ok], inten[ok]))
        masks.append(ok)
    rec_o, seq_o, _, _ = preprocess_oracle.winners_numpy(filtered, res, min_d)
    raw = np.flatnonzero(np.concatenate(masks))
    return rec_o, raw[seq_o], [int((~m).sum()) for m in masks]


def assert_equals(integ, rec_o, seq_raw):
    rec = integ.get_records()
    assert rec.dtype == np.float32 and rec.shape == rec_o.shape
    assert np.array_equal(rec.view(np.uint32), rec_o.view(np.uint32))
    assert np.array_equal(integ.last_seq, seq_raw)
    return rec


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_every_layout_at_every_size_equals_the_oracle(layout):
    channel = LAYOUTS[layout][1]
    for n in SIZES:
        rec = make_records(layout, n)
        if n >= 63:
            rec["y"][n // 2] = np.nan  # one skipped point in the middle: the raw numbering differs from the filtered one
        integ = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
        skipped = integ.insert_cloud2(message(rec), channel)
        rec_o, seq_raw, want_skipped = expected([(rec, channel)])
        assert skipped == want_skipped[0] == (1 if n >= 63 else 0), n
        assert integ.info()["offered"] == n
        assert_equals(integ, rec_o, seq_raw)
        if n == 4097:
            assert 1000 < len(rec_o) < n  # voxels shared by several points: last insert wins is exercised
        integ.close()


@pytest.mark.gpu
def test_uint32_intensity_above_2_pow_24_rounds_as_float_of_double():
    rec = make_records("u32_intensity", 65)
    rec["x"][:3], rec["y"][:3], rec["z"][:3] = [3.0, 4.0, 5.0], 0.1, 0.1
    integ = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
    integ.insert_cloud2(message(rec), "intensity")
    got = integ.get_records()
    first3 = got[np.isin(integ.last_seq, [0, 1, 2])]
    assert np.array_equal(first3[:, 3], np.array([2**24 + 1, 2**31 + 129, 2**32 - 1], dtype=np.float64).astype(np.float32))
    assert first3[0, 3] == 16777216.0 and first3[2, 3] == 4294967296.0  # ties to even / up to 2^32: not the integer
    integ.close()


NONFINITE = [(axis, v) for axis in "xyz" for v in (np.nan, np.inf, -np.inf)]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["ouster48", "u16_at_13_step18", "f64_step40", "step129_from_global"])
def test_non_finite_coordinates_are_skipped_counted_and_numbered(layout):
    """NaN, +inf and -inf in each coordinate alone at the first, the last and the records around the 64-lane and 256-record tile
    boundaries; every one of the nine takes every one of the nine positions in turn"""
    channel = LAYOUTS[layout][1]
    n = 600
    positions = [0, 63, 64, 255, 256, 257, 511, 512, n - 1]
    frames = []
    integ = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
    for turn in range(9):
        rec = make_records(layout, n, seed=turn)
        for k, p in enumerate(positions):
            axis, v = NONFINITE[(k + turn) % 9]
            rec[axis][p] = v
        frames.append((rec, channel))
        assert integ.insert_cloud2(message(rec), channel) == 9
        assert integ.info()["offered"] == n * (turn + 1)
    rec_o, seq_raw, skipped = expected(frames)
    assert skipped == [9] * 9
    got = assert_equals(integ, rec_o, seq_raw)
    assert np.isfinite(got[:, :3]).all() and not np.isin(seq_raw % n, positions).any()
    integ.close()


@pytest.mark.gpu
def test_a_nan_intensity_on_a_finite_point_is_kept():
    rec = make_records("xyzi16", 65)
    rec["x"][[7, 64]], rec["y"][[7, 64]], rec["z"][[7, 64]] = [[5.1, -6.3]], 0.1, 0.1  # voxels of their own
    rec["intensity"][[7, 64]] = [np.nan, np.inf]
    integ = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
    assert integ.insert_cloud2(message(rec), "intensity") == 0
    rec_o, seq_raw, _ = expected([(rec, "intensity")])
    got = assert_equals(integ, rec_o, seq_raw)
    assert np.isnan(got[integ.last_seq == 7, 3]).all() and np.isinf(got[integ.last_seq == 64, 3]).all() and (integ.last_seq == 7).sum() == 1
    integ.close()


@pytest.mark.gpu
def test_points_on_the_distance_gate_and_on_voxel_faces():
    """Dyadic coordinates: every square, sum, quotient and root below is exact or correctly rounded on both sides, so the decisions
    are the same whatever the association of the norm's sum.  At the gate `norm < min_distance` skips: a point AT 1.0 stays."""
    below = np.nextafter(np.float32(1.0), np.float32(0.0))
    pts = [(1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (below, 0.0, 0.0), (0.0, 0.0, -below), (0.75, 0.5, 0.25), (0.5, 0.5, 0.5), (0.75, 0.75, 0.0),
           (2.0, 2.0, 2.0), (np.nextafter(np.float32(2.0), np.float32(0.0)), 2.0, 2.0), (-2.0, -2.25, 2.0), (np.nextafter(np.float32(-2.0), np.float32(-3.0)), -2.25, 2.0),
           (-0.25, -1.0, 0.0), (-0.0, 1.25, -0.0), (0.0, 1.25, 0.0), (1.75, 0.0, -0.25)]
    for layout in ("xyzi16", "f64_step40", "u8_at_13_step22"):
        dt, channel = LAYOUTS[layout]
        rec = np.zeros(len(pts), dtype=dt)
        rec["x"], rec["y"], rec["z"] = np.array(pts).T
        rec[channel] = np.arange(len(pts)) + 1
        integ = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
        integ.insert_cloud2(message(rec), channel)
        o = preprocess_oracle.Integrator(RES, MIN_D)
        p, w, _ = decode(rec, channel)
        assert o.insert(p, w) == 12  # the two just inside the gate, (0.75, 0.5, 0.25) (norm^2 0.875) and (0.5, 0.5, 0.5) (0.75) are skipped
        rec_o, seq_o, vox_o = o.winners()
        assert_equals(integ, rec_o, seq_o)
        assert [3, 4, 5, 6] == sorted(set(range(len(pts))) - set(seq_o.tolist()) - {13})  # (13 and 14 share the voxel of -0.0 / +0.0: 14 wins)
        assert (vox_o[seq_o == 8] == [8, 8, 8]).all() and (vox_o[seq_o == 9] == [7, 8, 8]).all() and (vox_o[seq_o == 10] == [-8, -9, 8]).all() and (vox_o[seq_o == 11] == [-9, -9, 8]).all()
        integ.close()


@pytest.mark.gpu
def test_a_frame_with_an_out_of_range_voxel_inserts_nothing():
    integ = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
    first = make_records("ouster48", 300)
    integ.insert_cloud2(message(first), "reflectivity")
    before = (integ.get_records().copy(), integ.last_seq.copy(), integ.info())
    bad = make_records("ouster48", 700, seed=1)
    bad["x"][5], bad["z"][699] = np.nan, np.inf  # skipped points do not refuse a frame ...
    bad["y"][300] = 262144.0  # ... a finite point at voxel 2^20 does
    with pytest.raises(ValueError, match="outside the packed-key limit.*nothing was inserted"):
        integ.insert_cloud2(message(bad), "reflectivity")
    assert np.array_equal(integ.get_records().view(np.uint32), before[0].view(np.uint32)) and np.array_equal(integ.last_seq, before[1]) and integ.info() == before[2]
    bad["y"][300] = np.nextafter(np.float32(262144.0), np.float32(0.0))  # voxel 2^20 - 1: accepted
    assert integ.insert_cloud2(message(bad), "reflectivity") == 2
    rec_o, seq_raw, _ = expected([(first, "reflectivity"), (bad, "reflectivity")])
    assert_equals(integ, rec_o, seq_raw)
    assert 300 + 300 in seq_raw
    integ.close()


def _three_frames():
    frames = []
    for k, (layout, n) in enumerate((("ouster48", 1500), ("u16_at_13_step18", 700), ("f64_step40", 1300))):
        rec = make_records(layout, n, seed=10 + k)
        rec["x"][[0, n - 1]], rec["z"][n // 3] = np.nan, -np.inf
        frames.append((rec, LAYOUTS[layout][1]))
    return frames


@pytest.mark.gpu
def test_three_frames_equal_one_host_route_insert_of_their_filtered_concatenation():
    frames = _three_frames()
    integ = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
    for rec, channel in frames:
        assert integ.insert_cloud2(message(rec), channel) == 3
    got, got_seq = integ.get_records(), integ.last_seq
    decoded = [decode(rec, channel) for rec, channel in frames]
    pts = np.concatenate([p[ok] for p, _, ok in decoded])
    inten = np.concatenate([w[ok] for _, w, ok in decoded])
    host = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
    host.insert_points(pts, inten)
    assert np.array_equal(got.view(np.uint32), host.get_records().view(np.uint32))  # records and order
    raw = np.flatnonzero(np.concatenate([ok for _, _, ok in decoded]))
    assert np.array_equal(got_seq, raw[host.last_seq]) and not np.array_equal(got_seq, host.last_seq)  # only the numbering differs, predictably
    rec_o, seq_raw, _ = expected(frames)
    assert np.array_equal(got.view(np.uint32), rec_o.view(np.uint32)) and np.array_equal(got_seq, seq_raw)
    assert integ.info()["offered"] == 3500 and host.info()["offered"] == 3500 - 9
    integ.close(), host.close()


@pytest.mark.gpu
def test_two_runs_give_the_same_bytes():
    out = []
    for _ in range(2):
        integ = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
        for rec, channel in _three_frames():
            integ.insert_cloud2(message(rec), channel)
        out.append((integ.get_records().tobytes(), integ.last_seq.tobytes()))
        integ.close()
    assert out[0] == out[1]


@pytest.mark.gpu
def test_a_frame_across_the_integrators_chunk_edge():
    """2^20 + 65 records of 48 bytes: the claim / payload passes run in two chunks, the second numbered from offered + 2^20"""
    n = (1 << 20) + 65
    rec = make_records("ouster48", n)
    edge = [0, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, n - 1]
    rec["x"][edge] = np.nan
    warm = make_records("ouster48", 100, seed=5)
    integ = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
    integ.insert_cloud2(message(warm), "reflectivity")
    assert integ.insert_cloud2(message(rec), "reflectivity") == 5
    rec_o, seq_raw, _ = expected([(warm, "reflectivity"), (rec, "reflectivity")])
    assert_equals(integ, rec_o, seq_raw)
    assert (seq_raw >= 100 + (1 << 20)).sum() > 30 and integ.info()["offered"] == n + 100
    integ.close()


@pytest.mark.gpu
def test_invalid_arguments_are_refused_before_the_device_is_touched():
    """``data`` is an address that must not be read (no mapping at 16): every call below returns NIDREG_ERR_INVALID from the argument
    checks, which come before the upload"""
    lib = _lib.load()
    integ = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
    integ.insert_cloud2(message(make_records("xyzi16", 10)), "intensity")
    before = integ.info()
    skipped = ctypes.c_int64(-5)
    unreadable = ctypes.c_void_p(16)

    def call(data=unreadable, n=100, step=16, ox=0, oy=4, oz=8, xyz=7, oi=12, it=7, h=None):
        return lib.nidreg_integrator_insert_cloud2(integ._h if h is None else h, data, n, step, ox, oy, oz, xyz, oi, it, ctypes.byref(skipped))

    bad = [dict(ox=13), dict(oy=14), dict(oz=16), dict(ox=-1), dict(oi=13), dict(oi=-4), dict(oi=15, it=4), dict(oi=16, it=2), dict(oi=9, it=8), dict(xyz=8, oz=9),
           dict(step=0), dict(step=-16), dict(step=65536), dict(xyz=6), dict(xyz=0), dict(xyz=2), dict(it=1), dict(it=3), dict(it=5), dict(it=0), dict(it=9),
           dict(data=None), dict(n=-1), dict(n=-1, data=None), dict(n=2**62)]
    for kw in bad:
        assert call(**kw) == _lib.NIDREG_ERR_INVALID, kw
        assert "nidreg_integrator_insert_cloud2" in _lib.last_error() and skipped.value == 0
    assert lib.nidreg_integrator_insert_cloud2(None, unreadable, 100, 16, 0, 4, 8, 7, 12, 7, None) == _lib.NIDREG_ERR_INVALID
    # the edges that ARE valid: fields that end with the record, the largest step; n == 0 is a no-op (with any data pointer)
    assert call(n=0) == 0 and call(n=0, data=None) == 0 and call(n=0, step=65535, oi=65534, it=2, xyz=8, ox=0, oy=8, oz=65527) == 0
    assert call(n=0, ox=13) == _lib.NIDREG_ERR_INVALID  # (the layout is checked whatever n)
    assert integ.info() == before
    # the Python wrapper's own refusals
    rec = make_records("xyzi16", 10)
    mixed = message(rec)
    mixed["fields"] = [("x", 0, 7, 1), ("y", 4, 8, 1), ("z", 8, 7, 1), ("intensity", 12, 7, 1)]
    for msg, channel, what in ((mixed, "intensity", "different datatypes"), (message(rec), "reflectivity", "no 'reflectivity' field"), (message(rec, is_bigendian=1), "intensity", "big-endian"),
                               (message(rec, width=11), "intensity", "160 data bytes for 11 points"), (message(rec, fields=[("x", 0, 7, 1), ("y", 4, 7, 1), ("intensity", 12, 7, 1)]), "intensity", "no 'z' field")):
        with pytest.raises(ValueError, match=what):
            integ.insert_cloud2(msg, channel)
    assert integ.info() == before
    integ.close()
