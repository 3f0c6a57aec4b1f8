"""GPU tests of nidreg_velodyne_decode (csrc/nid_packet_kernels.hpp) against the numpy restatement tests/velodyne_oracle.py: the records
must be the oracle's BYTE FOR BYTE (compared as uint32, so the NaNs of the no-return records count), and the per-packet return counts the
oracle's.  The shapes are the smallest at which the kernel can go wrong: one packet and three, the two strides of the messages from an odd
address, azimuths that wrap between two blocks and into the last one, wrong flags, the extreme field values, both layouts with every
slot populated, a calibration with every correction non-zero, packet times off the float32 grid, and a change of table between calls."""
import math

import numpy as np
import pytest

import velodyne_oracle as vo
from direct_visual_lidar_calibration_amd import lidar_messages

pytestmark = pytest.mark.gpu


def _model(name):
    table, res, firing, laser = vo.model(name)
    return lidar_messages.VelodyneModel(name, table, res, firing, laser)


def _calibrated(n, seed):
    """Every correction non-zero, different for every laser"""
    rng = np.random.default_rng(seed)
    table = vo.laser_table(rng.uniform(-0.5, 0.3, n), rng.uniform(-0.1, 0.1, n), rng.uniform(-0.02, 0.02, n), rng.uniform(-0.03, 0.03, n), rng.uniform(-0.2, 0.4, n))
    assert np.all(table[:, :7] != 0.0)
    return lidar_messages.VelodyneModel("calibrated", table, 0.004 if n == 16 else 0.002, *vo.periods(n))


def _random_packets(n, seed, product_id=0x22):
    rng = np.random.default_rng(seed)
    packets = []
    for p in range(n):
        start, step = int(rng.integers(0, 36000)), int(rng.integers(0, 60))
        packets.append(vo.encode_packet([(start + b * step) % 36000 for b in range(12)], rng.integers(1, 65536, (12, 32)), rng.integers(0, 256, (12, 32)), device_time=p, product_id=product_id))
    return packets


def _assert_equal(packets, stride, lead, times, model):
    buf, view = vo.place_packets(packets, stride, lead)
    if lead:
        assert view.ctypes.data % 2 == 1
    want, want_counts = vo.decode(view, stride, times, model.table, model.distance_resolution, model.firing_period, model.laser_period)
    got, counts = lidar_messages.velodyne_decode(view, len(packets), stride, times, model, returns=True)
    assert got.shape == want.shape == (384 * len(packets), 5) and got.dtype == np.float32
    diff = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert diff.size == 0, (diff[:5], got[diff[:5]], want[diff[:5]])
    assert np.array_equal(counts, want_counts)
    without = lidar_messages.velodyne_decode(view, len(packets), stride, times, model)  # returns_per_packet = NULL
    assert np.array_equal(without.view(np.uint32), want.view(np.uint32))
    return want, want_counts


@pytest.mark.parametrize("name,product_id", [("vlp16", 0x22), ("hdl32e", 0x21)])
def test_one_packet_with_every_slot_populated(name, product_id):
    want, counts = _assert_equal(_random_packets(1, 1, product_id), 1206, 0, [0.0], _model(name))
    assert counts.tolist() == [384] and np.isfinite(want).all()  # every laser's row of the table was read


@pytest.mark.parametrize("stride", [1214, 1216])
@pytest.mark.parametrize("name", ["vlp16", "hdl32e"])
def test_three_packets_at_the_message_strides_from_an_odd_address(stride, name):
    # packet times that are no multiples of a float32 ulp: the sum is rounded once, from double
    times = [0.0, 0.001327 + 1e-11, 0.0026541234567]
    assert all(float(np.float32(t)) != t for t in times[1:])
    want, _ = _assert_equal(_random_packets(3, 2 + stride), stride, 1, times, _model(name))
    assert len(np.unique(want[:, 4])) > 60


def test_azimuths_that_wrap_and_the_reused_last_difference():
    rng = np.random.default_rng(3)
    wrap_mid = [35910, 35930, 35950, 35970, 35990, 10, 30, 50, 70, 90, 110, 130]  # 35990 -> 10 between blocks 4 and 5
    wrap_last = [35790 + 20 * b for b in range(11)] + [10]  # 35990 -> 10 between blocks 10 and 11: diff[11] reuses diff[10] = 20
    assert wrap_last[10] == 35990
    uneven = [100, 140, 141, 164, 188, 228, 35999, 0, 23, 47, 87, 88]  # the differences 40, 1, 23, 24, 40, ... with their exact halves
    packets = [vo.encode_packet(az, rng.integers(1, 65536, (12, 32)), rng.integers(0, 256, (12, 32))) for az in (wrap_mid, wrap_last, uneven)]
    for name in ("vlp16", "hdl32e"):
        _assert_equal(packets, 1214, 0, [0.0, 0.001, 0.002], _model(name))


def test_wrong_flags_and_extreme_fields():
    rng = np.random.default_rng(4)
    az = [100 * b for b in range(12)]
    dist = rng.integers(1, 65536, (12, 32))
    refl = rng.integers(0, 256, (12, 32))
    dist[0, :6], refl[0, :6] = [0, 1, 65535, 0, 1, 65535], [0, 0, 0, 255, 255, 255]
    dist[7, 16:22], refl[7, 16:22] = [0, 1, 65535, 0, 1, 65535], [255, 255, 255, 0, 0, 0]
    flags_mid, flags_last = [0xEEFF] * 12, [0xEEFF] * 12
    flags_mid[5], flags_last[11] = 0xDDFF, 0xFFEE  # (0xDDFF: the HDL-64E's lower block; 0xFFEE: the right bytes, swapped)
    packets = [vo.encode_packet(az, dist, refl, flags=flags_mid), vo.encode_packet(az, dist, refl, flags=flags_last), vo.encode_packet(az, dist, refl)]
    for name in ("vlp16", "hdl32e"):
        want, counts = _assert_equal(packets, 1216, 1, [0.0, 0.5, 1.0], _model(name))
        assert counts.tolist() == [384 - 32 - 4, 384 - 32 - 4, 384 - 4]
        block5 = want[5 * 32 : 6 * 32]
        assert np.isnan(block5[:, :3]).all() and not block5[:, 3].any() and np.isfinite(block5[:, 4]).all()  # the time is still written
        assert np.isnan(want[384 + 11 * 32 : 2 * 384, :3]).all()
        # the neighbours of the unflagged block still interpolate over its azimuth field: the flags play no part in diff
        assert np.isfinite(want[4 * 32 : 5 * 32, :3]).all()
        assert want[2 * 384 + 2, 3] == 0.0 and want[2 * 384 + 5, 3] == 255.0 and np.isfinite(want[2 * 384 + 2, :3]).all()


def test_azimuth_fields_above_35999_decode_as_the_oracle_does():
    """An azimuth field is any uint16: a corrupted or unflagged block may hold 36000..65535.  The rule's modulo is the floored one, so
    diff and the table index stay in [0, 35999] -- a[10] = 65535 before a[11] = 0 makes a[b+1] - a[b] + 36000 negative -- and such a packet
    decodes deterministically, as the oracle decodes it"""
    rng = np.random.default_rng(8)
    reviewer = [100 * b for b in range(10)] + [65535, 0]          # diff[10] = (0 - 65535 + 36000) mod 36000 = 6465, reused by block 11
    descending = [65535, 0, 65535, 36000, 35999, 36001, 0, 65535, 40000, 50000, 36000, 65535]
    high = [int(v) for v in rng.integers(36000, 65536, 12)]
    packets = [vo.encode_packet(az, rng.integers(1, 65536, (12, 32)), rng.integers(0, 256, (12, 32))) for az in (reviewer, descending, high)]
    a = np.array(reviewer)
    assert (a[11] - a[10] + 36000) < -36000 + 36000 and (a[11] - a[10] + 36000) % 36000 == 6465
    for name in ("vlp16", "hdl32e"):
        want, counts = _assert_equal(packets, 1214, 1, [0.0, 0.001, 0.002], _model(name))
        assert counts.tolist() == [384] * 3 and np.isfinite(want).all()


@pytest.mark.parametrize("lasers", [16, 32])
def test_a_calibration_with_every_correction(lasers):
    _assert_equal(_random_packets(2, 5), 1214, 1, [0.0, 0.0013], _calibrated(lasers, 50 + lasers))


def test_zero_packets_touch_nothing():
    rec, counts = lidar_messages.velodyne_decode(np.zeros(0, dtype=np.uint8), 0, 1214, [], _model("vlp16"), returns=True)
    assert rec.shape == (0, 5) and counts.shape == (0,)


def test_a_second_call_uses_its_own_table():
    packets = _random_packets(2, 6)
    _, view = vo.place_packets(packets, 1214)
    first, second = _calibrated(16, 7), _model("vlp16")
    a = lidar_messages.velodyne_decode(view, 2, 1214, [0.0, 0.1], first)
    b = lidar_messages.velodyne_decode(view, 2, 1214, [0.0, 0.1], second)
    want_a, _ = vo.decode(view, 1214, [0.0, 0.1], first.table, first.distance_resolution, first.firing_period, first.laser_period)
    want_b, _ = vo.decode(view, 1214, [0.0, 0.1], second.table, second.distance_resolution, second.firing_period, second.laser_period)
    assert np.array_equal(a.view(np.uint32), want_a.view(np.uint32)) and np.array_equal(b.view(np.uint32), want_b.view(np.uint32))
    assert not np.array_equal(a.view(np.uint32)[:, :3], b.view(np.uint32)[:, :3])
    # ... and a 32-laser call after a 16-laser one, on the same bytes
    c = lidar_messages.velodyne_decode(view, 2, 1214, [0.0, 0.1], _model("hdl32e"))
    want_c, _ = vo.decode(view, 1214, [0.0, 0.1], *vo.model("hdl32e"))
    assert np.array_equal(c.view(np.uint32), want_c.view(np.uint32))


def test_records_are_where_the_packet_bytes_are():
    """Record (packet * 12 + block) * 32 + slot: one return alone in a packet lands at its own index, with the manual's geometry"""
    dist = np.zeros((12, 32), dtype=np.int64)
    dist[9, 17] = 5000  # second firing of block 9, laser 1 (+1 degree)
    packets = [vo.encode_packet([0] * 12, np.zeros((12, 32)), np.zeros((12, 32))), vo.encode_packet([9000] * 12, dist, np.full((12, 32), 200))]
    _, view = vo.place_packets(packets, 1214)
    rec, counts = lidar_messages.velodyne_decode(view, 2, 1214, [0.0, 0.25], _model("vlp16"), returns=True)
    assert counts.tolist() == [0, 1]
    hit = np.flatnonzero(np.isfinite(rec[:, 0]))
    assert hit.tolist() == [(1 * 12 + 9) * 32 + 17]
    xy, z = 10.0 * math.cos(math.radians(1.0)) + 0.0007 * math.sin(math.radians(1.0)), 10.0 * math.sin(math.radians(1.0)) - 0.0007 * math.cos(math.radians(1.0))
    assert np.abs(rec[hit[0], :3].astype(np.float64) - [0.0, -xy, z]).max() < 1e-5 and rec[hit[0], 3] == 200.0
    assert rec[hit[0], 4] == np.float32(0.25 + (19 * 55.296e-6 + 1 * 2.304e-6))


def test_the_phase_clock_is_read_refused_and_kept_over_a_refused_call():
    import ctypes

    from direct_visual_lidar_calibration_amd import _lib

    lib, model = _lib.load(), _model("vlp16")
    _, view = vo.place_packets(_random_packets(1, 5), 1206, 0)
    assert lidar_messages.velodyne_decode(view, 1, 1206, [0.0], model).shape == (384, 5)
    ms = (ctypes.c_double * 3)(-1.0, -1.0, -1.0)
    assert lib.nidreg_velodyne_get_timing(ms) == 0 and all(math.isfinite(v) and v >= 0.0 for v in ms)  # upload, kernel, copy back
    assert lib.nidreg_velodyne_get_timing(None) == _lib.NIDREG_ERR_INVALID and _lib.last_error() == "nidreg_velodyne_get_timing: null argument"
    with pytest.raises(ValueError, match="num_lasers 17"):
        lidar_messages.velodyne_decode(view, 1, 1206, [0.0], model._replace(table=np.zeros((17, 8))))
    after = (ctypes.c_double * 3)(-1.0, -1.0, -1.0)
    assert lib.nidreg_velodyne_get_timing(after) == 0 and list(after) == list(ms)  # a refused call leaves the last call's values
