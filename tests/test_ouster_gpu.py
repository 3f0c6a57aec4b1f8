"""GPU tests of nidreg_ouster_decode (csrc/nid_ouster_kernels.hpp) against the numpy restatement tests/ouster_oracle.py: the records must
be the oracle's BYTE FOR BYTE (compared as uint32, so the NaNs of the no-return records count), and the per-packet return counts the
oracle's.  The shapes are the smallest at which the kernel can go wrong: one packet of each profile with every pixel populated, the
largest staged column (H = 128, LEGACY), four columns a packet, three packets at strides that put every column at another alignment
from an odd address, invalid columns, measurement ids at and past W, range 0, range fields with every bit above the mask set, the
extremes of the other fields, a timestamp that clamps, a transform with every entry distinct, and a change of tables between calls."""
import numpy as np
import pytest

import ouster_fixture as ofx
import ouster_oracle as oo
from direct_visual_lidar_calibration_amd import lidar_messages

pytestmark = pytest.mark.gpu

W = 512
TRANSFORM = (0.36, 0.48, -0.8, 11.5, -0.8, 0.6, 0.01, -7.25, 0.48, 0.64, 0.6, 36.18)  # every entry distinct, none 0 or 1
RANGE_BITS = {ofx.LEGACY: (32, 20), ofx.RNG19: (32, 19), ofx.RNG15: (16, 15)}  # (bits of the field, bits of the range)


def _info(profile, H, C, transform=oo.IDENTITY12, n_mm=15.806, seed=0, w=W):
    rng = np.random.default_rng(100 + seed)
    altitude, azimuth = np.sort(rng.uniform(-22.5, 22.5, H))[::-1], rng.uniform(-4.5, 4.5, H)
    return lidar_messages.OusterInfo(profile, oo.PROFILES.index(profile), H, w, C, oo.packet_size(profile, H, C), oo.column_table(w), oo.beam_table(azimuth, altitude), n_mm,
                                     np.array(transform, dtype=np.float64), "sensor")


def _random_column(profile, H, rng, m, t, status=None, high_bits=False):
    field, kept = RANGE_BITS[profile]
    r = rng.integers(1, 1 << kept, H)
    if high_bits:
        r = r | (((1 << field) - 1) ^ ((1 << kept) - 1))  # every bit above the mask set
    refl = rng.integers(0, 1 << (16 if profile == ofx.LEGACY else 8), H)
    nir = rng.integers(0, 1 << (8 if profile == ofx.RNG15 else 16), H)
    return ofx.Column(t, m, ofx.VALID[profile] if status is None else status, r, refl, rng.integers(0, 1 << 16, H), nir, unused=int(rng.integers(0, 256)), encoder=int(rng.integers(0, 1 << 32)))


def _random_packets(profile, H, C, n, seed, t0=10**15):
    rng = np.random.default_rng(seed)
    return [ofx.encode_packet(profile, [_random_column(profile, H, rng, int(rng.integers(0, W)), t0 + (p * C + c) * 97657) for c in range(C)], 7, unused=0x5A) for p in range(n)]


def _assert_equal(packets, info, stride=None, lead=0, ts0=None):
    stride = info.packet_size if stride is None else stride
    assert all(len(p) == info.packet_size for p in packets)
    buf, view = ofx.place_packets(packets, stride, lead)
    if lead:
        assert view.ctypes.data % 2 == 1
    n = len(packets)
    ts0 = oo.first_valid_timestamp(view, stride, n, info.profile_name, info.H, info.C) if ts0 is None else ts0
    want, want_counts = oo.decode(view, stride, n, info.profile_name, info.H, info.W, info.C, info.column_table, info.beam_table, info.n_mm, info.transform12, ts0)
    got, counts = lidar_messages.ouster_decode(view, n, stride, info, ts0, returns=True)
    assert got.shape == (n * info.C * info.H, 8) and got.dtype == np.uint32
    diff = np.flatnonzero((got != oo.as_words(want)).any(axis=1))
    assert diff.size == 0, (diff[:5], got[diff[:5]], oo.as_words(want)[diff[:5]])
    assert np.array_equal(counts, want_counts)
    without = lidar_messages.ouster_decode(view, n, stride, info, ts0)  # returns_per_packet = NULL
    assert np.array_equal(without, oo.as_words(want))
    return want, want_counts


@pytest.mark.parametrize("profile", [ofx.LEGACY, ofx.RNG19, ofx.RNG15])
def test_one_packet_with_every_pixel_populated(profile):
    want, counts = _assert_equal(_random_packets(profile, 16, 16, 1, 1), _info(profile, 16, 16))
    assert counts.tolist() == [256] and np.isfinite(want["x"]).all() and want["ring"].reshape(16, 16).tolist() == [list(range(16))] * 16
    if profile == ofx.RNG15:
        assert not want["intensity"].any() and (want["range"] % 8 == 0).all() and (want["ambient"] % 16 == 0).all()


def test_the_largest_staged_column():
    want, counts = _assert_equal(_random_packets(ofx.LEGACY, 128, 16, 2, 2), _info(ofx.LEGACY, 128, 16, TRANSFORM), stride=oo.packet_size(ofx.LEGACY, 128, 16) + 3, lead=1)
    assert counts.tolist() == [2048, 2048]


@pytest.mark.parametrize("profile,H", [(ofx.LEGACY, 32), (ofx.RNG19, 64), (ofx.RNG15, 128)])
def test_four_columns_a_packet(profile, H):
    _, counts = _assert_equal(_random_packets(profile, H, 4, 3, 3), _info(profile, H, 4, TRANSFORM))
    assert counts.tolist() == [4 * H] * 3


@pytest.mark.parametrize("extra", [1, 3])
@pytest.mark.parametrize("profile", [ofx.LEGACY, ofx.RNG19, ofx.RNG15])
def test_three_packets_at_odd_strides_from_an_odd_address(profile, extra):
    info = _info(profile, 16, 16, TRANSFORM)
    want, _ = _assert_equal(_random_packets(profile, 16, 16, 3, 4 + extra), info, stride=info.packet_size + extra, lead=1)
    assert len(np.unique(want["t"])) == 48


def test_invalid_columns():
    rng = np.random.default_rng(5)
    cols = [_random_column(ofx.LEGACY, 16, rng, m, 1000 + m, status=s) for m, s in enumerate([0, 0xFFFFFFFE, 0xFFFFFFFF, 0x7FFFFFFF, 0xFFFFFFFF, 1])]
    want, counts = _assert_equal([ofx.encode_packet(ofx.LEGACY, cols, 1)], _info(ofx.LEGACY, 16, 6))
    assert counts.tolist() == [32] and np.isfinite(want["x"].reshape(6, 16)).all(axis=1).tolist() == [False, False, True, False, True, False]
    dead = want.reshape(6, 16)[1]
    assert not dead["range"].any() and not dead["reflectivity"].any() and not dead["ambient"].any() and not dead["intensity"].any() and dead["ring"].tolist() == list(range(16))
    assert (want.reshape(6, 16)["t"][:, 0]).tolist() == [2**32 - 1, 2**32 - 1, 0, 1, 2, 3]  # ts0 is column 2's: the earlier columns wrap and clamp
    for profile in (ofx.RNG19, ofx.RNG15):  # bit 0 decides, whatever the other bits
        cols = [_random_column(profile, 16, rng, m, 1000 + m, status=s) for m, s in enumerate([0xFFFE, 0, 1, 0xFFFF, 0x8000, 3])]
        want, counts = _assert_equal([ofx.encode_packet(profile, cols, 1)], _info(profile, 16, 6))
        assert counts.tolist() == [48] and np.isfinite(want["x"].reshape(6, 16)).all(axis=1).tolist() == [False, False, True, True, False, True]


@pytest.mark.parametrize("profile", [ofx.LEGACY, ofx.RNG19, ofx.RNG15])
def test_measurement_ids_at_and_past_the_table(profile):
    rng = np.random.default_rng(6)
    for w in (W, 16, 4096):
        cols = [_random_column(profile, 16, rng, m, 1000 + k) for k, m in enumerate([w - 1, w, 65535, 0, w + 1])]
        want, counts = _assert_equal([ofx.encode_packet(profile, cols, 1)], _info(profile, 16, 5, w=w))
        assert counts.tolist() == [32] and np.isfinite(want["x"].reshape(5, 16)).all(axis=1).tolist() == [True, False, False, True, False]


@pytest.mark.parametrize("profile", [ofx.LEGACY, ofx.RNG19, ofx.RNG15])
def test_range_zero_the_bits_above_the_mask_and_the_field_extremes(profile):
    rng = np.random.default_rng(7)
    field, kept = RANGE_BITS[profile]
    above = ((1 << field) - 1) ^ ((1 << kept) - 1)
    plain = _random_column(profile, 16, rng, 3, 1000)
    plain.range[:4] = [0, above, 1, (1 << kept) - 1]  # range 0; range 0 under the bits above the mask; the smallest and the largest range
    high = _random_column(profile, 16, rng, 4, 1001, high_bits=True)
    top16, top8 = 65535, 255
    high.reflectivity[:2], high.signal[:2], high.near_ir[:2] = [0, top16 if profile == ofx.LEGACY else top8], [0, top16], [0, top8 if profile == ofx.RNG15 else top16]
    want, counts = _assert_equal([ofx.encode_packet(profile, [plain, high], 1)], _info(profile, 16, 2, TRANSFORM))
    assert counts.tolist() == [30] and np.isnan(want["x"][:2]).all() and np.isfinite(want["x"][2:]).all()
    shift = 3 if profile == ofx.RNG15 else 0
    assert want["range"][:4].tolist() == [0, 0, 1 << shift, ((1 << kept) - 1) << shift] and (want["range"][16:] < (1 << kept) << shift).all()
    assert want["reflectivity"][17] == (top16 if profile == ofx.LEGACY else top8) and want["ambient"][17] == (top8 << 4 if profile == ofx.RNG15 else top16)
    assert want["intensity"][17] == (0.0 if profile == ofx.RNG15 else 65535.0) and want["reflectivity"][16] == 0 and want["ambient"][16] == 0


def test_a_timestamp_four_seconds_behind_ts0_clamps():
    rng = np.random.default_rng(8)
    t0 = 2**63 + 12345  # the upper half of the 64 bits
    cols = [_random_column(ofx.RNG19, 16, rng, k, t0 + dt) for k, dt in enumerate([0, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 1, 2**40])]
    want, _ = _assert_equal([ofx.encode_packet(ofx.RNG19, cols, 1)], _info(ofx.RNG19, 16, 6))
    assert want["t"].reshape(6, 16)[:, 5].tolist() == [0, 2**32 - 2, 2**32 - 1, 2**32 - 1, 2**32 - 1, 2**32 - 1]


def test_zero_packets_touch_nothing():
    rec, counts = lidar_messages.ouster_decode(np.zeros(0, dtype=np.uint8), 0, 4096, _info(ofx.RNG19, 16, 16), 0, device=10**6, returns=True)  # no such device: none is touched
    assert rec.shape == (0, 8) and counts.shape == (0,)


def test_a_second_call_uses_its_own_tables():
    packets = _random_packets(ofx.RNG19, 16, 16, 2, 9)
    first, second = _info(ofx.RNG19, 16, 16, TRANSFORM, seed=1), _info(ofx.RNG19, 16, 16, n_mm=27.67, seed=2)
    a, _ = _assert_equal(packets, first)
    b, _ = _assert_equal(packets, second)
    assert not np.array_equal(a["x"], b["x"]) and np.array_equal(a["range"], b["range"])
    c, _ = _assert_equal(packets, first)  # ... and the first again, behind the second
    assert np.array_equal(oo.as_words(a), oo.as_words(c))
    # another W: the same measurement ids are other angles, or past the table
    _assert_equal(packets, _info(ofx.RNG19, 16, 16, w=256, seed=1))


def test_record_k_lies_at_byte_32_k():
    """Record (packet * C + column) * H + pixel: one return alone in two packets lands at its own index, with the fields at their offsets"""
    def empty(m):
        return ofx.Column(5000 + m, m, 1, [0] * 16, [9] * 16, [9] * 16, [9] * 16)

    cols = [[empty(0), empty(1), empty(2)], [empty(3), empty(W // 4), empty(5)]]
    cols[1][1].range[11], cols[1][1].reflectivity[11], cols[1][1].signal[11], cols[1][1].near_ir[11] = 6000, 200, 3000, 400
    info = lidar_messages.OusterInfo(ofx.RNG19, 1, 16, W, 3, oo.packet_size(ofx.RNG19, 16, 3), oo.column_table(W), oo.beam_table([0.0] * 16, [0.0] * 16), 0.0, np.array(oo.IDENTITY12), "lidar")
    packets = [ofx.encode_packet(ofx.RNG19, c, 1) for c in cols]
    _, view = ofx.place_packets(packets, info.packet_size)
    rec, counts = lidar_messages.ouster_decode(view, 2, info.packet_size, info, 5000, returns=True)
    assert counts.tolist() == [0, 1]
    k = (1 * 3 + 1) * 16 + 11
    raw = rec.reshape(-1).view(np.uint8)
    hit = np.flatnonzero(np.isfinite(rec[:, 0].view(np.float32)))
    assert hit.tolist() == [k]
    one = raw[32 * k : 32 * k + 32].view(oo.RECORD)[0]
    assert abs(one["x"]) < 1e-14 and one["y"] == np.float32(-6.0) and one["z"] == 0.0 and one["intensity"] == 3000.0 and one["t"] == W // 4
    assert (one["reflectivity"], one["ring"], one["ambient"], one["range"]) == (200, 11, 400, 6000) and not raw[32 * k + 26 : 32 * k + 28].any()


def test_every_refusal_of_the_entry_point_leaves_the_records_alone():
    import ctypes

    from direct_visual_lidar_calibration_amd import _lib

    lib = _lib.load()
    info = _info(ofx.RNG19, 16, 16)
    size = info.packet_size
    packets = np.frombuffer(_random_packets(ofx.RNG19, 16, 16, 1, 10)[0], dtype=np.uint8).copy()
    records = np.full((256, 8), 0xDEADBEEF, dtype=np.uint32)
    counts = np.full(1, -5, dtype=np.int32)
    good = dict(device=10**6, packets=packets.ctypes.data, n=1, stride=size, profile=1, H=16, W=W, C=16, columns=info.column_table.copy(), beams=info.beam_table.copy(), n_mm=15.806,
                transform=info.transform12.copy(), ts0=0, out=records.ctypes.data)

    def call(**changes):
        a = dict(good)
        a.update(changes)
        dp = lambda v: None if v is None else v.ctypes.data_as(_lib.c_double_p)  # noqa: E731
        rc = lib.nidreg_ouster_decode(a["device"], a["packets"], a["n"], a["stride"], a["profile"], a["H"], a["W"], a["C"], dp(a["columns"]), dp(a["beams"]), a["n_mm"], dp(a["transform"]),
                                      a["ts0"], a["out"], counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        return rc, _lib.last_error()

    def bad(table, index):
        t = table.copy()
        t.reshape(-1)[index] = np.nan if index % 2 else np.inf
        return t

    cases = [(dict(profile=3), "profile 3"), (dict(profile=-1), "profile -1"), (dict(H=48), "H 48"), (dict(H=256), "H 256"), (dict(W=15), "W 15"), (dict(W=4097), "W 4097"),
             (dict(C=0), "C 0"), (dict(C=17), "C 17"), (dict(n=-1), "num_packets -1"), (dict(n=4097), "num_packets 4097"), (dict(stride=size - 1), f"below the {size} bytes"),
             (dict(stride=32769), "above 32768"), (dict(packets=None), "null"), (dict(columns=None), "null"), (dict(beams=None), "null"), (dict(transform=None), "null"),
             (dict(out=None), "null"), (dict(columns=bad(info.column_table, 2 * W - 1)), f"column {W - 1} is not finite"), (dict(beams=bad(info.beam_table, 4 * 15 + 2)), "beam 15 is not finite"),
             (dict(transform=bad(info.transform12, 11)), "transform12 entry 11"), (dict(n_mm=float("nan")), "n_mm"), (dict(n_mm=float("-inf")), "n_mm")]
    for changes, text in cases:
        rc, message = call(**changes)  # device 10^6 does not exist: a refusal that came after the device was touched would read otherwise
        assert rc == _lib.NIDREG_ERR_INVALID and text in message and "nidreg_ouster_decode" in message, (changes, message)
        assert (records == 0xDEADBEEF).all() and counts[0] == -5
    assert call(n=0, packets=None, out=None)[0] == 0 and (records == 0xDEADBEEF).all() and counts[0] == -5  # zero packets: success, nothing touched
    with pytest.raises(ValueError, match="H 48"):  # the Python wrapper passes the refusal on
        lidar_messages.ouster_decode(packets, 1, size, info._replace(H=48), 0)
    assert lib.nidreg_ouster_get_timing(None) == _lib.NIDREG_ERR_INVALID
