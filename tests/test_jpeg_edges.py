"""The JPEG kernels (csrc/nid_jpeg_kernels.hpp) past the golden streams.  Every stream here is written in the test, seeded, by
tests/jpeg_fixture.py, and every device result is compared with the numpy restatement (tests/jpeg_oracle.py) for equality:

  a. the wrapping IDCT: 16-bit tables and coefficients whose products leave int16 and int32, where the decoder's result is its own;
  b. a scalar restatement of one block's decode in Python integers, every C operation reduced to int32 by hand, which vouches for
     the numpy oracle in that domain (CPU only);
  c. a colour lattice: every (Y, Cb, Cr) in {0, 1, 127, 128, 129, 254, 255}^3, each side of each clamp of the colour kernel;
  d. every size 1..18 x 1..18 in the four layouts, mid sizes, and chroma that drives every rounding residue of the upsampling;
  e. the largest accepted dimension, as one row and as one column;
  f. DC predictions that leave int16, and categories 15.

The CPU tests beside the GPU ones assert, on the oracle and on the inputs alone, that each case reaches what it is there for."""
import ctypes
import functools
import io
import itertools

import numpy as np
import pytest

import jpeg_fixture as jf
import jpeg_oracle as jo
from direct_visual_lidar_calibration_amd import _lib, dataset
from make_jpeg_golden import FLAT

MODES = ((dataset.JPEG_GRAY_LUMA, jo.LUMA), (dataset.JPEG_GRAY_BGR, jo.BGR))
LAYOUTS = {"gray": jf.GRAY, "444": jf.YCC444, "422": jf.YCC422, "420": jf.YCC420}


def device_decode(data, mode):
    """The device's decode, made twice: the same bytes both times"""
    first = dataset.decode_jpeg_gray(data, mode)
    again = dataset.decode_jpeg_gray(data, mode)
    assert first.tobytes() == again.tobytes(), "two decodes of one stream differ"
    return first


def assert_device_equals_oracle(data, label):
    for dev_mode, ora_mode in MODES:
        want = jo.decode_gray(data, ora_mode)
        got = device_decode(data, dev_mode)
        assert got.shape == want.shape, (label, dev_mode, got.shape, want.shape)
        if not np.array_equal(got, want):
            y, x = np.argwhere(got != want)[0]
            raise AssertionError(f"{label}, mode {dev_mode}: {int((got != want).sum())} pixels differ, the first at x={x} y={y}: device {got[y, x]}, oracle {want[y, x]}")


def pillow_planes(data):
    """(Pillow's Y plane, Pillow's RGB through the cv luma): libjpeg-turbo, a reference inside the int16 domain only"""
    from PIL import Image

    im = Image.open(io.BytesIO(data))
    im.draft("L", im.size)
    assert im.mode == "L"
    return np.asarray(im).copy(), jo.cv_luma(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))


def assert_oracle_equals_pillow(data, label):
    y, g = pillow_planes(data)
    assert np.array_equal(jo.decode_gray(data, jo.LUMA), y), label
    assert np.array_equal(jo.decode_gray(data, jo.BGR), g), label


def in_int16_domain(data):
    report = {}
    jo.decode_planes(data, report)
    return report["deq"] <= 32767 and report["pass1"] <= 32767


# ------------------------------------------------------------------------------------------------ a. the wrapping IDCT
# name -> (largest |coefficient|, coefficients a block (None: all 64), largest table entry)
WRAP_RANGES = {"c32767_q65535": (32767, None, 65535), "c2047_q65535": (2047, None, 65535), "c1023_q4096": (1023, None, 4096), "sparse3000_q4096": (3000, 2, 4096)}
PAST_INT32 = ("c32767_q65535", "c2047_q65535")
WRAP_SIZES = ((256, 64), (260, 72))  # 256 blocks: 32 full groups of the IDCT kernel; 33 x 9 = 297 blocks: a tail group of one, and a cropped last column
WRAP_CASES = [(name, w, h) for name in WRAP_RANGES for w, h in WRAP_SIZES]


def wrap_table(rng, name):
    return rng.integers(1, WRAP_RANGES[name][2] + 1, 64)


def wrap_blocks(rng, name, shape):
    """Quantised blocks of one range.  Never -32768, and no two successive DC values further apart than 32767: a DC difference of
    category 16 is refused."""
    amp, per_block, _ = WRAP_RANGES[name]
    bh, bw = shape
    b = rng.integers(-amp, amp + 1, (bh, bw, 64))
    if per_block is not None:  # sparse: one or two coefficients a block, anywhere in it
        keep = np.zeros((bh, bw, 64), dtype=bool)
        for by, bx in itertools.product(range(bh), range(bw)):
            keep[by, bx, rng.choice(64, size=int(rng.integers(1, per_block + 1)), replace=False)] = True
        b *= keep
    if 2 * amp > 32767:  # a walk over the whole range whose steps fit category 15
        prev = 0
        for by, bx in itertools.product(range(bh), range(bw)):
            prev = b[by, bx, 0] = int(rng.integers(max(-amp, prev - 32767), min(amp, prev + 32767) + 1))
    return b.astype(np.int16)


@functools.lru_cache(maxsize=None)
def wrap_stream(name, w, h):
    """(the stream, its blocks, its table): gray, SOF1, 16-bit table entries"""
    rng = np.random.default_rng([11, sorted(WRAP_RANGES).index(name), w, h])
    q = wrap_table(rng, name)
    blocks = [wrap_blocks(rng, name, jf.grid(w, h, jf.GRAY, 0))]
    return jf.write_jpeg(w, h, jf.GRAY, blocks, {0: q}, sof=0xC1, dqt16=True, segments=[jf.jfif()]), blocks, q


@functools.lru_cache(maxsize=None)
def wrap_stream_444():
    """4:4:4 with every component in the wrapping domain: the colour kernel is fed planes from wrapped blocks"""
    rng = np.random.default_rng(12)
    w, h = 64, 40
    tables = {0: wrap_table(rng, "c2047_q65535"), 1: wrap_table(rng, "c2047_q65535")}
    blocks = [wrap_blocks(rng, "c2047_q65535", jf.grid(w, h, jf.YCC444, ci)) for ci in range(3)]
    return jf.write_jpeg(w, h, jf.YCC444, blocks, tables, sof=0xC1, dqt16=True, segments=[jf.jfif()]), blocks, tables


def largest_product(blocks, q):
    return int(np.abs(blocks.astype(np.int64) * np.asarray(q, dtype=np.int64)).max())


def share_past_int32(blocks, q):
    """The share of the column pass's outputs (before the descale) that leave int32 when the pass is computed exactly, in int64 (no
    term of it comes near 2^63: |coefficient x entry| < 2^31, the multipliers are below 2^15 and a sum has at most 8 terms)"""
    deq = (blocks.astype(np.int64) * np.asarray(q, dtype=np.int64)).reshape(-1, 8, 8)
    exact = jo._idct_pass(deq.transpose(0, 2, 1))
    assert exact.dtype == np.int64
    return float((np.abs(exact) >= 2**31).mean())


def assert_blocks_wrap(blocks, q, name):
    """No single product can pass 2^31 (32767 x 65535 = 2^31 - 98303), so that is not what is asked of the two widest ranges: asked
    is that the arithmetic really wraps.  Every range leaves int16 with its products and int32 somewhere in the column pass; in the
    two widest a typical product is 2^30 or 2^26 and a multiplier 2^13, so most of the pass's outputs must have wrapped."""
    assert largest_product(blocks, q) > 32767, name
    share = share_past_int32(blocks, q)
    assert share > (0.5 if name in PAST_INT32 else 0.0), (name, share)


def assert_plane_tests_more_than_the_sign(plane, label):
    """Before the clamp the output is close to uniform over +-8192 in this domain: half the pixels are 0, half 255, and only the few
    in between tell a right low-order bit from a wrong one"""
    zeros, full, between = (plane == 0).mean(), (plane == 255).mean(), ((plane >= 1) & (plane <= 254)).mean()
    assert zeros >= 0.25 and full >= 0.25 and between >= 0.01, (label, zeros, full, between)


@pytest.mark.parametrize("name,w,h", WRAP_CASES)
def test_wrapping_streams_leave_int16_and_int32_and_test_more_than_the_sign(name, w, h):
    data, blocks, q = wrap_stream(name, w, h)
    assert b"\xff\xc1" in data and data[data.index(b"\xff\xdb") + 4] >> 4 == 1  # SOF1, 16-bit entries
    assert blocks[0].min() >= -32767 and np.abs(np.diff(blocks[0][:, :, 0].reshape(-1).astype(np.int64), prepend=0)).max() <= 32767
    assert_blocks_wrap(blocks[0], q, name)
    s, planes = jo.decode_planes(data)
    assert np.array_equal(jo.coefficients(data)[1][0], blocks[0]) and np.array_equal(s.qt[0], q)  # the stream holds what was asked for
    assert (len(blocks[0].reshape(-1, 64)) % 8 != 0) == ((w, h) == WRAP_SIZES[1])  # the tail group
    assert planes[0].shape == (h, w)
    assert_plane_tests_more_than_the_sign(planes[0], (name, w, h))


def test_wrapping_444_stream_wraps_in_every_component():
    data, blocks, tables = wrap_stream_444()
    for ci in range(3):
        assert_blocks_wrap(blocks[ci], tables[min(ci, 1)], "c2047_q65535")
    _s, planes = jo.decode_planes(data)
    for ci in range(3):
        assert_plane_tests_more_than_the_sign(planes[ci], ci)
    assert not np.array_equal(jo.decode_gray(data, jo.LUMA), jo.decode_gray(data, jo.BGR))


@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h", WRAP_CASES)
def test_wrapping_idct_equals_the_oracle(name, w, h):
    assert_device_equals_oracle(wrap_stream(name, w, h)[0], (name, w, h))


@pytest.mark.gpu
def test_wrapping_444_equals_the_oracle():
    assert_device_equals_oracle(wrap_stream_444()[0], "wrapping 4:4:4")


# ------------------------------------------------------------------------------------------------ b. the scalar reference
def i32(v):
    """A C int32 result: the low 32 bits, two's complement"""
    return ((v + 2**31) % 2**32) - 2**31


def scalar_pass(x):
    """One 8-point pass of jpeg_idct_islow before the descale (jidctint.c: CONST_BITS 13; FIX(0.298631336) = 2446, FIX(0.390180644) =
    3196, FIX(0.541196100) = 4433, FIX(0.765366865) = 6270, FIX(0.899976223) = 7373, FIX(1.175875602) = 9633, FIX(1.501321110) =
    12299, FIX(1.847759065) = 15137, FIX(1.961570560) = 16069, FIX(2.053119869) = 16819, FIX(2.562915447) = 20995,
    FIX(3.072711026) = 25172), in Python integers: every sum, difference, product and shift is reduced to int32 where it is made"""
    add, sub, mul = (lambda a, b: i32(a + b)), (lambda a, b: i32(a - b)), (lambda a, b: i32(a * b))
    # even part
    z2, z3 = x[2], x[6]
    z1 = mul(add(z2, z3), 4433)
    tmp2 = add(z1, mul(z3, -15137))
    tmp3 = add(z1, mul(z2, 6270))
    z2, z3 = x[0], x[4]
    tmp0 = i32(add(z2, z3) << 13)
    tmp1 = i32(sub(z2, z3) << 13)
    tmp10, tmp13, tmp11, tmp12 = add(tmp0, tmp3), sub(tmp0, tmp3), add(tmp1, tmp2), sub(tmp1, tmp2)
    # odd part
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = add(tmp0, tmp3), add(tmp1, tmp2), add(tmp0, tmp2), add(tmp1, tmp3)
    z5 = mul(add(z3, z4), 9633)
    tmp0, tmp1, tmp2, tmp3 = mul(tmp0, 2446), mul(tmp1, 16819), mul(tmp2, 25172), mul(tmp3, 12299)
    z1, z2, z3, z4 = mul(z1, -7373), mul(z2, -20995), mul(z3, -16069), mul(z4, -3196)
    z3, z4 = add(z3, z5), add(z4, z5)
    tmp0 = add(tmp0, add(z1, z3))
    tmp1 = add(tmp1, add(z2, z4))
    tmp2 = add(tmp2, add(z2, z3))
    tmp3 = add(tmp3, add(z1, z4))
    return [add(tmp10, tmp3), add(tmp11, tmp2), add(tmp12, tmp1), add(tmp13, tmp0), sub(tmp13, tmp0), sub(tmp12, tmp1), sub(tmp11, tmp2), sub(tmp10, tmp3)]


def scalar_descale(v, n):
    return i32(v + (1 << (n - 1))) >> n  # (Python's >> of a negative integer is the arithmetic shift)


def scalar_block(coef, q):
    """One block: 64 quantised coefficients and 64 table entries, natural order -> (8 x 8 pixels, 8 x 8 values before the clamp).
    Dequantise, the column pass descaled by CONST_BITS - PASS1_BITS = 11, the row pass descaled by CONST_BITS + PASS1_BITS + 3 = 18,
    + 128, saturate to [0, 255]."""
    deq = [i32(int(c) * int(t)) for c, t in zip(coef, q)]
    ws = [[0] * 8 for _ in range(8)]
    for c in range(8):
        for r, v in enumerate(scalar_pass([deq[8 * r + c] for r in range(8)])):
            ws[r][c] = scalar_descale(v, 11)
    raw = [[i32(scalar_descale(v, 18) + 128) for v in scalar_pass(ws[r])] for r in range(8)]
    return [[min(max(v, 0), 255) for v in row] for row in raw], raw


def numpy_raw(blocks, q):
    """What jpeg_oracle.idct_blocks holds before its clamp, from the oracle's own two functions: (n, 8, 8) int32"""
    with np.errstate(over="ignore"):
        deq = (blocks.astype(np.int32) * q.astype(np.int32)).reshape(-1, 8, 8)
        cols = jo._descale(jo._idct_pass(deq.transpose(0, 2, 1)), 11).transpose(0, 2, 1)
        return jo._descale(jo._idct_pass(cols), 18) + 128


SCALAR_BLOCKS = 256


def scalar_inputs(name):
    rng = np.random.default_rng([13, sorted(list(WRAP_RANGES) + ["int16_domain"]).index(name)])
    if name == "int16_domain":  # what the golden streams hold: sparse small coefficients, small tables
        return jf.random_blocks(rng, 8 * SCALAR_BLOCKS, 8, jf.GRAY, amplitude=60, density=0.3)[0], rng.integers(1, 17, 64)
    return wrap_blocks(rng, name, (1, SCALAR_BLOCKS)), wrap_table(rng, name)


@pytest.mark.parametrize("name", list(WRAP_RANGES) + ["int16_domain"])
def test_numpy_oracle_equals_the_scalar_restatement(name):
    blocks, q = scalar_inputs(name)
    if name == "int16_domain":
        report = {}
        jo.idct_blocks(blocks, q.astype(np.uint16), report)
        assert report["deq"] <= 32767 and report["pass1"] <= 32767
    else:
        assert_blocks_wrap(blocks, q, name)
    plane = jo.idct_blocks(blocks, q.astype(np.uint16))
    raw = numpy_raw(blocks, q.astype(np.uint16))
    assert plane.shape == (8, 8 * SCALAR_BLOCKS)
    between = 0
    for k in range(SCALAR_BLOCKS):
        pixels, before = scalar_block(blocks[0, k], q)
        assert pixels == plane[:, 8 * k : 8 * k + 8].tolist(), (name, k)
        assert before == raw[k].tolist(), (name, k)
        between += sum(1 <= v <= 254 for row in pixels for v in row)
    assert between >= 64  # the clamp hides none of the comparison above (the values before it are compared too)


def test_scalar_restatement_on_blocks_worked_by_hand():
    """A DC of 8 with a table entry of 4: 32 << 13 descaled by 11 is 128 in every row, 128 << 13 descaled by 18 is 4, + 128.
    And int32 wrapping where it first shows: 32767 x 65535 = 2147385345 fits, twice that does not."""
    assert scalar_block([8] + [0] * 63, [4] * 64)[0] == [[132] * 8] * 8
    assert i32(32767 * 65535) == 2147385345 and i32(2 * 32767 * 65535) == 2 * 2147385345 - 2**32 and i32(-(2**31) - 1) == 2**31 - 1
    assert scalar_descale(-1, 11) == 0 and scalar_descale(-1025, 11) == -1 and scalar_descale(2**31 - 1, 11) == -(2**20)  # the rounding add wraps


# ------------------------------------------------------------------------------------------------ c. the colour lattice
LATTICE = (0, 1, 127, 128, 129, 254, 255)


@functools.lru_cache(maxsize=None)
def lattice_stream():
    """(the stream, the (7, 49, 3) block constants): 392 x 56, 4:4:4, DC-only blocks, both tables flat at 8: a DC of d gives
    8 d << 13 descaled by 11 = 32 d, then 32 d << 13 descaled by 18 = d exactly, so each block is the constant d + 128"""
    values = np.array(list(itertools.product(LATTICE, repeat=3)), dtype=np.int64).reshape(7, 49, 3)
    blocks = []
    for ci in range(3):
        b = np.zeros((7, 49, 64), dtype=np.int16)
        b[:, :, 0] = values[:, :, ci] - 128
        blocks.append(b)
    return jf.write_jpeg(392, 56, jf.YCC444, blocks, {0: np.full(64, 8), 1: np.full(64, 8)}, segments=[jf.jfif()]), values


def test_lattice_planes_hold_the_constants_and_reach_each_side_of_each_clamp():
    data, values = lattice_stream()
    assert {tuple(v) for v in values.reshape(-1, 3)} == set(itertools.product(LATTICE, repeat=3)) and values.shape[:2] == (7, 49)
    assert in_int16_domain(data)
    _s, planes = jo.decode_planes(data)
    for ci in range(3):
        assert np.array_equal(planes[ci], np.kron(values[:, :, ci], np.ones((8, 8), dtype=np.int64)))
    # the three channels before their clamps, as the colour kernel's comment states them (libjpeg's jdcolor.c tables)
    y, cb, cr = values[:, :, 0], values[:, :, 1] - 128, values[:, :, 2] - 128
    channels = {"R": y + ((91881 * cr + 32768) >> 16), "G": y + ((-22554 * cb + 32768 - 46802 * cr) >> 16), "B": y + ((116130 * cb + 32768) >> 16)}
    for name, v in channels.items():
        assert (v < 0).any() and (v > 255).any() and ((v > 0) & (v < 255)).any(), name
    rgb = np.clip(np.stack([channels["R"], channels["G"], channels["B"]], axis=-1), 0, 255)
    assert np.array_equal(jo.decode_rgb(data)[::8, ::8], rgb)
    assert not np.array_equal(jo.decode_gray(data, jo.LUMA), jo.decode_gray(data, jo.BGR))


def test_lattice_oracle_equals_pillow():
    pytest.importorskip("PIL")
    assert_oracle_equals_pillow(lattice_stream()[0], "lattice")


@pytest.mark.gpu
def test_colour_lattice_equals_the_oracle():
    assert_device_equals_oracle(lattice_stream()[0], "lattice")


# ------------------------------------------------------------------------------------------------ d. the size sweep
SWEEP = [(w, h) for w in range(1, 19) for h in range(1, 19)]
# mid sizes: a colour grid of several 256-thread blocks, planes of many IDCT groups, and the block counts modulo 8 that 1..18 leave out
MID = {
    "gray": [(250, 37), (37, 250), (260, 37), (50, 3), (130, 19)],
    "444": [(250, 37), (37, 250), (260, 37), (50, 3), (130, 19)],
    "422": [(250, 37), (37, 250), (70, 5), (100, 3), (130, 19)],
    "420": [(250, 37), (37, 250), (40, 10), (70, 10), (90, 10), (100, 10), (130, 19)],
}


def sweep_sizes(layout):
    return SWEEP + MID[layout]


@functools.lru_cache(maxsize=None)
def sweep_streams(layout):
    """``{(w, h): stream}``: jpeg_fixture's sparse random blocks with the flat tables 3 / 5 of the golden generator"""
    comps = LAYOUTS[layout]
    rng = np.random.default_rng([14, sorted(LAYOUTS).index(layout)])
    return {(w, h): jf.write_jpeg(w, h, comps, jf.random_blocks(rng, w, h, comps), FLAT, segments=[jf.jfif()]) for w, h in sweep_sizes(layout)}


@functools.lru_cache(maxsize=None)
def dense_chroma_stream(layout):
    """Dense, large-amplitude chroma inside the int16 domain: the downsampled planes take values all over [0, 255], so the sums the
    upsampling rounds take every residue.  45 x 27: odd sizes, dw = 23, dh = 14 (4:2:0) or 27 (4:2:2)."""
    comps = LAYOUTS[layout]
    rng = np.random.default_rng([15, sorted(LAYOUTS).index(layout)])
    w, h = 45, 27
    blocks = jf.random_blocks(rng, w, h, comps)
    for ci in (1, 2):
        bh, bw = jf.grid(w, h, comps, ci)
        blocks[ci] = (rng.integers(-30, 31, (bh, bw, 64)) * (rng.random((bh, bw, 64)) < 0.5)).astype(np.int16)
        blocks[ci][:, :, 0] = rng.integers(-40, 41, (bh, bw))
    return jf.write_jpeg(w, h, comps, blocks, FLAT, segments=[jf.jfif()])


def test_sweep_visits_the_geometry_it_is_there_for():
    assert len(SWEEP) == 324 and 4 * len(SWEEP) == 1296
    for layout, comps in LAYOUTS.items():
        sizes = sweep_sizes(layout)
        assert len(set(sizes)) == len(sizes) and sorted(sweep_streams(layout)) == sorted(sizes)
        # the tail group of the IDCT kernel: every block count modulo 8 that the layout can have (a component of h x v blocks an MCU
        # has a multiple of h v blocks: 4:2:2 luma only even counts, 4:2:0 luma only multiples of 4)
        for ci in range(len(comps)):
            per_mcu = 1 if len(comps) == 1 else comps[ci][1] * comps[ci][2]
            seen = {int(np.prod(jf.grid(w, h, comps, ci))) % 8 for w, h in sizes}
            assert seen == {per_mcu * k % 8 for k in range(8)}, (layout, ci, seen)
        # the colour kernel's grid: one block, and several
        if len(comps) == 3:
            groups = [-(-w // 8) * 2 * h for w, h in sizes]
            assert min(groups) <= 256 and max(groups) > 4 * 256
        # Y and chroma planes that end in different tail groups
        if layout in ("422", "420"):
            assert any(int(np.prod(jf.grid(w, h, comps, 0))) % 8 != int(np.prod(jf.grid(w, h, comps, 1))) % 8 for w, h in MID[layout])
    assert {int(np.prod(jf.grid(w, h, jf.GRAY, 0))) % 8 for w, h in sweep_sizes("gray")} == set(range(8))  # luma: all eight
    for layout, vs in (("422", 1), ("420", 2)):
        assert {int(np.prod(jf.grid(w, h, LAYOUTS[layout], 1))) % 8 for w, h in sweep_sizes(layout)} == set(range(8))  # chroma: all eight
        geometry = {(w, h): (-(-w // 2), -(-h // vs)) for w, h in SWEEP}  # (dw, dh)
        for (w, h), (dw, dh) in geometry.items():  # as the oracle's parser has them
            c = jo.parse(sweep_streams(layout)[(w, h)]).comps[1]
            assert (c["dw"], c["dh"]) == (dw, dh)
        assert {dw for dw, _ in geometry.values()} >= {1, 2, 3}  # replication (dw <= 2) and the first fancy width
        assert {dh % 2 for _, dh in geometry.values()} == {0, 1}
        # an odd image width with the triangle filter: the last column's right neighbour is the min(i + 1, dw - 1) clamp
        assert any(w % 2 == 1 and dw > 2 for (w, _h), (dw, _dh) in geometry.items())
        assert any(w % 2 == 0 and dw > 2 for (w, _h), (dw, _dh) in geometry.items())
    # 4:2:0: a last image row y that is odd and whose chroma row r = y >> 1 is the last one: far is the min(r + 1, dh - 1) clamp
    assert any((h - 1) % 2 == 1 and (h - 1) >> 1 == -(-h // 2) - 1 and -(-w // 2) > 2 for w, h in SWEEP)
    assert any((h - 1) % 2 == 0 and -(-w // 2) > 2 for w, h in SWEEP)  # and one that is even: far is the row above


def test_dense_chroma_takes_every_rounding_residue():
    for layout in ("422", "420"):
        data = dense_chroma_stream(layout)
        assert in_int16_domain(data)
        s, planes = jo.decode_planes(data)
        assert s.comps[1]["dw"] == 23 and s.comps[1]["dh"] == (27 if layout == "422" else 14)
        for plane in planes[1:]:
            a = plane.astype(np.int64)
            assert a.shape == (s.comps[1]["dh"], 23)
            if layout == "422":  # 3 near + neighbour: the left one for an even output column, the right one for an odd one
                left, right = jo._edge(a, 1)[:, :-2], jo._edge(a, 1)[:, 2:]
                for parity, sums in (("even", 3 * a + left), ("odd", 3 * a + right)):
                    assert set((sums % 4).reshape(-1).tolist()) == {0, 1, 2, 3}, (layout, parity)
            else:  # col = 3 near + far for each output row parity, then 3 col[i] + col[i -+ 1]
                rows = jo._edge(a, 0)
                for row_parity, col in (("even", 3 * a + rows[:-2]), ("odd", 3 * a + rows[2:])):
                    left, right = jo._edge(col, 1)[:, :-2], jo._edge(col, 1)[:, 2:]
                    for parity, sums in (("even", 3 * col + left), ("odd", 3 * col + right)):
                        assert set((sums % 16).reshape(-1).tolist()) == set(range(16)), (layout, row_parity, parity)


def test_sweep_oracle_equals_pillow():
    pytest.importorskip("PIL")
    for layout in LAYOUTS:
        for size in SWEEP:
            data = sweep_streams(layout)[size]
            assert_oracle_equals_pillow(data, (layout, size))
    for layout in ("422", "420"):
        assert_oracle_equals_pillow(dense_chroma_stream(layout), ("dense chroma", layout))


def test_mid_size_oracle_equals_pillow():
    pytest.importorskip("PIL")
    for layout in LAYOUTS:
        for size in MID[layout]:
            data = sweep_streams(layout)[size]
            assert in_int16_domain(data), (layout, size)
            assert_oracle_equals_pillow(data, (layout, size))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_every_small_size_and_the_mid_sizes_equal_the_oracle(layout):
    for size, data in sweep_streams(layout).items():
        assert_device_equals_oracle(data, (layout, size))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["422", "420"])
def test_dense_chroma_equals_the_oracle(layout):
    assert_device_equals_oracle(dense_chroma_stream(layout), ("dense chroma", layout))


# ------------------------------------------------------------------------------------------------ e. extreme shapes
EXTREME = [(layout, w, h) for layout in ("gray", "420") for w, h in ((32768, 1), (1, 32768))]


@functools.lru_cache(maxsize=None)
def extreme_stream(layout, w, h):
    comps = LAYOUTS[layout]
    rng = np.random.default_rng([16, sorted(LAYOUTS).index(layout), w])
    return jf.write_jpeg(w, h, comps, jf.random_blocks(rng, w, h, comps, amplitude=0), FLAT, segments=[jf.jfif()])


def test_extreme_streams_have_the_largest_accepted_dimension():
    for layout, w, h in EXTREME:
        data = extreme_stream(layout, w, h)
        info = dataset.jpeg_info(data)
        assert info[:2] == (w, h) and info[3] == (0 if layout == "gray" else 3)
        s, blocks = jo.coefficients(data)
        assert all((b[:, :, 1:] == 0).all() for b in blocks) and all(len(np.unique(b[:, :, 0])) > 50 for b in blocks)  # DC-only, not flat
        if layout == "420":
            assert (s.comps[1]["dw"], s.comps[1]["dh"]) == ((16384, 1) if w == 32768 else (1, 16384))
    # one more in either direction is refused
    for w, h in ((32769, 1), (1, 32769)):
        with pytest.raises(ValueError, match="dimensions"):
            dataset.jpeg_info(jf.write_jpeg(w, h, jf.GRAY, [np.zeros((-(-h // 8), -(-w // 8), 64), dtype=np.int16)], FLAT, segments=[jf.jfif()]))


@pytest.mark.gpu
@pytest.mark.parametrize("layout,w,h", EXTREME)
def test_extreme_shapes_equal_the_oracle(layout, w, h):
    assert_device_equals_oracle(extreme_stream(layout, w, h), (layout, w, h))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,pad", [(1, 32768, 3), (32768, 1, 5)])
def test_extreme_shapes_with_a_row_stride_above_the_width_leave_the_padding_untouched(w, h, pad):
    data = extreme_stream("420", w, h)
    lib = _lib.load()
    for dev_mode, ora_mode in MODES:
        want = jo.decode_gray(data, ora_mode)
        for _ in range(2):  # the same bytes both times
            out = np.full((h, w + pad), 0xAB, dtype=np.uint8)
            _lib.check(lib.nidreg_jpeg_decode_gray(0, data, len(data), dev_mode, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), w + pad), "nidreg_jpeg_decode_gray")
            assert np.array_equal(out[:, :w], want) and (out[:, w:] == 0xAB).all()


# ------------------------------------------------------------------------------------------------ f. DC past int16, categories 15
def wrap16(v):
    return (np.asarray(v, dtype=np.int64) + 32768) % 65536 - 32768


@functools.lru_cache(maxsize=None)
def dc_walk_stream():
    """(the stream, the unwrapped DC values): gray, table all 1, 40 blocks whose DC differences are + 2047 each.  The writer gets
    the running sums themselves, in a wide integer array."""
    blocks = np.zeros((1, 40, 64), dtype=np.int64)
    blocks[0, :, 0] = 2047 * np.arange(1, 41)
    return jf.write_jpeg(320, 8, jf.GRAY, [blocks], {0: np.full(64, 1)}, segments=[jf.jfif()]), blocks[0, :, 0].copy()


@functools.lru_cache(maxsize=None)
def category15_stream():
    """(the stream, its blocks): one DC difference of category 15 in each direction and AC coefficients of +-32767"""
    blocks = np.zeros((1, 4, 64), dtype=np.int16)
    blocks[0, :, 0] = [-16384, 16383, 16383, -16384]  # differences -16384, +32767, 0, -32767
    blocks[0, 1, 1] = 32767
    blocks[0, 2, 8] = -32767
    blocks[0, 3, 63] = 32767
    return jf.write_jpeg(32, 8, jf.GRAY, [blocks], {0: np.full(64, 1)}, segments=[jf.jfif()]), blocks


def library_coefficients(data, count):
    out = np.full(count, 0x5A5A, dtype=np.int16)
    rc = _lib.load().nidreg_jpeg_coefficients(data, len(data), 0, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), count, None)
    assert rc == _lib.NIDREG_OK, _lib.last_error()
    return out


def test_dc_predictions_past_int16_are_stored_reduced_by_oracle_and_library():
    data, sums = dc_walk_stream()
    assert sums.max() == 81880 and (np.diff(sums, prepend=0) == 2047).all()
    _s, blocks = jo.coefficients(data)  # (raised OverflowError before the oracle reduced what it stores)
    assert blocks[0].dtype == np.int16 and np.array_equal(blocks[0][0, :, 0], wrap16(sums)) and (blocks[0][:, :, 1:] == 0).all()
    assert blocks[0][0, 15, 0] == 32752 and blocks[0][0, 16, 0] == -30737 and blocks[0][0, 39, 0] == 81880 - 65536
    assert np.array_equal(library_coefficients(data, 40 * 64).reshape(1, 40, 64), blocks[0])
    plane = jo.decode_gray(data, jo.LUMA)
    assert plane[0, 8 * 15] == 255 and plane[0, 8 * 16] == 0  # the wrap is in the picture


def test_categories_15_are_accepted_by_oracle_and_library():
    data, want = category15_stream()
    s = jo.parse(data)
    assert 15 in s.huff[(0, 0)].values() and {0x0F, 0x1F, 0xEF, 0xF0} <= set(s.huff[(1, 0)].values())  # DC category 15; AC size 15 after runs of 0, 1 and 3 x 16 + 14
    _s, blocks = jo.coefficients(data)
    assert np.array_equal(blocks[0], want)
    assert np.array_equal(library_coefficients(data, want.size).reshape(want.shape), want)


def test_writer_refuses_a_dc_difference_of_category_16():
    """DC values wrapped to int16 beforehand turn a difference of + 2047 into one of - 63489: no stream may hold that"""
    _data, sums = dc_walk_stream()
    blocks = np.zeros((1, 40, 64), dtype=np.int16)
    blocks[0, :, 0] = wrap16(sums)
    with pytest.raises(AssertionError, match="category"):
        jf.write_jpeg(320, 8, jf.GRAY, [blocks], {0: np.full(64, 1)}, segments=[jf.jfif()])


@pytest.mark.gpu
def test_dc_past_int16_equals_the_oracle():
    assert_device_equals_oracle(dc_walk_stream()[0], "DC walk")


@pytest.mark.gpu
def test_categories_15_equal_the_oracle():
    assert_device_equals_oracle(category15_stream()[0], "categories 15")
