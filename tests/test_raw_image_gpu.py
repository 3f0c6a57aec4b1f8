"""GPU tests of the raw image encodings (nidreg_image_to_mono8): Bayer mosaics, packed YUV 4:2:2 and 16-bit images against the numpy
restatement of tests/raw_image_oracle.py, byte for byte -- both parities of the size in each direction, widths on either side of the
4-pixel store and of a wave's row, the smallest legal mosaic, odd row steps, output strides whose padding must stay, saturation, byte
order, every 16-bit value, and source bytes at an odd address.  The rules are unpinned against OpenCV and cv_bridge."""
import ctypes

import numpy as np
import pytest

import raw_image_oracle as ro
import rosbag1_fixture as fx
from direct_visual_lidar_calibration_amd import _lib, rosbag1

pytestmark = pytest.mark.gpu


def convert(data, width, height, step, encoding, is_bigendian=0, pad=0):
    """Through the ABI from the array ``data`` as it lies; ``pad`` bytes of 0xAB behind every output row must survive"""
    data = np.asarray(data, dtype=np.uint8)
    out = np.full((height, width + pad), 0xAB, dtype=np.uint8)
    rc = _lib.load().nidreg_image_to_mono8(0, data.ctypes.data, data.size, width, height, step, encoding.encode(), is_bigendian, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                           width + pad if pad else 0)
    _lib.check(rc, "nidreg_image_to_mono8")
    assert (out[:, width:] == 0xAB).all()
    return out[:, :width]


def random_image(width, height, encoding, step_pad, seed):
    """``(bytes as a uint8 array, step)``: random samples, the padding of every row random too"""
    step = width * ro.bytes_per_pixel(encoding) + step_pad
    return np.random.default_rng(seed).integers(0, 256, height * step, dtype=np.uint8), step


def check(width, height, encoding, step_pad=0, is_bigendian=0, pad=0, seed=1):
    data, step = random_image(width, height, encoding, step_pad, seed)
    got = convert(data, width, height, step, encoding, is_bigendian, pad)
    assert np.array_equal(got, ro.to_mono8(data, width, height, step, encoding, is_bigendian)), (encoding, width, height, step_pad, pad)


@pytest.mark.parametrize("encoding", ro.BAYER_ENCODINGS)
def test_bayer_at_the_sizes_around_the_store_width_the_waves_row_and_the_smallest_mosaic(encoding):
    for k, (width, height) in enumerate([(3, 3), (4, 3), (3, 4), (5, 5), (8, 3), (9, 7), (31, 5), (33, 19), (64, 8)]):
        check(width, height, encoding, seed=10 + k)


@pytest.mark.parametrize("encoding", ro.BAYER_ENCODINGS)
def test_bayer_with_odd_row_steps_and_output_strides_that_keep_their_padding(encoding):
    check(33, 19, encoding, step_pad=3, seed=20)
    for pad in (1, 3, 7):
        check(33, 19, encoding, step_pad=3, pad=pad, seed=21 + pad)


def test_saturation_all_ones_in_255_out_and_a_checkerboard_of_0_and_65535():
    yy, xx = np.mgrid[0:9, 0:14]
    board = np.where((xx + yy) % 2 == 0, 0, 65535).astype("<u2")
    for pattern in ro.BAYER:
        assert (convert(np.full(9 * 14, 255, dtype=np.uint8), 14, 9, 14, f"bayer_{pattern}8") == 255).all()
        assert (convert(np.full(9 * 28, 255, dtype=np.uint8), 14, 9, 28, f"bayer_{pattern}16") == 255).all()
        for b in (board, 65535 - board):
            data = np.frombuffer(b.tobytes(), dtype=np.uint8)
            got = convert(data, 14, 9, 28, f"bayer_{pattern}16")
            assert np.array_equal(got, ro.to_mono8(data, 14, 9, 28, f"bayer_{pattern}16")) and 0 < got.min() and got.max() < 255
    for encoding in ("mono16",) + ro.COLOR16_ENCODINGS:
        bpp = ro.bytes_per_pixel(encoding)
        assert (convert(np.full(5 * 7 * bpp, 255, dtype=np.uint8), 7, 5, 7 * bpp, encoding) == 255).all()


@pytest.mark.parametrize("encoding", ["mono16", "bayer_grbg16", "rgb16"])
def test_big_endian_samples_are_swapped_first(encoding):
    data, step = random_image(13, 7, encoding, 0, seed=30)
    swapped = data.reshape(-1, 2)[:, ::-1].reshape(-1).copy()
    little = convert(data, 13, 7, step, encoding)
    assert np.array_equal(little, ro.to_mono8(data, 13, 7, step, encoding)) and np.array_equal(convert(swapped, 13, 7, step, encoding, is_bigendian=1), little)
    assert np.array_equal(ro.to_mono8(swapped, 13, 7, step, encoding, 1), little) and not np.array_equal(convert(swapped, 13, 7, step, encoding), little)


def test_8_bit_encodings_ignore_the_byte_order_flag():
    for encoding in ("bayer_rggb8", "yuv422", "rgb8"):
        data, step = random_image(9, 5, encoding, 1, seed=31)
        assert np.array_equal(convert(data, 9, 5, step, encoding, is_bigendian=1), ro.to_mono8(data, 9, 5, step, encoding))


def test_mono16_over_every_value():
    table = np.random.default_rng(32).permutation(65536).astype("<u2").reshape(256, 256)
    data = np.frombuffer(table.tobytes(), dtype=np.uint8)
    got = convert(data, 256, 256, 512, "mono16")
    assert np.array_equal(got, ((table.astype(np.int64) + 128) // 257).astype(np.uint8)) and np.array_equal(got, ro.to_mono8(data, 256, 256, 512, "mono16"))


@pytest.mark.parametrize("encoding", ro.COLOR16_ENCODINGS)
def test_16_bit_colour_with_step_padding(encoding):
    check(13, 7, encoding, step_pad=5, seed=33)
    check(13, 7, encoding, step_pad=5, is_bigendian=1, pad=3, seed=34)


@pytest.mark.parametrize("encoding", sorted(ro.YUV))
@pytest.mark.parametrize("width", [1, 2, 5, 33])
def test_packed_yuv_takes_the_y_byte(encoding, width):
    height, step = 6, 2 * width + 3
    rows = np.full((height, step), 0xEE, dtype=np.uint8)
    y = np.random.default_rng(35 + width).integers(0, 128, (height, width), dtype=np.uint8)  # Y below 128, U and V 128 and above: a wrong byte shows
    rows[:, ro.YUV[encoding] : 2 * width : 2] = y
    rows[:, 1 - ro.YUV[encoding] : 2 * width : 2] = 128 + (np.arange(width) % 2) * 64 + np.arange(height)[:, None]
    got = convert(rows.reshape(-1), width, height, step, encoding, pad=1)
    assert np.array_equal(got, y) and np.array_equal(got, ro.to_mono8(rows.reshape(-1), width, height, step, encoding))


@pytest.mark.parametrize("encoding", ro.EIGHT_BIT_ENCODINGS)
def test_the_five_8_bit_encodings_through_the_abi_equal_to_mono8(encoding):
    ch = ro.bytes_per_pixel(encoding)
    px = np.random.default_rng(36).integers(0, 256, (19, 33, ch) if ch > 1 else (19, 33), dtype=np.uint8)
    msg = rosbag1.decode_image(fx.image((1, 2), px, encoding, step=33 * ch + 3))
    want = rosbag1.to_mono8(msg)
    assert np.array_equal(convert(msg.data, 33, 19, msg.step, encoding, pad=3), want) and np.array_equal(ro.to_mono8(msg.data, 33, 19, msg.step, encoding), want)


@pytest.mark.parametrize("encoding", ["bayer_gbrg16", "mono16", "rgba16", "yuyv", "bayer_bggr8"])
def test_a_source_at_an_odd_host_address_gives_the_same_bytes(encoding):
    data, step = random_image(33, 9, encoding, 3, seed=37)
    larger = np.zeros(data.size + 17, dtype=np.uint8)
    offset = 1 if larger.ctypes.data % 2 == 0 else 2
    view = larger[offset : offset + data.size]
    view[:] = data
    assert view.ctypes.data % 2 == 1
    assert np.array_equal(convert(view, 33, 9, step, encoding), convert(data, 33, 9, step, encoding))
    msg = rosbag1.Image((0, 0), "camera", 9, 33, encoding, 0, step, view)
    assert np.array_equal(rosbag1.image_to_mono8(msg), ro.to_mono8(data, 33, 9, step, encoding))


def test_the_timing_of_the_last_call_is_reported():
    check(64, 8, "bayer_rggb8", seed=38)
    ms = (ctypes.c_double * 3)()
    assert _lib.load().nidreg_image_get_timing(ms) == 0 and all(v >= 0.0 for v in ms) and ms[1] > 0.0
