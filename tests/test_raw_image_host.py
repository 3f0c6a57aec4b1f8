"""Host tests of the raw image encodings (Bayer, packed YUV 4:2:2, 16 bit): the numpy restatement (tests/raw_image_oracle.py) against
properties that do not rest on a second restatement -- a mosaic sampled from a linear colour field demosaics to the field's luma
exactly, which a swapped R / B, a wrong pattern phase, a swapped horizontal / vertical pair at green pixels or a wrong rounding all
break --, the depth-change identity over all 65536 values, and every refusal of nidreg_image_to_mono8, which validates before it
touches a device and so runs on a machine without one.  The rules are unpinned against OpenCV and cv_bridge."""
import ctypes

import numpy as np
import pytest

import raw_image_oracle as ro
import rosbag1_fixture as fx
from direct_visual_lidar_calibration_amd import _lib, rosbag1, rosbag2

FIELD = {"r": (3, 5, 10), "g": (7, 2, 20), "b": (2, 9, 5)}  # a x + b y + c: R != B everywhere, the slopes in x and y differ; at most 127 at 13 x 7


def _field(width, height):
    yy, xx = np.mgrid[0:height, 0:width].astype(np.int64)
    return {k: a * xx + b * yy + c for k, (a, b, c) in FIELD.items()}


def _mosaic(pattern, width, height, scale):
    f = _field(width, height)
    red, green, blue = ro.color_masks(pattern, width, height)
    return scale * np.where(red, f["r"], np.where(green, f["g"], f["b"]))


@pytest.mark.parametrize("pattern", ro.BAYER)
@pytest.mark.parametrize("width,height", [(3, 3), (5, 4), (4, 5), (13, 7)])
@pytest.mark.parametrize("bits", [8, 16])
def test_a_mosaic_of_a_linear_colour_field_gives_the_luma_of_the_field(pattern, width, height, bits):
    scale = 1 if bits == 8 else 257
    p = _mosaic(pattern, width, height, scale)
    assert p.max() < 256 * scale and len({int(p[0, 0]), int(p[0, 1]), int(p[1, 0]), int(p[1, 1])}) >= 3
    data = p.astype("<u2" if bits == 16 else np.uint8).tobytes()
    got = ro.to_mono8(data, width, height, width * bits // 8, f"bayer_{pattern}{bits}")
    f = _field(width, height)
    want = ro.luma(scale * f["r"], scale * f["g"], scale * f["b"])
    if bits == 16:
        want = ro.depth8(want)
    assert np.array_equal(got[1:-1, 1:-1], want[1:-1, 1:-1])
    # the border: the interior pixel at the clamped coordinate
    yc, xc = np.clip(np.arange(height), 1, height - 2), np.clip(np.arange(width), 1, width - 2)
    assert np.array_equal(got, got[np.ix_(yc, xc)]) and np.array_equal(got, want[np.ix_(yc, xc)])


def test_the_linear_field_tells_the_colours_and_directions_apart():
    """The property has teeth: R and B differ by more than the rounding, and so do the two directions"""
    f = _field(13, 7)
    assert (np.abs(ro.luma(f["r"], f["g"], f["b"]) - ro.luma(f["b"], f["g"], f["r"]))[1:-1, 1:-1] >= 1).any()
    p = _mosaic("rggb", 13, 7, 1)
    assert not np.array_equal(ro.bayer_gray(p, "rggb"), ro.bayer_gray(p, "bggr")) and not np.array_equal(ro.bayer_gray(p, "rggb"), ro.bayer_gray(p, "grbg"))
    # the horizontal and vertical pairs at the green pixels swapped: red and blue trade places there
    green = ro.color_masks("rggb", 13, 7)[1]
    assert ((ro.C_R - ro.C_B) * np.abs(f["r"] - f["b"])[1:-1, 1:-1][green[1:-1, 1:-1]] >= 2 * 2**14).any()


@pytest.mark.parametrize("pattern", ro.BAYER)
def test_an_all_65535_mosaic_gives_255_everywhere(pattern):
    data = np.full((5, 6), 65535, dtype="<u2").tobytes()
    assert (ro.to_mono8(data, 6, 5, 12, f"bayer_{pattern}16") == 255).all()
    assert (ro.bayer_gray(np.full((5, 6), 65535), pattern) == 65535).all()  # 4 * 65535 * 16384 + 2^15 < 2^32: no wrap in unsigned 32 bit
    assert 4 * 65535 * 16384 + 2**15 < 2**32 and 4 * 65535 * 16384 + 2**15 >= 2**31


def test_the_depth_change_is_cv_bridges_float32_rounding_for_every_value():
    v = np.arange(65536)
    assert np.array_equal(ro.depth8(v), ro.depth8_float(v))
    assert ro.depth8(0) == 0 and ro.depth8(128) == 0 and ro.depth8(129) == 1 and ro.depth8(65535) == 255


def test_byte_order_packed_yuv_and_colour_of_the_oracle():
    le = np.array([[0x1234, 0xFF00, 0x00FF]], dtype="<u2")
    assert np.array_equal(ro.samples(le.tobytes(), 3, 1, 6, "mono16"), [[0x1234, 0xFF00, 0x00FF]])
    assert np.array_equal(ro.samples(le.astype(">u2").tobytes(), 3, 1, 6, "mono16", 1), [[0x1234, 0xFF00, 0x00FF]])
    row = bytes([200, 10, 201, 11, 202, 12])  # three pixels
    assert np.array_equal(ro.to_mono8(row, 3, 1, 6, "yuv422"), [[10, 11, 12]]) and np.array_equal(ro.to_mono8(row, 3, 1, 6, "uyvy"), [[10, 11, 12]])
    assert np.array_equal(ro.to_mono8(row, 3, 1, 6, "yuv422_yuy2"), [[200, 201, 202]]) and np.array_equal(ro.to_mono8(row, 3, 1, 6, "yuyv"), [[200, 201, 202]])
    px = np.array([[1000, 20000, 65535, 7]], dtype="<u2")  # one rgba16 pixel
    assert ro.to_mono8(px.tobytes(), 1, 1, 8, "rgba16")[0, 0] == ((4899 * 1000 + 9617 * 20000 + 1868 * 65535 + 8192) // 16384 + 128) // 257
    assert ro.to_mono8(px.tobytes(), 1, 1, 8, "bgra16")[0, 0] == ((1868 * 1000 + 9617 * 20000 + 4899 * 65535 + 8192) // 16384 + 128) // 257


# ---------------------------------------------------------------------------------------------- the library's refusals, no GPU needed
def _call(data, width, height, step, encoding, is_bigendian=0, out=None, out_row_stride=0, size=None, null_data=False, null_out=False):
    lib = _lib.load()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.full((8, 8), 0xAB, dtype=np.uint8) if out is None else out
    rc = lib.nidreg_image_to_mono8(0, None if null_data else buf.ctypes.data, len(buf) if size is None else size, width, height, step, encoding.encode() if encoding is not None else None,
                                   is_bigendian, None if null_out else out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), out_row_stride)
    assert (out == 0xAB).all()  # a refusal writes nothing
    return rc, _lib.last_error()


@pytest.mark.parametrize("encoding", ["8UC1", "16UC1", "32FC1", "nv21", "nv24", "bayer_rggb12", "MONO16", "", "yuv422_yuy"])
def test_every_other_encoding_is_refused_by_name(encoding):
    rc, msg = _call(bytes(64), 4, 4, 16, encoding)
    assert rc == _lib.NIDREG_ERR_INVALID and f"sensor_msgs/Image encoding '{encoding}' is not converted here (" in msg and "bayer" in msg and "mono16" in msg


@pytest.mark.parametrize("width,height,number", [(0, 4, "0 x 4"), (4, 0, "4 x 0"), (-1, 4, "-1 x 4"), (16385, 1, "16385 x 1"), (1, 16385, "1 x 16385")])
def test_a_size_outside_the_range_is_refused(width, height, number):
    rc, msg = _call(bytes(64), width, height, 70000, "mono16")
    assert rc == _lib.NIDREG_ERR_INVALID and "mono16" in msg and number in msg and "[1, 16384]" in msg


@pytest.mark.parametrize("encoding,width,height", [("bayer_rggb8", 2, 3), ("bayer_grbg16", 3, 2), ("bayer_bggr8", 1, 1), ("bayer_gbrg16", 2, 16)])
def test_a_mosaic_without_an_interior_is_refused(encoding, width, height):
    rc, msg = _call(bytes(256), width, height, 8, encoding)
    assert rc == _lib.NIDREG_ERR_INVALID and encoding in msg and f"{width} x {height}" in msg and "3 x 3" in msg


@pytest.mark.parametrize("encoding,bpp", [("mono16", 2), ("bayer_rggb8", 1), ("bayer_rggb16", 2), ("yuv422", 2), ("yuyv", 2), ("rgb16", 6), ("bgra16", 8), ("rgb8", 3), ("mono8", 1)])
def test_a_step_below_the_row_and_too_few_bytes_are_refused(encoding, bpp):
    assert ro.bytes_per_pixel(encoding) == bpp
    rc, msg = _call(bytes(1024), 5, 4, 5 * bpp - 1, encoding)
    assert rc == _lib.NIDREG_ERR_INVALID and encoding in msg and f"step {5 * bpp - 1} " in msg and f"{5 * bpp} bytes" in msg
    rc, msg = _call(bytes(4 * (5 * bpp + 3) - 1), 5, 4, 5 * bpp + 3, encoding)
    assert rc == _lib.NIDREG_ERR_INVALID and encoding in msg and f"{4 * (5 * bpp + 3) - 1} data bytes" in msg
    rc, msg = _call(bytes(64), 5, 4, 5 * bpp, encoding, size=-1)
    assert rc == _lib.NIDREG_ERR_INVALID and "-1 data bytes" in msg
    rc, msg = _call(bytes(64), 5, 4, 2**62, encoding)  # height * step does not fit 64 bits
    assert rc == _lib.NIDREG_ERR_INVALID and str(2**62) in msg


def test_null_pointers_and_a_short_output_stride_are_refused():
    for kw in ({"null_data": True}, {"null_out": True}):
        rc, msg = _call(bytes(64), 4, 4, 8, "mono16", **kw)
        assert rc == _lib.NIDREG_ERR_INVALID and "null" in msg and "mono16" in msg
    rc, msg = _call(bytes(64), 4, 4, 8, None)
    assert rc == _lib.NIDREG_ERR_INVALID and "null encoding" in msg
    for stride in (3, -1):
        rc, msg = _call(bytes(64), 4, 4, 8, "mono16", out_row_stride=stride)
        assert rc == _lib.NIDREG_ERR_INVALID and f"out_row_stride {stride} " in msg and "mono16" in msg
    assert _lib.load().nidreg_image_get_timing(None) == _lib.NIDREG_ERR_INVALID


# ---------------------------------------------------------------------------------------------- the Python surface
def test_image_to_mono8_on_the_five_8_bit_encodings_is_to_mono8_and_needs_no_gpu():
    rng = np.random.default_rng(3)
    assert rosbag2.image_to_mono8 is rosbag1.image_to_mono8
    for enc, ch in (("mono8", 1), ("rgb8", 3), ("bgr8", 3), ("rgba8", 4), ("bgra8", 4)):
        px = rng.integers(0, 256, (7, 9, ch) if ch > 1 else (7, 9), dtype=np.uint8)
        msg = rosbag1.decode_image(fx.image((1, 2), px, enc, step=9 * ch + 3))
        assert np.array_equal(rosbag1.image_to_mono8(msg), rosbag1.to_mono8(msg)), enc
        assert np.array_equal(rosbag1.to_mono8(msg), ro.to_mono8(msg.data, 9, 7, 9 * ch + 3, enc)), enc


def test_to_mono8_still_refuses_what_it_refused_and_image_to_mono8_refuses_the_rest():
    gray = np.zeros((4, 6), dtype=np.uint8)
    for enc in ("mono16", "bayer_rggb8"):
        with pytest.raises(ValueError, match=enc):
            rosbag1.to_mono8(rosbag1.decode_image(fx.image((1, 2), gray, enc)))
    with pytest.raises(ValueError, match=r"camera: .*encoding '16UC1' is not converted here"):
        rosbag1.image_to_mono8(rosbag1.decode_image(fx.image((1, 2), gray, "16UC1")), where="camera")
    with pytest.raises(ValueError, match=r"mono16 image of 6 x 4: step 6 is below the 12 bytes"):  # 6 bytes a row hold 3 pixels
        rosbag1.image_to_mono8(rosbag1.decode_image(fx.image((1, 2), gray, "mono16")))
    huge = rosbag1.Image((0, 0), "camera", 2**32 - 1, 2**32 - 1, "mono16", 0, 8, np.zeros(8, dtype=np.uint8))
    with pytest.raises(ValueError, match=r"\[1, 16384\]"):
        rosbag1.image_to_mono8(huge)
