"""The numpy restatement of the raw image encodings (include/nidreg.h: nidreg_image_to_mono8): every rule as plain int64 array
arithmetic, written from the rules' text and not from the kernels.  The rules restate cv_bridge::toCvCopy(msg, "mono8") and OpenCV
(the bilinear Bayer2Gray, channel extraction for packed YUV, convertTo for the depth change) from memory; they are unpinned against
OpenCV and cv_bridge.  Test infrastructure: tests/test_raw_image_*.py and tools/raw_image_time.py compare the device's bytes with
``to_mono8`` here."""
import numpy as np

C_R, C_G, C_B = 4899, 9617, 1868

BAYER = ("rggb", "bggr", "gbrg", "grbg")
BAYER_ENCODINGS = tuple(f"bayer_{p}{d}" for d in (8, 16) for p in BAYER)
COLOR = {"rgb": (0, 1, 2, 3), "bgr": (2, 1, 0, 3), "rgba": (0, 1, 2, 4), "bgra": (2, 1, 0, 4)}  # sample index of R, G, B; samples a pixel
COLOR16_ENCODINGS = tuple(n + "16" for n in COLOR)
EIGHT_BIT_ENCODINGS = ("mono8",) + tuple(n + "8" for n in COLOR)
YUV = {"yuv422": 1, "uyvy": 1, "yuv422_yuy2": 0, "yuyv": 0}  # the byte of a pixel's two that is its Y
ENCODINGS = EIGHT_BIT_ENCODINGS + ("mono16",) + COLOR16_ENCODINGS + tuple(YUV) + BAYER_ENCODINGS


def luma(r, g, b):
    return (C_R * np.asarray(r, dtype=np.int64) + C_G * np.asarray(g, dtype=np.int64) + C_B * np.asarray(b, dtype=np.int64) + 8192) >> 14


def depth8(v):
    """16 bit to 8 bit: cv_bridge's convertTo(CV_8U, 255 / 65535), as an integer"""
    return (np.asarray(v, dtype=np.int64) + 128) // 257


def depth8_float(v):
    """... and as cv_bridge computes it: float32, round half to even"""
    return np.rint(np.asarray(v).astype(np.float32) * np.float32(255.0 / 65535.0)).astype(np.int64)


def bytes_per_pixel(encoding):
    if encoding in YUV or encoding == "mono16":
        return 2
    if encoding.startswith("bayer_") or encoding == "mono8":
        return 2 if encoding.endswith("16") else 1
    name, depth = (encoding[:-2], 2) if encoding.endswith("16") else (encoding[:-1], 1)
    return COLOR[name][3] * depth


def samples(data, width, height, step, encoding, is_bigendian=0):
    """The image's samples as an int64 array (height, width * samples a pixel), from the bytes as stored"""
    bpp = bytes_per_pixel(encoding)
    rows = np.frombuffer(data, dtype=np.uint8, count=height * step).reshape(height, step)[:, : width * bpp].astype(np.int64)
    if encoding.endswith("16"):
        first, second = rows[:, 0::2], rows[:, 1::2]
        return first * 256 + second if is_bigendian else second * 256 + first
    return rows


def color_masks(pattern, width, height):
    """Boolean (height, width) masks of the red, green and blue pixels; the letters are row 0 (columns 0, 1), then row 1"""
    yy, xx = np.mgrid[0:height, 0:width]
    letter = np.array(list(pattern))[(yy % 2) * 2 + xx % 2]
    return letter == "r", letter == "g", letter == "b"


def bayer_gray(p, pattern):
    """The mosaic ``p`` (int64, at least 3 x 3) to gray, before any depth change"""
    p = np.asarray(p, dtype=np.int64)
    h, w = p.shape
    assert h >= 3 and w >= 3
    red, green, blue = color_masks(pattern, w, h)
    c = p[1:-1, 1:-1]
    left, right, up, down = p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]
    diagonal = p[:-2, :-2] + p[:-2, 2:] + p[2:, :-2] + p[2:, 2:]
    at_red = (C_R * 4 * c + C_G * (left + right + up + down) + C_B * diagonal + 2**15) >> 16
    at_blue = (C_B * 4 * c + C_G * (left + right + up + down) + C_R * diagonal + 2**15) >> 16
    green_red_beside = (C_R * (left + right) + C_B * (up + down) + C_G * 2 * c + 2**14) >> 15
    green_blue_beside = (C_B * (left + right) + C_R * (up + down) + C_G * 2 * c + 2**14) >> 15
    red_beside = np.zeros((h, w), dtype=bool)
    red_beside[:, 1:] |= red[:, :-1]
    red_beside[:, :-1] |= red[:, 1:]
    inner = lambda a: a[1:-1, 1:-1]  # noqa: E731
    interior = np.where(inner(red), at_red, np.where(inner(blue), at_blue, np.where(inner(red_beside), green_red_beside, green_blue_beside)))
    return np.pad(interior, 1, mode="edge")  # a border pixel repeats the interior pixel at the clamped coordinate


def to_mono8(data, width, height, step, encoding, is_bigendian=0):
    """(height, width) uint8: what nidreg_image_to_mono8 must give for an image it accepts"""
    s = samples(data, width, height, step, encoding, is_bigendian)
    if encoding in YUV:
        gray = s[:, YUV[encoding] :: 2]
    elif encoding.startswith("bayer_"):
        gray = bayer_gray(s, encoding[6:10])
    elif encoding.startswith("mono"):
        gray = s
    else:
        r, g, b, n = COLOR[encoding.rstrip("0123456789")]
        gray = luma(s[:, r::n], s[:, g::n], s[:, b::n])
    if encoding.endswith("16"):
        gray = depth8(gray)
    assert gray.shape == (height, width) and gray.min() >= 0 and gray.max() <= 255
    return gray.astype(np.uint8)
