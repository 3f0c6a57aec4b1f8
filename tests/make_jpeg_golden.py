"""Writes tests/golden/jpeg_cases.npz: per case the stream's bytes (``<name>.jpg``), Pillow's Y plane (libjpeg-turbo asked for
grayscale through ``draft('L')``, what ``cv::imread(path, 0)`` gets; stored as ``<name>.ydx``, its horizontal differences modulo 256,
which compress better) and Pillow's RGB decode taken through OpenCV's fixed-point luma (what ``cv_bridge`` gives as mono8; stored as
``<name>.gmy``, its difference from the Y plane modulo 256, and only where the two differ).  ``jpeg_oracle.load_cases`` reads it.  Run where Pillow exists:

    python tests/make_jpeg_golden.py
    python tests/make_jpeg_golden.py --dump-streams DIR     (no Pillow needed: the committed streams, one file each)

Every stream is deterministic (seeded).  The generator asserts, for every stream, that all dequantised coefficients and all
column-pass outputs of the inverse DCT fit in int16: the domain in which libjpeg's C code, libjpeg-turbo's SIMD code and this
project's decoder must all agree (beyond it the SIMD code's 16-bit intermediates differ from the 32-bit ones)."""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import jpeg_fixture as jf  # noqa: E402
import jpeg_oracle as jo  # noqa: E402

SIZES = [(1, 1), (8, 8), (9, 8), (3, 2), (4, 5), (5, 3), (17, 17), (33, 19), (16, 9), (2, 40), (1, 7)]
SAMPLINGS = {"gray": None, "444": "4:4:4", "422": "4:2:2", "420": "4:2:0"}
LAYOUTS = {"gray": jf.GRAY, "444": jf.YCC444, "422": jf.YCC422, "420": jf.YCC420}
FLAT = {0: np.full(64, 3), 1: np.full(64, 5)}


def pillow_encode(pixels, quality, sampling, optimize=False):
    from PIL import Image

    out = io.BytesIO()
    kw = {} if sampling is None else {"subsampling": sampling}
    Image.fromarray(pixels, "L" if pixels.ndim == 2 else "RGB").save(out, "JPEG", quality=quality, optimize=optimize, **kw)
    return out.getvalue()


def pillow_decode(data):
    """(Y plane, gray of the RGB decode)"""
    from PIL import Image

    im = Image.open(io.BytesIO(data))
    im.draft("L", im.size)
    assert im.mode == "L"
    y = np.asarray(im).copy()
    rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    return y, jo.cv_luma(rgb)


def scene_frame():
    """The 640 x 480 image of the synthetic scene the end-to-end tests use, with its equalisation undone and a tint that varies over
    the image, so that the chroma planes are not flat"""
    from direct_visual_lidar_calibration_amd import synth

    scene = synth.make_scene("pinhole_vga", num_points=1000, seed=30)
    raw = (scene.image_u8 // 2 + 40).astype(np.int64)
    yy, xx = np.mgrid[0 : raw.shape[0], 0 : raw.shape[1]]
    rgb = np.stack([raw + (xx * 60 // raw.shape[1]) - 30, raw + 10 - (yy * 40 // raw.shape[0]), raw + ((xx + yy) % 64) - 32], axis=2)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def synthetic_cases():
    rng = np.random.default_rng(2024)
    cases = {}
    # DRI = 1 over 11 MCUs: RST0 .. RST7, RST0, RST1
    cases["dri1_gray"] = jf.write_jpeg(88, 8, jf.GRAY, jf.random_blocks(rng, 88, 8, jf.GRAY), FLAT, dri=1, segments=[jf.jfif()])
    cases["dri1_420"] = jf.write_jpeg(130, 20, jf.YCC420, jf.random_blocks(rng, 130, 20, jf.YCC420), FLAT, dri=1, segments=[jf.jfif()])
    # DRI = 3 over 7 MCUs: the last interval holds one
    cases["dri3_422"] = jf.write_jpeg(100, 7, jf.YCC422, jf.random_blocks(rng, 100, 7, jf.YCC422), FLAT, dri=3, segments=[jf.jfif()])
    # 0xFF fill bytes before every RSTn
    cases["fill_444"] = jf.write_jpeg(40, 8, jf.YCC444, jf.random_blocks(rng, 40, 8, jf.YCC444), FLAT, dri=2, fill_before_rst=3, segments=[jf.jfif()])
    # stuffed 0xFF00: dense blocks of large coefficients, whose codes and extra bits hold runs of ones across byte boundaries
    cases["stuffed_gray"] = jf.write_jpeg(128, 32, jf.GRAY, jf.random_blocks(rng, 128, 32, jf.GRAY, amplitude=255, density=0.6), {0: np.full(64, 1)}, segments=[jf.jfif()])
    assert cases["stuffed_gray"].count(b"\xff\x00") >= 3
    # ZRL runs, a coefficient at position 63 (no EOB), a block with nothing but position 63
    blocks = jf.random_blocks(rng, 24, 8, jf.GRAY, amplitude=0)
    z = np.zeros((3, 64), dtype=np.int16)
    z[0, [1, 40, 63]] = [5, -3, 2]
    z[1, 63] = -7
    z[2, [17, 34, 62]] = [1, -1, 9]
    blocks[0][0, :, :][:, jo.ZIGZAG] = z
    cases["zrl_gray"] = jf.write_jpeg(24, 8, jf.GRAY, blocks, FLAT, segments=[jf.jfif()])
    # 16-bit DQT entries (SOF1: extended sequential, Huffman, 8-bit samples)
    blocks = jf.random_blocks(rng, 20, 20, jf.YCC420, amplitude=2)
    for b in blocks:
        b[:, :, 0] //= 8  # (the column pass scales by 4: its outputs must stay within int16)
    cases["dqt16_420"] = jf.write_jpeg(20, 20, jf.YCC420, blocks, {0: np.arange(64) * 9 + 260, 1: np.full(64, 300)}, sof=0xC1,
                                       dqt16=True, segments=[jf.jfif()])
    # Huffman codes of every length 1 .. 16: 15 blocks with one AC coefficient each, 15 different (run, size) symbols, and EOB
    blocks = jf.random_blocks(rng, 120, 8, jf.GRAY, amplitude=0)
    symbols = []
    for i in range(15):
        run, size = i % 5, 1 + i % 7
        zz = np.zeros(64, dtype=np.int16)
        zz[1 + run] = (1 << size) - 1 if i % 2 else -(1 << (size - 1))
        blocks[0][0, i][jo.ZIGZAG] = zz
        symbols.append((run << 4) | size)
    assert len(set(symbols)) == 15
    lengths = {s: 16 - k for k, s in enumerate(symbols)}  # the first block's symbol gets the 16-bit code
    lengths[0x00] = 1
    cases["huff16_gray"] = jf.write_jpeg(120, 8, jf.GRAY, blocks, FLAT, ac_lengths={0: lengths}, segments=[jf.jfif()])
    # DC differences of category 11
    blocks = jf.random_blocks(rng, 48, 8, jf.GRAY, amplitude=2)
    blocks[0][0, :, 0] = [1023, -1024, 1023, -1024, 1000, -1000]
    cases["dc11_gray"] = jf.write_jpeg(48, 8, jf.GRAY, blocks, {0: np.full(64, 1)}, segments=[jf.jfif()])
    # DQT all 255: blocks that saturate at both ends, inside the int16 domain
    blocks = jf.random_blocks(rng, 32, 8, jf.YCC444, amplitude=0)
    for b in blocks:
        b[:, :, 0] = 0
    blocks[0][0, 0, 1] = 32
    blocks[0][0, 1, 8] = -23  # (a vertical frequency gains 1.39 in the column pass, which also scales by 4)
    blocks[0][0, 2, [0, 9]] = [4, 22]
    blocks[0][0, 3, [1, 8]] = [20, 20]
    blocks[1][0, 0, 1] = 30
    blocks[2][0, 1, 8] = 23
    cases["saturate_444"] = jf.write_jpeg(32, 8, jf.YCC444, blocks, {0: np.full(64, 255), 1: np.full(64, 255)}, segments=[jf.jfif()])
    # no JFIF but Adobe transform 1; a COM and an APP2 segment, Exif orientation, one DHT segment per table, bytes after EOI
    cases["adobe_420"] = jf.write_jpeg(19, 21, jf.YCC420, jf.random_blocks(rng, 19, 21, jf.YCC420), FLAT,
                                       segments=[jf.segment(0xFE, b"a comment"), jf.adobe(1), jf.segment(0xE2, b"ICC_PROFILE\0" + bytes(40)), jf.exif(6, little_endian=False, extra_entries=2)],
                                       split_tables=True, tail=b"\xff\xd9trailing bytes \xff\xda\x00")
    # no marker at all: YCbCr
    cases["nomarker_422"] = jf.write_jpeg(9, 5, jf.YCC422, jf.random_blocks(rng, 9, 5, jf.YCC422), FLAT)
    return cases


def pillow_cases():
    rng = np.random.default_rng(7)
    cases = {}
    for k, (w, h) in enumerate(SIZES):
        for name, sampling in SAMPLINGS.items():
            pixels = rng.integers(0, 256, (h, w) if sampling is None else (h, w, 3), dtype=np.uint8)
            q = (30, 95)[k % 2]
            cases[f"size_{name}_{w}x{h}"] = pillow_encode(pixels, q, sampling, optimize=q == 30)
    for n in (1, 7, 8, 9):  # blocks: the tail of the 8-block IDCT workgroup
        cases[f"blocks_{n}"] = pillow_encode(rng.integers(0, 256, (8, 8 * n), dtype=np.uint8), 75, None)
    for w in range(1, 10):  # the 4-pixel store tail of the colour kernel
        cases[f"width_444_{w}"] = pillow_encode(rng.integers(0, 256, (3, w, 3), dtype=np.uint8), 85, "4:4:4")
    cases["frame_420"] = pillow_encode(scene_frame(), 50, "4:2:0")
    return cases


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--dump-streams":  # the committed streams as files (for tools/jpeg_parse_check.cpp)
        os.makedirs(sys.argv[2], exist_ok=True)
        for name, (data, _y, _g) in jo.load_cases(os.path.join(HERE, "golden", "jpeg_cases.npz")).items():
            with open(os.path.join(sys.argv[2], name + ".jpg"), "wb") as f:
                f.write(data)
        return
    cases = {**pillow_cases(), **synthetic_cases()}
    arrays = {}
    for name, data in cases.items():
        report = {}
        jo.decode_planes(data, report)
        assert report["deq"] <= 32767 and report["pass1"] <= 32767, (name, report)
        y, g = pillow_decode(data)
        assert np.array_equal(jo.decode_gray(data, jo.LUMA), y) and np.array_equal(jo.decode_gray(data, jo.BGR), g), name
        arrays[name + ".jpg"] = np.frombuffer(data, dtype=np.uint8)
        arrays[name + ".ydx"] = np.diff(y, axis=1, prepend=np.uint8(0))  # modulo 256; jpeg_oracle.load_cases undoes it
        if not np.array_equal(y, g):
            arrays[name + ".gmy"] = g - y  # modulo 256
    path = os.path.join(HERE, "golden", "jpeg_cases.npz")
    np.savez_compressed(path, **arrays)
    print(f"{len(cases)} cases, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
