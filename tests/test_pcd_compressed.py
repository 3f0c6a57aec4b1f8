"""Host tests of the compressed PCD route: the LZF decoder (csrc/nid_lzf_host.hpp) through its C entry point over the literal-run
packer and the hand-assembled streams of tests/las_oracle.py, and ``dataset.read_pcd`` of ``DATA binary_compressed`` against the same
cloud written as ``DATA binary``.  Unpinned against PCL / liblzf and real files.  No GPU."""
import ctypes
import struct

import numpy as np
import pytest

import las_oracle as lo
from direct_visual_lidar_calibration_amd import _lib, dataset


def lzf(stream, out_size):
    """(rc, error text, the bytes written) of nidreg_lzf_decompress into a buffer of exactly out_size bytes"""
    lib = _lib.load()
    out = ctypes.create_string_buffer(max(out_size, 1))
    written = ctypes.c_int64(-1)
    rc = lib.nidreg_lzf_decompress(bytes(stream) or None, len(stream), out, out_size, ctypes.byref(written))
    return rc, (_lib.last_error() if rc else ""), out.raw[: written.value]


def test_literal_streams_round_trip():
    rng = np.random.default_rng(3)
    for n in (0, 1, 31, 32, 33, 64, 1000):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        stream = lo.lzf_pack_literals(data)
        assert len(stream) == n + (n + 31) // 32
        rc, _, got = lzf(stream, n)
        assert rc == 0 and got == data
        assert np.array_equal(dataset.lzf_decompress(stream, n + 5), np.frombuffer(data, dtype=np.uint8))  # a larger buffer: the bytes written say how many


@pytest.mark.parametrize("name", sorted(k for k, v in lo.LZF_STREAMS.items() if v[1] is not None))
def test_back_references(name):
    stream, want = lo.LZF_STREAMS[name]
    rc, msg, got = lzf(stream, len(want))
    assert rc == 0 and got == want, msg
    # one byte less room: refused as an overrun, at the offset of the token that does not fit, and nothing is written past the buffer
    rc, msg, got = lzf(stream, len(want) - 1)
    assert rc == _lib.NIDREG_ERR_INVALID and "overruns the output" in msg and "input offset" in msg and got == want[: len(got)]
    # every proper prefix either decodes to a prefix of the output (it ends between two tokens) or is refused as ending inside a token
    for cut in range(len(stream)):
        rc, msg, got = lzf(stream[:cut], len(want))
        assert got == want[: len(got)]
        assert rc == 0 or (rc == _lib.NIDREG_ERR_INVALID and "ends inside" in msg and "input offset" in msg), (cut, msg)
    assert sum(lzf(stream[:cut], len(want))[0] != 0 for cut in range(max(0, len(stream) - 40), len(stream))) > 0


def test_refusals_give_the_input_offset():
    stream, _ = lo.LZF_STREAMS["reference_before_output"]
    rc, msg, got = lzf(stream, 16)
    assert rc == _lib.NIDREG_ERR_INVALID and "starts before the output" in msg and "input offset 2" in msg and got == b"a"
    rc, msg, _ = lzf(bytes([0x05, 1, 2, 3]), 16)  # a literal run of 6 with 3 bytes present
    assert rc == _lib.NIDREG_ERR_INVALID and "ends inside a literal run" in msg and "input offset 0" in msg
    rc, msg, _ = lzf(bytes([0x00, 7, 0xE0]), 16)  # the extension byte is missing
    assert rc == _lib.NIDREG_ERR_INVALID and "ends inside a back-reference" in msg and "input offset 2" in msg
    rc, msg, _ = lzf(bytes([0x00, 7, 0xE0, 4]), 16)  # the distance byte is missing
    assert rc == _lib.NIDREG_ERR_INVALID and "ends inside a back-reference" in msg and "input offset 2" in msg
    rc, msg, _ = lzf(bytes([0x20, 0x00]), 16)  # a reference as the first token: there is no output yet
    assert rc == _lib.NIDREG_ERR_INVALID and "starts before the output" in msg and "input offset 0" in msg
    lib = _lib.load()
    assert lib.nidreg_lzf_decompress(None, 4, ctypes.create_string_buffer(4), 4, None) == _lib.NIDREG_ERR_INVALID
    assert lib.nidreg_lzf_decompress(b"\0a", -1, ctypes.create_string_buffer(4), 4, None) == _lib.NIDREG_ERR_INVALID
    assert lib.nidreg_lzf_decompress(b"\0a", 2, None, 4, None) == _lib.NIDREG_ERR_INVALID
    assert lib.nidreg_lzf_decompress(b"\0a", 2, ctypes.create_string_buffer(4), 4, None) == 0  # `written` is optional
    with pytest.raises(ValueError, match="starts before the output"):
        dataset.lzf_decompress(stream, 16)


FIELDS, SIZES, TYPES, COUNTS = ["x", "normal", "y", "z", "label", "intensity"], [4, 4, 4, 4, 2, 4], ["F", "F", "F", "F", "U", "F"], [1, 3, 1, 1, 1, 1]


def header(n, data, fields=FIELDS, sizes=SIZES, types=TYPES, counts=COUNTS):
    return (f"# .PCD v0.7\nVERSION 0.7\nFIELDS {' '.join(fields)}\nSIZE {' '.join(map(str, sizes))}\nTYPE {' '.join(types)}\nCOUNT {' '.join(map(str, counts))}\n"
            f"WIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA {data}\n").encode("ascii")


def cloud(n, seed=5):
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, dtype=[("x", "<f4"), ("normal", "<f4", (3,)), ("y", "<f4"), ("z", "<f4"), ("label", "<u2"), ("intensity", "<f4")])
    rec["x"], rec["y"], rec["z"] = rng.uniform(-40, 40, (3, n)).astype(np.float32)
    rec["normal"], rec["label"], rec["intensity"] = rng.normal(size=(n, 3)), rng.integers(0, 65536, n), rng.uniform(0, 255, n)
    return rec


def planes(rec):
    """the body before compression: one plane per field in header order"""
    return b"".join(np.ascontiguousarray(rec[k]).tobytes() for k in rec.dtype.names)


def write_compressed(path, rec, stream=None, sizes=None, head=None):
    body = planes(rec)
    stream = lo.lzf_pack_literals(body) if stream is None else stream
    comp, uncomp = (len(stream), len(body)) if sizes is None else sizes
    with open(path, "wb") as f:
        f.write((header(len(rec), "binary_compressed") if head is None else head) + struct.pack("<II", comp, uncomp) + stream)


@pytest.mark.parametrize("n", [0, 1, 37, 1000])
def test_compressed_pcd_equals_the_binary_one(tmp_path, n):
    rec = cloud(n)
    a, b = str(tmp_path / "a.pcd"), str(tmp_path / "b.pcd")
    with open(a, "wb") as f:
        f.write(header(n, "binary") + rec.tobytes())
    write_compressed(b, rec)
    xyz_a, inten_a = dataset.read_pcd(a)
    xyz_b, inten_b = dataset.read_pcd(b)
    assert xyz_b.dtype == np.float32 and inten_b.dtype == np.float32 and xyz_b.shape == (n, 3)
    assert np.array_equal(xyz_a.view(np.uint32), xyz_b.view(np.uint32)) and np.array_equal(inten_a.view(np.uint32), inten_b.view(np.uint32))
    if n:
        assert np.array_equal(xyz_b[:, 1], rec["y"]) and np.array_equal(inten_b, rec["intensity"])  # the COUNT 3 plane between x and y was skipped by its width


def test_compressed_pcd_with_back_references_and_without_intensity(tmp_path):
    n = 8
    rec = np.zeros(n, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
    rec["x"], rec["y"], rec["z"] = 1.5, 1.5, 1.5  # 96 bytes of one repeated float: four literal bytes, then references at distance 4
    stream = bytes([0x03]) + np.float32(1.5).tobytes() + bytes([0xE0, 80, 0x03])  # length 7 + 80 + 2 = 89 ...
    stream += bytes([(1 << 5) | 0, 0x03])  # ... and the shortest reference there is, 3 bytes: 4 + 89 + 3 = 96
    path = str(tmp_path / "c.pcd")
    write_compressed(path, rec, stream=stream, head=header(n, "binary_compressed", ["x", "y", "z"], [4] * 3, ["F"] * 3, [1] * 3))
    xyz, inten = dataset.read_pcd(path)
    assert np.array_equal(xyz, np.full((n, 3), 1.5, dtype=np.float32)) and np.array_equal(inten, np.zeros(n, dtype=np.float32))


def test_every_refusal_on_this_branch_names_binary_compressed(tmp_path):
    rec = cloud(20)
    path = str(tmp_path / "r.pcd")
    good = lo.lzf_pack_literals(planes(rec))
    with open(path, "wb") as f:
        f.write(header(20, "binary_compressed") + b"\1\2\3")  # no room for the two size words
    with pytest.raises(ValueError, match="binary_compressed"):
        dataset.read_pcd(path)
    for kw, text in (
        ({"sizes": (len(good), len(planes(rec)) - 1)}, "uncompressed bytes"),  # the announced size is not n x the record
        ({"sizes": (len(good) + 1, len(planes(rec)))}, "compressed bytes announced"),  # the stream is shorter than announced
        ({"stream": good[:-1]}, "ends inside"),  # ... or ends inside a token
        ({"stream": good[: -(len(planes(rec)) % 32 + 1)]}, "decodes to"),  # ... or between two tokens: fewer bytes than announced
        ({"stream": good + b"\0z"}, "overruns"),  # more than announced
        ({"stream": bytes([0x20, 0x00]) + good}, "starts before the output"),
    ):
        write_compressed(path, rec, **kw)
        with pytest.raises(ValueError, match="binary_compressed") as e:
            dataset.read_pcd(path)
        assert text in str(e.value), str(e.value)
    write_compressed(path, rec, head=header(20, "binary_compressed", sizes=[8, 4, 4, 4, 2, 4]))
    with pytest.raises(ValueError, match="F 8"):  # the field rule of the other routes comes first
        dataset.read_pcd(path)
