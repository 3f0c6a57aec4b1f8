"""The oracle of the survey-map route (tests/test_las_host.py, tests/test_las_gpu.py, tests/test_pcd_compressed.py), written from
the public ASPRS LAS 1.0 - 1.4 specification and the public description of the LZF stream -- independently of
``dataset.read_las_header``, ``csrc/nid_las_kernels.hpp`` and ``csrc/nid_lzf_host.hpp``.  UNPINNED against laspy / PDAL / PCL /
liblzf and real files: none of them is available to the tests.

* ``parse_header``: the public header block through one ``struct`` format per version;
* ``pack_records`` / ``write_las``: any of the 11 point formats from arrays, optional extra bytes; every byte the decoder must not
  look at is filled from the generator;
* ``decode``: the numpy restatement -- ``(X.astype(f8) * s + o) - g`` as three numpy operations, the luma in uint32, the filters
  as boolean masks;
* ``lzf_pack_literals`` and ``LZF_STREAMS``: a literal-run-only LZF packer and hand-assembled streams with back-references.
"""
import struct

import numpy as np

BASE_LENGTH = (20, 28, 26, 34, 57, 63, 30, 36, 38, 59, 67)
RGB_OFFSET = {2: 20, 3: 28, 5: 28, 7: 30, 8: 30, 10: 30}
HEADER_SIZE = {0: 227, 1: 227, 2: 227, 3: 235, 4: 375}

# signature, file source id, global encoding, GUID, major, minor, system id, software, day, year, header size, point offset, VLRs,
# format, record length, legacy count, legacy count by return x 5, scale x 3, offset x 3, max x, min x, max y, min y, max z, min z
_HEAD = "<4sHH16sBB32s32sHHHIIBHI5I3d3d6d"
assert struct.calcsize(_HEAD) == 227
_TAIL_13 = "<Q"  # start of waveform data
_TAIL_14 = "<QQIQ15Q"  # start of waveform data, first EVLR, EVLRs, 64-bit count, count by return x 15
assert 227 + struct.calcsize(_TAIL_14) == 375


def build_header(point_format, record_length, count, scale, offset, mins, maxs, minor=2, vlr_bytes=0, legacy_count=None, count64=None, major=1, signature=b"LASF", format_byte=None):
    """The header bytes of a 1.``minor`` file followed by ``vlr_bytes`` of variable-length-record space before the points"""
    size = HEADER_SIZE[minor]
    legacy = (count if count < 2**32 else 0) if legacy_count is None else legacy_count
    head = struct.pack(_HEAD, signature, 7, 0, bytes(range(16)), major, minor, b"oracle", b"las_oracle.py", 1, 2024, size, size + vlr_bytes, 0,
                       point_format if format_byte is None else format_byte, record_length, legacy, legacy, 0, 0, 0, 0, *scale, *offset, maxs[0], mins[0], maxs[1], mins[1], maxs[2], mins[2])
    if minor == 3:
        head += struct.pack(_TAIL_13, 0)
    if minor == 4:
        head += struct.pack(_TAIL_14, 0, 0, 0, count if count64 is None else count64, *([0] * 15))
    return head + b"\xa5" * vlr_bytes


def parse_header(data):
    """The fields ``dataset.read_las_header`` returns, from the bytes of a file, by ``struct``"""
    f = struct.unpack_from(_HEAD, data, 0)
    major, minor = f[4], f[5]
    out = {"version": (major, minor), "header_size": f[10], "point_offset": f[11], "point_format": f[13], "record_length": f[14], "num_points": f[15], "scale": tuple(f[21:24]),
           "offset": tuple(f[24:27]), "max": (f[27], f[29], f[31]), "min": (f[28], f[30], f[32]), "file_size": len(data)}
    if minor >= 4 and out["header_size"] >= 375:
        count64 = struct.unpack_from(_TAIL_14, data, 227)[3]
        if count64:
            out["num_points"] = count64
    return out


def pack_records(point_format, X, Y, Z, intensity, classification=None, withheld=None, rgb=None, extra=0, rng=None, flags=None):
    """``(n, BASE_LENGTH + extra)`` uint8 records.  ``classification`` 0..31 (formats 0 - 5) or 0..255 (6 - 10); ``withheld`` bool;
    ``flags`` (formats 0 - 5): the synthetic / key-point bits (bits 5, 6 of byte 15) -- random when ``None``; ``rgb`` (n, 3) uint16
    for the formats that carry colour.  All other bytes come from ``rng``: return numbers, scan angle, GPS time, NIR, wave packets
    and the extra bytes are noise the decoder must ignore."""
    rng = np.random.default_rng(0) if rng is None else rng
    n = len(X)
    step = BASE_LENGTH[point_format] + extra
    rec = rng.integers(0, 256, (n, step), dtype=np.uint8)
    for k, v in enumerate((X, Y, Z)):
        rec[:, 4 * k : 4 * k + 4] = np.asarray(v, dtype="<i4").reshape(n, 1).view(np.uint8)
    rec[:, 12:14] = np.asarray(intensity, dtype="<u2").reshape(n, 1).view(np.uint8)
    cls = np.zeros(n, dtype=np.uint8) if classification is None else np.asarray(classification, dtype=np.uint8)
    wh = np.zeros(n, dtype=np.uint8) if withheld is None else np.asarray(withheld, dtype=bool).astype(np.uint8)
    if point_format <= 5:
        assert (cls < 32).all()
        fl = rng.integers(0, 4, n, dtype=np.uint8) if flags is None else np.asarray(flags, dtype=np.uint8)
        rec[:, 15] = cls | (fl << 5) | (wh << 7)
    else:
        rec[:, 15] = (rec[:, 15] & np.uint8(0xFB)) | (wh << 2)
        rec[:, 16] = cls
    if rgb is not None:
        o = RGB_OFFSET[point_format]
        rec[:, o : o + 6] = np.ascontiguousarray(rgb, dtype="<u2").reshape(n, 3).view(np.uint8)
    return rec


def write_las(path, point_format, records, scale, offset, minor=2, vlr_bytes=0, mins=None, maxs=None, **header_kw):
    """A LAS file of ``records`` (``pack_records``); the header bounds are the coordinates' unless given"""
    records = np.ascontiguousarray(records, dtype=np.uint8)
    n, step = records.shape
    if mins is None or maxs is None:
        xyz, _, _ = decode(records, point_format, scale, offset, (0.0, 0.0, 0.0))
        lo = xyz.min(axis=0) if n else np.zeros(3)
        hi = xyz.max(axis=0) if n else np.zeros(3)
        mins = tuple(lo) if mins is None else mins
        maxs = tuple(hi) if maxs is None else maxs
    with open(path, "wb") as f:
        f.write(build_header(point_format, step, n, scale, offset, mins, maxs, minor=minor, vlr_bytes=vlr_bytes, **header_kw))
        f.write(records.tobytes())


def decode(records, point_format, scale, offset, origin, intensity="intensity", exclude_classes=(), keep_withheld=False):
    """``(xyz (n, 3) float64, intensities (n,) float64, keep (n,) bool)`` of ``records`` (n, step) uint8"""
    rec = np.ascontiguousarray(records, dtype=np.uint8)
    n = rec.shape[0]
    xyz = np.empty((n, 3), dtype=np.float64)
    for k in range(3):
        v = np.ascontiguousarray(rec[:, 4 * k : 4 * k + 4]).view("<i4").reshape(n)
        scaled = v.astype(np.float64) * np.float64(scale[k])
        placed = scaled + np.float64(offset[k])
        xyz[:, k] = placed - np.float64(origin[k])
    if intensity == "rgb":
        o = RGB_OFFSET[point_format]
        c = np.ascontiguousarray(rec[:, o : o + 6]).view("<u2").reshape(n, 3).astype(np.uint32)
        inten = (np.uint32(77) * c[:, 0] + np.uint32(150) * c[:, 1] + np.uint32(29) * c[:, 2]).astype(np.float64)
    else:
        inten = np.ascontiguousarray(rec[:, 12:14]).view("<u2").reshape(n).astype(np.float64)
    if point_format <= 5:
        cls = rec[:, 15] & 0x1F
        withheld = (rec[:, 15] & 0x80) != 0
    else:
        cls = rec[:, 16]
        withheld = (rec[:, 15] & 0x04) != 0
    keep = ~np.isin(cls, np.asarray(list(exclude_classes), dtype=np.int64))
    if not keep_withheld:
        keep &= ~withheld
    return xyz, inten, keep


# ------------------------------------------------------------------------------------------------ LZF
def lzf_pack_literals(data):
    """``data`` as an LZF stream of literal runs only: a control byte ``run - 1`` (< 32), then the run's bytes"""
    data = bytes(data)
    out = bytearray()
    for s in range(0, len(data), 32):
        chunk = data[s : s + 32]
        out.append(len(chunk) - 1)
        out += chunk
    return bytes(out)


_RAMP = bytes((i * 7 + (i >> 8)) & 0xFF for i in range(8192))

# name -> (stream, expected output, or None when the stream must be refused)
LZF_STREAMS = {
    # literal "a", then length 5 at distance 1: the copy overlaps its own output and replicates
    "distance_1_overlapping": (bytes([0x00, 0x61, (3 << 5) | 0, 0x00]), b"a" * 6),
    # literal "ab", then the 3-bit length field = 7 and an extension byte 10: length 7 + 10 + 2 = 19 at distance 2
    "length_extension": (bytes([0x01, 0x61, 0x62, (7 << 5) | 0, 10, 0x01]), b"ab" + b"ab" * 9 + b"a"),
    # 8192 literal bytes, then length 3 at the largest distance, ((31 << 8) | 255) + 1 = 8192: the first three bytes again
    "largest_distance": (lzf_pack_literals(_RAMP) + bytes([(1 << 5) | 31, 0xFF]), _RAMP + _RAMP[:3]),
    # a literal between two references, and a reference whose source is an earlier reference's output
    "mixed": (bytes([0x02, 1, 2, 3, (1 << 5) | 0, 2, 0x00, 9, (2 << 5) | 0, 3]), bytes([1, 2, 3, 1, 2, 3, 9, 1, 2, 3, 9])),
    # literal "a", then a reference at distance 2: it starts one byte before the output
    "reference_before_output": (bytes([0x00, 0x61, (1 << 5) | 0, 0x01]), None),
}


if __name__ == "__main__":
    import argparse
    import os

    ap = argparse.ArgumentParser(description="the LZF streams above as files, for tools/lzf_check.cpp")
    ap.add_argument("--dump-lzf", required=True, metavar="DIR")
    out = ap.parse_args().dump_lzf
    os.makedirs(out, exist_ok=True)
    streams = dict((k, v[0]) for k, v in LZF_STREAMS.items())
    streams["literals_1000"] = lzf_pack_literals(_RAMP[:1000])
    for name, stream in streams.items():
        with open(os.path.join(out, name + ".lzf"), "wb") as f:
            f.write(stream)
    print("wrote", len(streams), "streams to", out)
