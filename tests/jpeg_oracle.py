"""numpy restatement of the baseline JPEG decoder (include/nidreg.h: nidreg_jpeg_*): marker parsing, Huffman decoding, dequantisation,
libjpeg's jpeg_idct_islow, libjpeg-turbo's chroma upsampling, libjpeg's YCbCr -> RGB tables and OpenCV's fixed-point luma.  Test
infrastructure: it is written for clarity, shares no code with csrc/, and only decodes streams that are inside the accepted scope
(anything else raises ValueError).  tests/test_jpeg_host.py pins it to Pillow's libjpeg-turbo bit for bit on tests/golden/jpeg_cases.npz.
"""
import struct

import numpy as np

LUMA, BGR = 0, 1

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])  # fmt: skip


class Stream:
    pass


def exif_orientation(payload):
    """Tag 0x0112 of IFD0 in an APP1 payload ("Exif\\0\\0" + TIFF), or None"""
    if payload[:6] != b"Exif\0\0" or len(payload) < 14:
        return None
    t = payload[6:]
    if t[:2] not in (b"II", b"MM"):
        return None
    e = "<" if t[:2] == b"II" else ">"
    if struct.unpack(e + "H", t[2:4])[0] != 42:
        return None
    (ifd,) = struct.unpack(e + "I", t[4:8])
    if ifd + 2 > len(t):
        return None
    (count,) = struct.unpack(e + "H", t[ifd : ifd + 2])
    for i in range(count):
        ent = t[ifd + 2 + 12 * i : ifd + 14 + 12 * i]
        if len(ent) < 12:
            return None
        tag, typ, n = struct.unpack(e + "HHI", ent[:8])
        if tag == 0x0112:
            (v,) = struct.unpack(e + "H", ent[8:10])
            return v if typ == 3 and n == 1 and 1 <= v <= 8 else None
    return None


def parse(data):
    """Headers up to the scan: sizes, sampling, tables (quantisation tables in natural order), the scan's offset"""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    s = Stream()
    s.qt, s.huff, s.dri, s.orientation, s.sof = {}, {}, 0, 1, None
    have_exif = False
    pos = 2
    while True:
        if data[pos] != 0xFF:
            raise ValueError("no marker")
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        (length,) = struct.unpack(">H", data[pos : pos + 2])
        seg = data[pos + 2 : pos + length]
        if length < 2 or len(seg) != length - 2:
            raise ValueError("bad segment")
        pos += length
        if m in (0xC0, 0xC1):
            prec, s.height, s.width, n = struct.unpack(">BHHB", seg[:6])
            if prec != 8 or s.sof is not None:
                raise ValueError("bad frame")
            s.sof = m
            s.comps = [dict(id=seg[6 + 3 * c], h=seg[7 + 3 * c] >> 4, v=seg[7 + 3 * c] & 15, tq=seg[8 + 3 * c]) for c in range(n)]
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8):
            raise ValueError("not a baseline stream")
        elif m == 0xC4:
            o = 0
            while o < len(seg):
                key = (seg[o] >> 4, seg[o] & 15)
                counts = list(seg[o + 1 : o + 17])
                vals = list(seg[o + 17 : o + 17 + sum(counts)])
                o += 17 + sum(counts)
                table, code, k = {}, 0, 0
                for length_ in range(1, 17):
                    for _ in range(counts[length_ - 1]):
                        table[(length_, code)] = vals[k]
                        code, k = code + 1, k + 1
                    code <<= 1
                s.huff[key] = table
        elif m == 0xDB:
            o = 0
            while o < len(seg):
                pq, tq = seg[o] >> 4, seg[o] & 15
                q = np.zeros(64, dtype=np.uint16)
                if pq:
                    q[ZIGZAG] = np.frombuffer(seg[o + 1 : o + 129], dtype=">u2")
                else:
                    q[ZIGZAG] = np.frombuffer(seg[o + 1 : o + 65], dtype=np.uint8)
                s.qt[tq] = q
                o += 129 if pq else 65
        elif m == 0xDD:
            (s.dri,) = struct.unpack(">H", seg)
        elif m == 0xE1 and not have_exif:
            v = exif_orientation(seg)
            if v is not None:
                s.orientation, have_exif = v, True
        elif m == 0xDA:
            if seg[0] != len(s.comps):
                raise ValueError("not one interleaved scan")
            for c, comp in enumerate(s.comps):
                assert seg[1 + 2 * c] == comp["id"]
                comp["td"], comp["ta"] = seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15
            s.scan = pos
            break
    n = len(s.comps)
    if n == 1:
        s.comps[0]["h"] = s.comps[0]["v"] = 1
    elif n != 3 or any((c["h"], c["v"]) != (1, 1) for c in s.comps[1:]) or (s.comps[0]["h"], s.comps[0]["v"]) not in ((1, 1), (2, 1), (2, 2)):
        raise ValueError("sampling outside the scope")
    s.hmax, s.vmax = s.comps[0]["h"], s.comps[0]["v"]
    s.subsampling = 0 if n == 1 else {(1, 1): 1, (2, 1): 2, (2, 2): 3}[(s.hmax, s.vmax)]
    s.mcux, s.mcuy = -(-s.width // (8 * s.hmax)), -(-s.height // (8 * s.vmax))
    for c in s.comps:
        c["bw"], c["bh"] = s.mcux * c["h"], s.mcuy * c["v"]
        c["dw"], c["dh"] = -(-s.width * c["h"] // s.hmax), -(-s.height * c["v"] // s.vmax)
    return s


def _intervals(data, pos):
    """The entropy-coded segment as one bit array per restart interval: stuffing undone, fill bytes dropped"""
    out, cur = [], bytearray()
    while pos < len(data):
        b = data[pos]
        if b != 0xFF:
            cur.append(b)
            pos += 1
            continue
        q = pos + 1
        while q < len(data) and data[q] == 0xFF:
            q += 1
        if q >= len(data):
            break
        if data[q] == 0:
            cur.append(0xFF)
            pos = q + 1
        elif 0xD0 <= data[q] <= 0xD7:
            assert data[q] == 0xD0 + len(out) % 8, "restart markers out of sequence"
            out.append(cur)
            cur = bytearray()
            pos = q + 1
        else:
            break
    out.append(cur)
    return [np.unpackbits(np.frombuffer(bytes(c), dtype=np.uint8)).tolist() for c in out]


class _Bits:
    def __init__(self, bits):
        self.bits, self.pos = bits, 0

    def take(self, n):
        v = 0
        for b in self.bits[self.pos : self.pos + n]:
            v = (v << 1) | b
        if self.pos + n > len(self.bits):
            raise ValueError("entropy data ends early")
        self.pos += n
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.take(1)
            if (length, code) in table:
                return table[(length, code)]
        raise ValueError("no such Huffman code")


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def coefficients(data):
    """``(stream, [blocks (bh, bw, 64) int16 in natural order, one array per component])``: the quantised coefficients"""
    data = bytes(data)
    s = parse(data)
    blocks = [np.zeros((c["bh"], c["bw"], 64), dtype=np.int16) for c in s.comps]
    chunks = _intervals(data, s.scan)
    per = s.dri if s.dri else s.mcux * s.mcuy
    for k in range(s.mcux * s.mcuy):
        if k % per == 0:
            br, pred = _Bits(chunks[k // per]), [0] * len(s.comps)
        my, mx = divmod(k, s.mcux)
        for ci, c in enumerate(s.comps):
            dc, ac = s.huff[(0, c["td"])], s.huff[(1, c["ta"])]
            for by in range(c["v"]):
                for bx in range(c["h"]):
                    blk = blocks[ci][my * c["v"] + by, mx * c["h"] + bx]
                    t = br.symbol(dc)
                    pred[ci] += _extend(br.take(t), t)
                    blk[0] = (pred[ci] + 32768) % 65536 - 32768  # the store reduces to int16, as libjpeg's (JCOEF) cast does
                    i = 1
                    while i < 64:
                        rs = br.symbol(ac)
                        r, sz = rs >> 4, rs & 15
                        if sz == 0:
                            if r != 15:
                                break
                            i += 16
                            continue
                        i += r
                        blk[ZIGZAG[i]] = _extend(br.take(sz), sz)
                        i += 1
    return s, blocks


# ---------------------------------------------------------------------------------------------- arithmetic
def _idct_pass(v):
    """One 8-point pass of jpeg_idct_islow along the LAST axis, before the descale; int32, wrapping"""
    i = [v[..., k] for k in range(8)]
    z2, z3 = i[2], i[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 - z3 * 15137
    tmp3 = z1 + z2 * 6270
    z2, z3 = i[0], i[4]
    tmp0 = (z2 + z3) * 8192
    tmp1 = (z2 - z3) * 8192
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3], axis=-1)


def _descale(v, n):
    return (v + np.int32(1 << (n - 1))) >> n


def idct_blocks(blocks, qt, report=None):
    """(bh, bw, 64) quantised int16 blocks -> the (8 bh, 8 bw) uint8 plane.  ``report``: a dict that receives the extremes of the
    dequantised coefficients and of the column pass's outputs (the int16 domain of libjpeg-turbo's SIMD code)."""
    bh, bw, _ = blocks.shape
    with np.errstate(over="ignore"):
        deq = (blocks.astype(np.int32) * qt.astype(np.int32)).reshape(bh, bw, 8, 8)  # [row, column]
        cols = _descale(_idct_pass(deq.transpose(0, 1, 3, 2)), 11).transpose(0, 1, 3, 2)  # along the rows of each column
        rows = _descale(_idct_pass(cols), 18) + 128
    if report is not None:
        report["deq"] = max(report.get("deq", 0), int(np.abs(deq.astype(np.int64)).max()))
        report["pass1"] = max(report.get("pass1", 0), int(np.abs(cols.astype(np.int64)).max()))
    return np.clip(rows, 0, 255).astype(np.uint8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)  # SATURATE (libjpeg-turbo SIMD)


def _edge(a, axis):
    """a with its first and last entries along ``axis`` repeated once: the replicated neighbours"""
    return np.concatenate([np.take(a, [0], axis), a, np.take(a, [-1], axis)], axis)


def upsample(plane, hs, vs):
    """libjpeg-turbo's upsampling of a downsampled (dh, dw) plane by hs x vs in {1x1, 2x1, 2x2}: the triangle ("fancy") filter when
    dw > 2, plain replication otherwise"""
    a = plane.astype(np.int32)
    dh, dw = a.shape
    if hs == 1:
        return plane.copy()
    if dw <= 2:
        return np.repeat(np.repeat(plane, vs, axis=0), 2, axis=1)
    if vs == 1:
        e = _edge(a, 1)
        out = np.empty((dh, 2 * dw), dtype=np.int32)
        out[:, 0::2] = (3 * a + e[:, :-2] + 1) >> 2
        out[:, 1::2] = (3 * a + e[:, 2:] + 2) >> 2
        return out.astype(np.uint8)
    e = _edge(a, 0)
    col = np.empty((2 * dh, dw), dtype=np.int32)
    col[0::2] = 3 * a + e[:-2]  # even output row: far = the row above
    col[1::2] = 3 * a + e[2:]   # odd: the row below
    e = _edge(col, 1)
    out = np.empty((2 * dh, 2 * dw), dtype=np.int32)
    out[:, 0::2] = (3 * col + e[:, :-2] + 8) >> 4
    out[:, 1::2] = (3 * col + e[:, 2:] + 7) >> 4
    return out.astype(np.uint8)


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def cv_luma(rgb):
    """OpenCV's 8-bit fixed-point BGR2GRAY / RGB2GRAY"""
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)


def decode_planes(data, report=None):
    """``(stream, [component planes, cropped to their downsampled sizes])``"""
    s, blocks = coefficients(data)
    return s, [idct_blocks(b, s.qt[c["tq"]], report)[: c["dh"], : c["dw"]] for b, c in zip(blocks, s.comps)]


def decode_rgb(data):
    s, planes = decode_planes(data)
    if len(planes) == 1:
        return np.repeat(planes[0][:, :, None], 3, axis=2)
    cb, cr = (upsample(p, s.hmax, s.vmax)[: s.height, : s.width] for p in planes[1:])
    return ycc_to_rgb(planes[0], cb, cr)


def decode_gray(data, mode):
    """LUMA: the Y plane (cv::imread(path, 0)); BGR: RGB through the cv luma (cv_bridge to mono8).  No EXIF orientation."""
    s, planes = decode_planes(data)
    if len(planes) == 1 or mode == LUMA:
        return planes[0]
    cb, cr = (upsample(p, s.hmax, s.vmax)[: s.height, : s.width] for p in planes[1:])
    return cv_luma(ycc_to_rgb(planes[0], cb, cr))


def apply_orientation(img, orientation):
    """OpenCV's ExifTransform for orientations 1-8"""
    if orientation == 2:
        return img[:, ::-1]
    if orientation == 3:
        return img[::-1, ::-1]
    if orientation == 4:
        return img[::-1]
    if orientation == 5:
        return img.T
    if orientation == 6:
        return img.T[:, ::-1]
    if orientation == 7:
        return img.T[::-1, ::-1]
    if orientation == 8:
        return img.T[::-1]
    return img


def load_cases(path):
    """tests/golden/jpeg_cases.npz (tests/make_jpeg_golden.py) as ``{name: (stream bytes, Pillow's Y plane, Pillow's RGB through the
    cv luma)}``"""
    with np.load(path) as z:
        out = {}
        for key in z.files:
            if key.endswith(".jpg"):
                name = key[:-4]
                y = np.cumsum(z[name + ".ydx"], axis=1, dtype=np.uint8)
                g = y + z[name + ".gmy"] if name + ".gmy" in z.files else y
                out[name] = (z[key].tobytes(), y, g)
    return out
