"""On-disk input/output of the calibration path (SURVEY.md "next" row N3): the preprocessed-directory
format ``preprocess`` writes and ``calibrate`` reads.

======================================  ==============================================================
here                                    reference
======================================  ==============================================================
``VisualLiDARData(data_path, bag)``     ``vlcal::VisualLiDARData`` (src/vlcal/common/visual_lidar_data.cpp:10-27):
                                        ``<bag>.png`` via ``cv::imread(.., 0)`` + ``<bag>.ply`` via ``glk::load_ply``
``read_ply`` / ``write_ply``            ``glk::load_ply`` / ``glk::save_ply_binary`` (Iridescence, not in the tree);
                                        the writer emits what preprocess.cpp:161-169 hands it: float x y z + float intensity
``write_ply_colored``                   no counterpart: float x y z + uchar red green blue, what the headless viewer saves
``read_pcd``                            ``pcl::io::load`` of a PCD map into ``PointXYZI`` (PCL, not in the tree; preprocess_map.cpp:129-131)
``read_png_gray`` / ``write_png_gray``  ``cv::imread(path, 0)`` / ``cv::imwrite`` for 8-bit single-channel PNGs
``write_index_png``                     ``cv::imwrite`` of the CV_8UC4 view of an int32 index image (preprocess.cpp:207-211)
``read_image_gray``                     ``cv::imread(path, 0)`` for a camera photograph (preprocess_map.cpp:69): PNG as above, or a baseline
                                        JPEG -- the Y plane, then the EXIF orientation -- decoded on the GPU (``decode_jpeg_gray``)
``decode_jpeg_gray``                    libjpeg as OpenCV drives it, in the two ways the reference does: ``cv::imread(path, 0)`` (LUMA) and
                                        ``cv_bridge::toCvCopy(msg, "mono8")`` (BGR, preprocess_ros1.cpp:104-134); unpinned against OpenCV itself
``read_calib`` / ``write_calib``        ``calib.json`` (preprocess.cpp:220-232; calibrate.cpp:36-46, 56-65, 128-140)
``init_T_lidar_camera(config)``         calibrate.cpp:56-77 (manual guess first, then the automatic one)
======================================  ==============================================================

Pure host code (numpy + zlib + json) except the JPEG decoder, whose arithmetic runs on the GPU (``nidreg_jpeg_decode_gray``); nothing
here is on the per-evaluation path.
"""
import functools
import json
import os
import struct
import zlib

import numpy as np

from . import se3

# --------------------------------------------------------------------------------------------- PLY
_PLY_TYPES = {
    "char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4",
    "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8",
}


def _parse_ply_header(data, path):
    """``(format, elements, body offset)`` of a PLY file whose first bytes (the whole header at least) are ``data``;
    elements = [(name, count, [(prop name, dtype code) | None for lists])]."""
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    nl = data.find(b"\n", end)
    if nl < 0:
        raise ValueError(f"{path}: truncated PLY header")
    header = data[:end].decode("ascii", "replace").splitlines()
    body = nl + 1
    fmt = None
    elements = []  # (name, count, [(prop name, dtype code) | None for lists])
    for line in header[1:]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise ValueError(f"{path}: property before any element")
            if tok[1] == "list":
                elements[-1][2].append(None)
            else:
                if tok[1] not in _PLY_TYPES:
                    raise ValueError(f"{path}: unknown PLY type {tok[1]}")
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise ValueError(f"{path}: unsupported PLY format {fmt}")
    return fmt, elements, body


_INTENSITY_NAMES = ("intensity", "scalar_intensity", "intensities")


def read_ply(path):
    """Vertex positions and intensities of a PLY file.  Returns ``(points (n, 4) float64 homogeneous,
    intensities (n,) float64 or None)`` -- ``FrameCPU(ply->vertices)`` + ``add_intensities``
    (visual_lidar_data.cpp:25-26).  ascii, binary_little_endian and binary_big_endian are accepted;
    only the vertex element is read."""
    with open(path, "rb") as f:
        data = f.read()
    fmt, elements, body = _parse_ply_header(data, path)
    offset = body
    for name, count, props in elements:
        if name == "vertex":
            if any(p is None for p in props):
                raise ValueError(f"{path}: list property in the vertex element")
            names = [p[0] for p in props]
            if fmt == "ascii":
                text = data[offset:].split(b"\n", count)[:count]
                arr = np.array([ln.split() for ln in text], dtype=np.float64).reshape(count, len(props))
                cols = {n: arr[:, i] for i, n in enumerate(names)}
            else:
                order = "<" if fmt == "binary_little_endian" else ">"
                dt = np.dtype([(n, order + c) for n, c in props])
                if offset + count * dt.itemsize > len(data):
                    raise ValueError(f"{path}: truncated PLY vertex data")
                rec = np.frombuffer(data, dtype=dt, count=count, offset=offset)
                cols = {n: rec[n] for n in names}
            for k in ("x", "y", "z"):
                if k not in cols:
                    raise ValueError(f"{path}: vertex element has no '{k}' property")
            pts = np.ones((count, 4), dtype=np.float64)
            pts[:, 0], pts[:, 1], pts[:, 2] = cols["x"], cols["y"], cols["z"]
            inten = None
            for k in _INTENSITY_NAMES:
                if k in cols:
                    inten = np.ascontiguousarray(cols[k], dtype=np.float64)
                    break
            return pts, inten
        # skip an element stored before the vertices
        if fmt == "ascii":
            for _ in range(count):
                offset = data.index(b"\n", offset) + 1
        else:
            if any(p is None for p in props):
                raise ValueError(f"{path}: list element '{name}' precedes the vertices")
            offset += count * sum(np.dtype(c).itemsize for _, c in props)
    raise ValueError(f"{path}: no vertex element")


def read_ply_float32(path):
    """The cloud as ``preprocess`` stores it (preprocess.cpp:161-169), without a widening pass: ``(xyz (n, 3), intensities (n,))``,
    float32 views over ONE read of the file's vertex block (rows strided by the record size; both alias the same buffer), for
    ``nid.Cloud.from_float32``.  ``None`` -- use ``read_ply`` -- unless the file is binary_little_endian and its vertex element has
    float ``x y z`` (consecutive) and a float intensity property (the one ``read_ply`` picks) at 4-byte aligned offsets.
    Widened, the views equal ``read_ply``'s arrays bit for bit."""
    with open(path, "rb") as f:
        head = f.read(1 << 16)
        while b"end_header" not in head or head.find(b"\n", head.find(b"end_header")) < 0:
            more = f.read(1 << 16)
            if not more:
                break
            head += more
        size = f.seek(0, os.SEEK_END)
    fmt, elements, offset = _parse_ply_header(head, path)
    if fmt != "binary_little_endian":
        return None
    for name, count, props in elements:
        if any(p is None for p in props):
            return None
        if name != "vertex":
            offset += count * sum(np.dtype(c).itemsize for _, c in props)  # an element stored before the vertices
            continue
        dt = np.dtype([(n, "<" + c) for n, c in props])
        key = next((k for k in _INTENSITY_NAMES if k in dt.names), None)
        if key is None or any(k not in dt.names or dt[k] != np.dtype("<f4") for k in ("x", "y", "z", key)):
            return None
        ox, oi = dt.fields["x"][1], dt.fields[key][1]
        if dt.fields["y"][1] != ox + 4 or dt.fields["z"][1] != ox + 8 or dt.itemsize % 4 or ox % 4 or oi % 4:
            return None
        if offset + count * dt.itemsize > size:
            return None  # (read_ply says: truncated)
        if count == 0:
            return np.zeros((0, 3), dtype=np.float32), np.zeros(0, dtype=np.float32)
        raw = np.fromfile(path, dtype=np.uint8, count=count * dt.itemsize, offset=offset)  # not a memmap: no page faults inside the upload
        xyz = np.ndarray((count, 3), dtype="<f4", buffer=raw, offset=ox, strides=(dt.itemsize, 4))
        inten = np.ndarray((count,), dtype="<f4", buffer=raw, offset=oi, strides=(dt.itemsize,))
        return xyz, inten
    return None


def write_ply(path, points, intensities):
    """binary_little_endian PLY with float x y z + float intensity per vertex: the record
    preprocess.cpp:161-169 fills (``p.cast<float>().head<3>()`` and the intensity narrowed to float)."""
    pts = np.asarray(points)
    n = pts.shape[0]
    rec = np.empty(n, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")])
    rec["x"], rec["y"], rec["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    rec["intensity"] = np.asarray(intensities)
    header = f"ply\nformat binary_little_endian 1.0\nelement vertex {n}\nproperty float x\nproperty float y\nproperty float z\nproperty float intensity\nend_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())


def write_ply_colored(path, points, rgb8):
    """binary_little_endian PLY with float x y z + uchar red green blue per vertex (the headless viewer's ``--save_ply``); any PLY
    viewer shows it.  ``read_ply`` reads its positions back."""
    pts = np.asarray(points)
    rgb = np.asarray(rgb8, dtype=np.uint8).reshape(-1, 3)
    n = pts.shape[0]
    if rgb.shape[0] != n:
        raise ValueError("write_ply_colored: one RGB colour per point expected")
    rec = np.empty(n, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    rec["x"], rec["y"], rec["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {n}\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())


# --------------------------------------------------------------------------------------------- PCD
def read_pcd(path):
    """The x y z (and, if present, intensity) fields of a PCD file, ``DATA ascii`` or ``DATA binary`` -- what
    ``pcl::io::load`` into a ``PointXYZI`` cloud keeps (preprocess_map.cpp:129-131).  Returns what ``read_ply_float32`` returns:
    ``(xyz (n, 3), intensities (n,))`` float32 (views over one buffer for binary files; zeros where the file has no intensity
    field).  The four fields must be ``F 4``; other fields are skipped by their SIZE x COUNT.  ``DATA binary_compressed`` (one LZF
    stream of per-field planes, ``_pcd_compressed_columns``) is read too.  Other data formats and field types are refused with a
    ValueError that names what was found."""
    with open(path, "rb") as f:
        data = f.read()
    head = {}
    pos = 0
    while "DATA" not in head:
        nl = data.find(b"\n", pos)
        if nl < 0:
            raise ValueError(f"{path}: not a PCD file (no DATA line)")
        tok = data[pos:nl].decode("ascii", "replace").split()
        pos = nl + 1
        if tok and not tok[0].startswith("#"):
            head[tok[0].upper()] = tok[1:]
    fields = head.get("FIELDS") or head.get("COLUMNS")
    if not fields or "SIZE" not in head or "TYPE" not in head:
        raise ValueError(f"{path}: PCD header without FIELDS / SIZE / TYPE")
    sizes = [int(v) for v in head["SIZE"]]
    types = [v.upper() for v in head["TYPE"]]
    counts = [int(v) for v in head.get("COUNT", ["1"] * len(fields))]
    if not (len(sizes) == len(types) == len(counts) == len(fields)):
        raise ValueError(f"{path}: PCD header lists {len(fields)} fields but {len(sizes)} sizes, {len(types)} types, {len(counts)} counts")
    if "POINTS" in head:
        n = int(head["POINTS"][0])
    elif "WIDTH" in head and "HEIGHT" in head:
        n = int(head["WIDTH"][0]) * int(head["HEIGHT"][0])
    else:
        raise ValueError(f"{path}: PCD header without POINTS or WIDTH / HEIGHT")
    fmt = head["DATA"][0].lower() if head["DATA"] else ""
    if fmt not in ("ascii", "binary", "binary_compressed"):
        raise ValueError(f"{path}: unsupported PCD data format '{fmt}' (ascii, binary and binary_compressed are read)")
    wanted = [k for k in ("x", "y", "z", "intensity") if k in fields]
    for k in ("x", "y", "z"):
        if k not in fields:
            raise ValueError(f"{path}: PCD file has no '{k}' field")
    for k in wanted:
        i = fields.index(k)
        if (types[i], sizes[i], counts[i]) != ("F", 4, 1):
            raise ValueError(f"{path}: field '{k}' is {types[i]} {sizes[i]} x {counts[i]}; only F 4 x 1 is read")
    if fmt == "binary":
        dt = np.dtype({"names": [f"f{i}" for i in range(len(fields))], "formats": [("<f4" if fields[i] in wanted else f"V{sizes[i] * counts[i]}") for i in range(len(fields))]})
        if pos + n * dt.itemsize > len(data):
            raise ValueError(f"{path}: truncated PCD point data")
        rec = np.frombuffer(data, dtype=dt, count=n, offset=pos)
        cols = {k: rec[f"f{fields.index(k)}"] for k in wanted}
    elif fmt == "binary_compressed":
        cols = _pcd_compressed_columns(path, data, pos, n, fields, sizes, counts, wanted)
    else:
        first = np.concatenate([[0], np.cumsum(counts)])  # first token of every field
        rows = [ln.split() for ln in data[pos:].decode("ascii", "replace").splitlines() if ln.strip()][:n]
        if len(rows) < n:
            raise ValueError(f"{path}: truncated PCD point data")
        cols = {k: np.array([r[first[fields.index(k)]] for r in rows], dtype=np.float64).astype(np.float32) for k in wanted}
    xyz = np.empty((n, 3), dtype=np.float32)
    xyz[:, 0], xyz[:, 1], xyz[:, 2] = cols["x"], cols["y"], cols["z"]
    inten = np.ascontiguousarray(cols["intensity"]) if "intensity" in cols else np.zeros(n, dtype=np.float32)
    return xyz, inten


def lzf_decompress(stream, out_size):
    """``nidreg_lzf_decompress`` (host only, csrc/nid_lzf_host.hpp): the LZF stream ``stream`` into at most ``out_size`` bytes, as a
    uint8 array of the bytes produced.  ``ValueError`` with the input offset for a stream that ends inside a token, refers to before
    the output or overruns ``out_size``."""
    import ctypes

    from . import _lib

    lib = _lib.load()
    src = np.frombuffer(bytes(stream), dtype=np.uint8)
    out = np.empty(max(int(out_size), 1), dtype=np.uint8)
    written = ctypes.c_int64()
    rc = lib.nidreg_lzf_decompress(src.ctypes.data if src.size else None, src.size, out.ctypes.data, int(out_size), ctypes.byref(written))
    if rc == _lib.NIDREG_ERR_INVALID:
        raise ValueError(_lib.last_error())
    _lib.check(rc, "nidreg_lzf_decompress")
    return out[: int(written.value)]


def _pcd_compressed_columns(path, data, pos, n, fields, sizes, counts, wanted):
    """The wanted columns of a ``DATA binary_compressed`` body: a u32 compressed size, a u32 uncompressed size, then one LZF stream
    whose output is one plane per field in header order, ``n x SIZE x COUNT`` bytes each (what
    ``pcl::io::savePCDFileBinaryCompressed`` writes).  Unpinned against PCL / liblzf and real files."""
    if pos + 8 > len(data):
        raise ValueError(f"{path}: truncated PCD point data (binary_compressed: no size words)")
    comp, uncomp = struct.unpack_from("<II", data, pos)
    widths = [s * c for s, c in zip(sizes, counts)]
    if uncomp != n * sum(widths):
        raise ValueError(f"{path}: binary_compressed body says {uncomp} uncompressed bytes; {n} points of {sum(widths)} bytes are {n * sum(widths)}")
    if pos + 8 + comp > len(data):
        raise ValueError(f"{path}: truncated PCD point data (binary_compressed: {comp} compressed bytes announced, {len(data) - pos - 8} present)")
    try:
        plain = lzf_decompress(data[pos + 8 : pos + 8 + comp], uncomp)
    except ValueError as e:
        raise ValueError(f"{path}: binary_compressed body does not decode: {e}") from None
    if plain.size != uncomp:
        raise ValueError(f"{path}: binary_compressed body decodes to {plain.size} bytes, {uncomp} announced")
    starts = np.concatenate([[0], np.cumsum(widths)]) * n
    return {k: np.array(plain[starts[fields.index(k)] : starts[fields.index(k)] + 4 * n].view("<f4")) for k in wanted}  # (copies: a plane may start off a 4-byte boundary)


# --------------------------------------------------------------------------------------------- LAS
LAS_BASE_LENGTH = (20, 28, 26, 34, 57, 63, 30, 36, 38, 59, 67)  # point formats 0..10
LAS_RGB_OFFSET = {2: 20, 3: 28, 5: 28, 7: 30, 8: 30, 10: 30}  # byte of the u16 red channel; the other formats have no colour


def read_las_header(path):
    """The public header block of an ASPRS LAS 1.0 - 1.4 file, little-endian, as a dict: ``version`` (major, minor),
    ``header_size``, ``point_offset``, ``point_format``, ``record_length``, ``num_points`` (the 64-bit count of a 1.4 header when it
    is non-zero, else the legacy count), ``scale`` / ``offset`` / ``min`` / ``max`` (three floats each) and ``file_size``.  Read
    from the public format description; unpinned against laspy / PDAL and real files.  ``ValueError`` that names what was found for
    a wrong signature, a version other than 1.0 - 1.4, a compressed file (LAZ), a point format above 10, a record shorter than its
    format, a zero or non-finite scale, a non-finite offset, a header or point offset past the file and a truncated point block."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(375)
    if len(head) < 4 or head[:4] != b"LASF":
        raise ValueError(f"{path}: not a LAS file (signature {head[:4]!r}, 'LASF' expected)")
    if len(head) < 227:
        raise ValueError(f"{path}: truncated LAS header ({len(head)} bytes; the public header block is at least 227)")
    major, minor = head[24], head[25]
    if major != 1 or minor > 4:
        raise ValueError(f"{path}: LAS version {major}.{minor}; 1.0 to 1.4 are read")
    header_size, point_offset = struct.unpack_from("<HI", head, 94)
    fmt_byte, record_length, legacy_count = struct.unpack_from("<BHI", head, 104)
    if fmt_byte & 0xC0:
        raise ValueError(f"{path}: compressed LAS (LAZ) is not read (point format byte {fmt_byte:#04x})")
    if fmt_byte > 10:
        raise ValueError(f"{path}: LAS point format {fmt_byte}; formats 0 to 10 are read")
    if record_length < LAS_BASE_LENGTH[fmt_byte]:
        raise ValueError(f"{path}: LAS record length {record_length} is below the {LAS_BASE_LENGTH[fmt_byte]} bytes of point format {fmt_byte}")
    scale = struct.unpack_from("<3d", head, 131)
    offset = struct.unpack_from("<3d", head, 155)
    bounds = struct.unpack_from("<6d", head, 179)  # max x, min x, max y, min y, max z, min z
    if any(not np.isfinite(s) or s == 0.0 for s in scale):
        raise ValueError(f"{path}: LAS scale {scale} has a zero or non-finite factor")
    if any(not np.isfinite(o) for o in offset):
        raise ValueError(f"{path}: LAS offset {offset} is not finite")
    if header_size < 227 or header_size > size:
        raise ValueError(f"{path}: LAS header size {header_size} lies outside the file ({size} bytes; at least 227)")
    if point_offset < header_size or point_offset > size:
        raise ValueError(f"{path}: LAS offset to point data {point_offset} lies outside the file ({size} bytes, header {header_size})")
    count = legacy_count
    if minor >= 4 and header_size >= 375 and len(head) >= 255:
        count64 = struct.unpack_from("<Q", head, 247)[0]
        if count64:
            count = count64
    if point_offset + count * record_length > size:
        raise ValueError(f"{path}: truncated LAS point data ({count} records of {record_length} bytes from offset {point_offset} need {point_offset + count * record_length} bytes, the file has {size})")
    return {"version": (int(major), int(minor)), "header_size": int(header_size), "point_offset": int(point_offset), "point_format": int(fmt_byte), "record_length": int(record_length),
            "num_points": int(count), "scale": tuple(scale), "offset": tuple(offset), "min": (bounds[1], bounds[3], bounds[5]), "max": (bounds[0], bounds[2], bounds[4]), "file_size": int(size)}


def read_las_chunks(path, header, chunk_points=1 << 23):
    """The point records of a LAS file as ``(chunk_points x record_length,)`` uint8 arrays, one ``np.fromfile`` per chunk (not a
    memmap: no page faults inside the upload): host memory is one chunk, whatever the file size."""
    if chunk_points < 1:
        raise ValueError("read_las_chunks: chunk_points must be positive")
    step, n = header["record_length"], header["num_points"]
    for first in range(0, n, int(chunk_points)):
        m = min(int(chunk_points), n - first)
        raw = np.fromfile(path, dtype=np.uint8, count=m * step, offset=header["point_offset"] + first * step)
        if raw.size != m * step:
            raise ValueError(f"{path}: truncated LAS point data (records {first}..{first + m})")
        yield raw


# --------------------------------------------------------------------------------------------- PNG
_PNG_SIG = b"\x89PNG\r\n\x1a\n"
PNG_SIGNATURE = _PNG_SIG
_PNG_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def _unfilter(raw, height, stride, bpp):
    """Undo the per-scanline PNG filters.  None / Sub / Up rows are vectorised (Sub is a wrapping
    prefix sum per byte lane); Average / Paeth rows fall back to a scalar loop."""
    out = np.empty((height, stride), dtype=np.uint8)
    prev = np.zeros(stride, dtype=np.uint8)
    pos = 0
    for y in range(height):
        ft = raw[pos]
        line = np.frombuffer(raw, dtype=np.uint8, count=stride, offset=pos + 1)
        pos += stride + 1
        if ft == 0:
            cur = line.copy()
        elif ft == 1:
            cur = np.empty(stride, dtype=np.uint8)
            for c in range(bpp):
                cur[c::bpp] = np.add.accumulate(line[c::bpp], dtype=np.uint8)
        elif ft == 2:
            cur = line + prev  # uint8 wraps
        elif ft in (3, 4):
            cur = np.zeros(stride, dtype=np.int64)
            ln = line.astype(np.int64)
            up = prev.astype(np.int64)
            for x in range(stride):
                a = cur[x - bpp] if x >= bpp else 0
                b = up[x]
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    c = up[x - bpp] if x >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[x] = (ln[x] + pred) & 255
            cur = cur.astype(np.uint8)
        else:
            raise ValueError(f"PNG: bad filter type {ft}")
        out[y] = cur
        prev = cur
    return out


def read_png(path):
    """Decode a non-interlaced PNG (gray 1/2/4/8/16 bit, palette 1/2/4/8 bit, gray+alpha / RGB / RGBA 8/16 bit).
    Returns ``(array (H, W) or (H, W, C), bit_depth)`` with the file's own channel order (RGB)."""
    with open(path, "rb") as f:
        data = f.read()
    return decode_png(data, path)


def decode_png(data, path="PNG data"):
    """``read_png`` of the file's bytes (a ``sensor_msgs/CompressedImage`` payload); ``path`` names them in error messages"""
    if data[:8] != _PNG_SIG:
        raise ValueError(f"{path}: not a PNG file")
    pos = 8
    ihdr = None
    idat = []
    palette = None
    while pos + 8 <= len(data):
        (length,) = struct.unpack(">I", data[pos : pos + 4])
        ctype = data[pos + 4 : pos + 8]
        chunk = data[pos + 8 : pos + 8 + length]
        pos += 12 + length
        if ctype == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", chunk)
        elif ctype == b"PLTE":
            palette = np.frombuffer(chunk, dtype=np.uint8).reshape(-1, 3)
        elif ctype == b"IDAT":
            idat.append(chunk)
        elif ctype == b"IEND":
            break
    if ihdr is None or not idat:
        raise ValueError(f"{path}: PNG without IHDR / IDAT")
    width, height, depth, color, _comp, _filt, interlace = ihdr
    if interlace != 0:
        raise ValueError(f"{path}: interlaced PNGs are not supported")
    sub_byte = depth in (1, 2, 4) and color in (0, 3)
    if color not in _PNG_CHANNELS or not (depth in (8, 16) or sub_byte) or (color == 3 and depth == 16):
        raise ValueError(f"{path}: unsupported PNG colour type {color} / bit depth {depth}")
    ch = _PNG_CHANNELS[color]
    bpp = max(1, ch * depth // 8)
    stride = (width * ch * depth + 7) // 8
    raw = zlib.decompress(b"".join(idat))
    if len(raw) < height * (stride + 1):
        raise ValueError(f"{path}: truncated PNG image data")
    rows = _unfilter(raw, height, stride, bpp)
    if depth == 16:
        img = rows.reshape(height, width * ch, 2)
        img = (img[:, :, 0].astype(np.uint16) << 8) | img[:, :, 1]
    elif sub_byte:
        # packed samples, most significant bits first; gray is expanded to 8 bits by replication
        # (png_set_expand_gray_1_2_4_to_8, what cv::imread does), palette indices stay indices
        bits = np.unpackbits(rows, axis=1)[:, : width * depth].reshape(height, width, depth)
        img = np.zeros((height, width), dtype=np.uint8)
        for k in range(depth):
            img = (img << 1) | bits[:, :, k]
        if color == 0:
            img = (img.astype(np.uint16) * (255 // ((1 << depth) - 1))).astype(np.uint8)
        depth = 8
    else:
        img = rows
    img = img.reshape(height, width, ch) if ch > 1 else img.reshape(height, width)
    if color == 3:
        if palette is None:
            raise ValueError(f"{path}: palette PNG without PLTE")
        img = palette[img]
    return img, depth


def read_png_gray(path):
    """``cv::imread(path, 0)``: an 8-bit single-channel image.  16-bit samples keep their high byte;
    colour images are converted with OpenCV's fixed-point BGR2GRAY weights (R 4899, G 9617, B 1868, >> 14).
    Preprocessed directories only contain 8-bit gray PNGs, for which this is the identity."""
    return _png_to_gray(*read_png(path))


def decode_png_gray(data, path="PNG data"):
    """``cv::imdecode(data, 0)``: ``read_png_gray`` of the file's bytes"""
    return _png_to_gray(*decode_png(data, path))


def _png_to_gray(img, depth):
    if depth == 16:
        img = (img >> 8).astype(np.uint8)
    if img.ndim == 3:
        if img.shape[2] == 2:  # gray + alpha
            img = img[:, :, 0]
        else:
            r, g, b = (img[:, :, k].astype(np.int64) for k in range(3))
            img = ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)
    return np.ascontiguousarray(img, dtype=np.uint8)


def _png_chunk(ctype, payload):
    return struct.pack(">I", len(payload)) + ctype + payload + struct.pack(">I", zlib.crc32(ctype + payload) & 0xFFFFFFFF)


def write_png(path, image):
    """8-bit PNG, non-interlaced: (H, W) gray or (H, W, 4) RGBA (the ``_lidar_indices.png`` layout:
    the int32 index image reinterpreted as 4 bytes per pixel, preprocess.cpp:207-211).  Sub filter on
    every row, like OpenCV's encoder."""
    img = np.ascontiguousarray(image, dtype=np.uint8)
    if img.ndim == 2:
        color, ch = 0, 1
    elif img.ndim == 3 and img.shape[2] == 4:
        color, ch = 6, 4
    elif img.ndim == 3 and img.shape[2] == 3:
        color, ch = 2, 3
    else:
        raise ValueError("write_png: (H, W), (H, W, 3) or (H, W, 4) uint8 expected")
    h, w = img.shape[:2]
    flat = img.reshape(h, w * ch)
    filt = flat.copy()
    filt[:, ch:] = flat[:, ch:] - flat[:, :-ch]  # Sub: wraps modulo 256
    raw = np.empty((h, w * ch + 1), dtype=np.uint8)
    raw[:, 0] = 1
    raw[:, 1:] = filt
    with open(path, "wb") as f:
        f.write(_PNG_SIG)
        f.write(_png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, color, 0, 0, 0)))
        f.write(_png_chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)))
        f.write(_png_chunk(b"IEND", b""))


def write_index_png(path, index):
    """An int32 (H, W) index image in the ``_lidar_indices.png`` layout (preprocess.cpp:207-211), which ``pose.read_index_image``
    reads back: the little-endian words as 4 bytes per pixel; cv::imwrite takes the CV_8UC4 buffer as BGRA and the PNG stores RGBA,
    so bytes 0 and 2 swap."""
    idx = np.asarray(index)
    idx4 = np.ascontiguousarray(idx, dtype="<i4").view(np.uint8).reshape(idx.shape[0], idx.shape[1], 4)
    write_png(path, idx4[:, :, [2, 1, 0, 3]])


def write_png_gray(path, image):
    img = np.asarray(image)
    if img.ndim != 2:
        raise ValueError("write_png_gray: single-channel image expected")
    write_png(path, img)


# --------------------------------------------------------------------------------------------- JPEG
JPEG_GRAY_LUMA, JPEG_GRAY_BGR = 0, 1  # NIDREG_JPEG_GRAY_*
_JPEG_REFUSAL = "JPEG images are not decoded here"


def _jpeg_refusal(path, message):
    """``error: failed to load image <where>: JPEG images are not decoded here unless ... (<reason>)`` from the library's error text"""
    at = message.find(_JPEG_REFUSAL)
    return ValueError(f"error: failed to load image {path}: {message[at:] if at >= 0 else message}")


def jpeg_info(data, path="JPEG data"):
    """``nidreg_jpeg_info`` (host only): ``(width, height, components, subsampling, exif_orientation)``; a stream outside the
    decoder's scope raises ``ValueError`` with the reason"""
    import ctypes

    from . import _lib

    lib = _lib.load()
    data = bytes(data)
    out = [ctypes.c_int32() for _ in range(5)]
    rc = lib.nidreg_jpeg_info(data, len(data), *[ctypes.byref(v) for v in out])
    if rc == _lib.NIDREG_ERR_INVALID:
        raise _jpeg_refusal(path, _lib.last_error())
    _lib.check(rc, "nidreg_jpeg_info")
    return tuple(int(v.value) for v in out)


def decode_jpeg_gray(data, mode, device=0, path="JPEG data"):
    """A baseline JPEG stream as an (H, W) uint8 gray image, decoded on the GPU (``nidreg_jpeg_decode_gray``; the entropy decode
    runs on the host first).  ``mode``: ``JPEG_GRAY_LUMA`` is ``cv::imread(path, 0)`` -- the Y plane --, ``JPEG_GRAY_BGR`` is
    ``cv_bridge::toCvCopy(msg, "mono8")`` -- decode to BGR, then OpenCV's fixed-point luma; the two differ for colour streams.
    No EXIF orientation is applied (``read_image_gray`` does that).  A stream outside the decoder's scope raises ``ValueError``
    that names the reason; ``path`` names the bytes in it."""
    import ctypes

    from . import _lib

    data = bytes(data)
    width, height = jpeg_info(data, path)[:2]
    out = np.empty((height, width), dtype=np.uint8)
    lib = _lib.load()
    rc = lib.nidreg_jpeg_decode_gray(int(device), data, len(data), int(mode), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), width)
    if rc == _lib.NIDREG_ERR_INVALID and _JPEG_REFUSAL in _lib.last_error():
        raise _jpeg_refusal(path, _lib.last_error())
    _lib.check(rc, "nidreg_jpeg_decode_gray")
    return out


def apply_exif_orientation(image, orientation):
    """What ``cv::imread`` does with EXIF orientations 2-8 (OpenCV's ExifTransform): flips and transposes"""
    if orientation == 2:
        image = image[:, ::-1]
    elif orientation == 3:
        image = image[::-1, ::-1]
    elif orientation == 4:
        image = image[::-1]
    elif orientation == 5:
        image = image.T
    elif orientation == 6:
        image = image.T[:, ::-1]
    elif orientation == 7:
        image = image.T[::-1, ::-1]
    elif orientation == 8:
        image = image.T[::-1]
    return np.ascontiguousarray(image)


def read_image_gray(path, device=0):
    """``cv::imread(path, 0)`` for the formats decoded here.  A PNG goes through ``read_png_gray``, unchanged.  A JPEG (by its SOI
    marker or its file name) is decoded in LUMA mode and then turned as its EXIF orientation says: ``cv::imread`` honours the tag
    unless ``IMREAD_UNCHANGED`` is passed."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != _PNG_SIG and (data[:2] == b"\xff\xd8" or path.lower().endswith((".jpg", ".jpeg"))):
        orientation = jpeg_info(data, path)[4]
        return apply_exif_orientation(decode_jpeg_gray(data, JPEG_GRAY_LUMA, device=device, path=path), orientation)
    return read_png_gray(path)


# --------------------------------------------------------------------------------------------- calib.json
def read_calib(data_path):
    """``calib.json`` of a preprocessed directory.  Raises like the reference aborts (calibrate.cpp:30-34)."""
    path = os.path.join(data_path, "calib.json")
    if not os.path.exists(path):
        raise FileNotFoundError(f"error: failed to open {path}")
    with open(path) as f:
        return json.load(f)


def write_calib(data_path, config):
    """``ofs << config.dump(2)`` (nlohmann::json keeps object keys sorted)."""
    with open(os.path.join(data_path, "calib.json"), "w") as f:
        json.dump(config, f, indent=2, sort_keys=True)
        f.write("\n")


def camera_from_calib(config):
    """(camera_model, intrinsics, distortion_coeffs) -- calibrate.cpp:38-41"""
    cam = config["camera"]
    return cam["camera_model"], [float(v) for v in cam["intrinsics"]], [float(v) for v in cam["distortion_coeffs"]]


def init_T_lidar_camera(config):
    """The initial guess as TUM values [tx ty tz qx qy qz qw]: the manual one if present, else the
    automatic one, else ``None`` (the reference aborts, calibrate.cpp:56-71)."""
    res = config.get("results", {})
    for key in ("init_T_lidar_camera", "init_T_lidar_camera_auto"):
        if key in res:
            return [float(v) for v in res[key]], key
    return None, None


def tum_to_T_camera_lidar(values):
    """calibrate.cpp:73-77: T_lidar_camera from [tx ty tz qx qy qz qw] (quaternion normalised), inverted.
    Returns Sophus-order parameters [qx qy qz qw tx ty tz] of T_camera_lidar."""
    v = np.asarray(values, dtype=np.float64)
    q = v[3:7] / np.linalg.norm(v[3:7])
    T_lidar_camera = np.concatenate([q, v[0:3]])
    return se3.inverse(T_lidar_camera)


def T_camera_lidar_to_tum(x):
    """calibrate.cpp:128-133: [tx ty tz qx qy qz qw] of T_lidar_camera = inverse(T_camera_lidar)."""
    inv = se3.inverse(np.asarray(x, dtype=np.float64))
    return [float(inv[4]), float(inv[5]), float(inv[6]), float(inv[0]), float(inv[1]), float(inv[2]), float(inv[3])]


class VisualLiDARData:
    """``vlcal::VisualLiDARData``: one bag's image (8-bit gray) and cloud (points (n,4), intensities).

    A cloud stored as float32 records (what ``preprocess`` writes) is kept as read: ``xyz_f32`` / ``intensities_f32``
    (``read_ply_float32``), uploaded as such by ``calibrate``; ``points`` / ``intensities`` are then widened on first use (and
    cached), with the values ``read_ply`` gives.  Any other file loads eagerly (``xyz_f32`` is ``None``)."""

    def __init__(self, data_path, bag_name):
        png = os.path.join(data_path, bag_name + ".png")
        ply = os.path.join(data_path, bag_name + ".ply")
        if not os.path.exists(png):
            raise FileNotFoundError(f"warning: failed to load {png}")
        if not os.path.exists(ply):
            raise FileNotFoundError(f"warning: failed to load {ply}")
        self.bag_name = bag_name
        self.image = read_png_gray(png)
        f32 = read_ply_float32(ply)
        if f32 is not None:
            self.xyz_f32, self.intensities_f32 = f32
        else:
            self.xyz_f32 = self.intensities_f32 = None
            self.points, self.intensities = read_ply(ply)
            if self.intensities is None:
                raise ValueError(f"{ply}: no intensity property")
        self.num_points = int(self.xyz_f32.shape[0] if f32 is not None else self.points.shape[0])

    # float32 bags only (an eagerly loaded bag has these as plain attributes, which take precedence)
    @functools.cached_property
    def points(self):
        pts = np.ones((self.num_points, 4), dtype=np.float64)
        pts[:, :3] = self.xyz_f32
        return pts

    @functools.cached_property
    def intensities(self):
        return np.ascontiguousarray(self.intensities_f32, dtype=np.float64)


def load_dataset(data_path, first_n_bags=None):
    """calibrate.cpp:36-52: ``(config, [VisualLiDARData, ...])``"""
    config = read_calib(data_path)
    names = list(config["meta"]["bag_names"])
    if first_n_bags is not None:
        names = names[: int(first_n_bags)]
    return config, [VisualLiDARData(data_path, n) for n in names]


def load_mask(data_path, bag_name, spec, image_shape, log=None):
    """The image mask of one bag for ``--mask``: (H, W) uint8, non-zero = use, zero = ignore -- or ``None`` (the bag is used whole).
    ``spec`` is ``None`` (no mask), a PNG path (one mask for every bag) or ``auto``: ``<data_path>/<bag>_mask.png`` if it exists,
    else ``<data_path>/mask.png``, else none, which is logged.  Files are read with ``read_png_gray``.  A named file that does not
    exist, and a mask whose size is not ``image_shape`` (H, W), are refused with a ValueError / FileNotFoundError that names the
    file: host work only, before a device is touched."""
    if spec is None:
        return None
    if spec == "auto":
        candidates = [os.path.join(data_path, bag_name + "_mask.png"), os.path.join(data_path, "mask.png")]
        path = next((p for p in candidates if os.path.exists(p)), None)
        if path is None:
            if log is not None:
                log(f"{bag_name}: no {bag_name}_mask.png and no mask.png in {data_path}: the whole image is used")
            return None
    else:
        path = str(spec)
        if not os.path.exists(path):
            raise FileNotFoundError(f"error: failed to open mask {path}")
    mask = read_png_gray(path)
    if tuple(mask.shape) != (int(image_shape[0]), int(image_shape[1])):
        raise ValueError(f"{path}: the mask is {mask.shape[1]}x{mask.shape[0]}, the image of {bag_name} {int(image_shape[1])}x{int(image_shape[0])}")
    return mask


def add_selection_options(parser):
    """``--mask``, ``--mask_margin``, ``--min_range``, ``--max_range`` of ``calibrate`` and ``viewer`` (extensions; the reference has
    no such options)."""
    parser.add_argument("--mask", default=None, metavar="PATH|auto", help="8-bit PNG of the image's size, zero = ignore: one file for all bags, or 'auto' = <bag>_mask.png, else mask.png (extension)")
    parser.add_argument("--mask_margin", type=int, default=None, help="pixels the ignored region is grown by, 0..64 (default 2: the reach of the B-spline) (extension)")
    parser.add_argument("--min_range", type=float, default=None, help="ignore LiDAR points closer than this [m] (default 0) (extension)")
    parser.add_argument("--max_range", type=float, default=None, help="ignore LiDAR points farther than this [m] (default inf) (extension)")


def selection_options(args):
    """``None`` when none of the four options is given (the caller's code path is then the one without them), else
    ``{"mask": spec | None, "margin", "min_range", "max_range"}`` with the defaults filled in.  Refuses (SystemExit) a margin outside
    [0, 64], a negative or NaN range and ``max_range < min_range``: host checks, before a device is touched."""
    given = [getattr(args, k, None) for k in ("mask", "mask_margin", "min_range", "max_range")]
    if all(v is None for v in given):
        return None
    margin = 2 if args.mask_margin is None else int(args.mask_margin)
    lo = 0.0 if args.min_range is None else float(args.min_range)
    hi = float("inf") if args.max_range is None else float(args.max_range)
    if not 0 <= margin <= 64:
        raise SystemExit("error: --mask_margin must lie in [0, 64]")
    if not lo >= 0.0 or not hi >= lo:  # (a NaN fails both)
        raise SystemExit("error: 0 <= --min_range <= --max_range expected")
    return {"mask": args.mask, "margin": margin, "min_range": lo, "max_range": hi}


def write_preprocessed(data_path, camera, bags, init_T_lidar_camera_tum=None, meta=None, lidar_images=None):
    """Write a directory in ``preprocess``'s output format (preprocess.cpp:150-232): ``calib.json``,
    ``<bag>.png``, ``<bag>.ply`` and, when given, ``<bag>_lidar_intensities.png`` /
    ``<bag>_lidar_indices.png``.  ``camera`` = (model, intrinsics, distortion); ``bags`` = list of
    ``(name, image_u8, points, intensities)``; ``lidar_images`` = {name: (intensity float HxW, index int32 HxW)}."""
    os.makedirs(data_path, exist_ok=True)
    for name, image, points, intensities in bags:
        write_png_gray(os.path.join(data_path, name + ".png"), image)
        write_ply(os.path.join(data_path, name + ".ply"), points, intensities)
        if lidar_images and name in lidar_images:
            inten, idx = lidar_images[name]
            # convertTo(CV_8UC1, 255.0): saturate_cast<uchar>(round-half-even(v * 255))
            write_png_gray(os.path.join(data_path, name + "_lidar_intensities.png"), np.clip(np.rint(np.asarray(inten) * 255.0), 0, 255).astype(np.uint8))
            write_index_png(os.path.join(data_path, name + "_lidar_indices.png"), idx)
    config = {
        "meta": dict({"data_path": data_path, "bag_names": [b[0] for b in bags]}, **(meta or {})),
        "camera": {"camera_model": camera[0], "intrinsics": [float(v) for v in camera[1]], "distortion_coeffs": [float(v) for v in camera[2]]},
    }
    if init_T_lidar_camera_tum is not None:
        config["results"] = {"init_T_lidar_camera": [float(v) for v in init_T_lidar_camera_tum]}
    write_calib(data_path, config)
    return config
