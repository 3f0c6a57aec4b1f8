"""A reader of ROS1 bag files (format 2.0) and of the four message types ``preprocess`` needs, in pure Python: there is no ROS here.

==============================================  =========================================================
here                                            reference (through rosbag / cv_bridge, neither in the tree)
==============================================  =========================================================
``valid_bag(path)``                             ``rosbag::Bag(path).isOpen()`` (src/preprocess_ros1.cpp:74-77)
``topics_and_types(path)``                      ``rosbag::View::getConnections`` (:79-89)
``Bag(path).messages(topic)``                   ``rosbag::View(bag, rosbag::TopicQuery(topic))`` (:21-26, :54-63)
``decode_pointcloud2 / _image / _compressed_image / _camera_info``   ``m.instantiate<sensor_msgs::...>()``
``decode_points`` (``lidar_messages``)          the vendor driver replayed between the bag and the points topic
``to_mono8`` / ``image_to_mono8`` / ``compressed_to_mono8``   ``cv_bridge::toCvCopy(msg, "mono8")`` (:126-135)
==============================================  =========================================================

The file format (the public "Bag format 2.0" specification): the line ``#ROSBAG V2.0``, then records ``u32 header_len, header,
u32 data_len, data``, all little-endian; a header is a sequence of ``u32 field_len, name=value`` fields with a one-byte ``op``:
bag header (3), chunk (5: ``compression`` none / bz2 / lz4, its data a run of connection and message-data records), connection
(7), message data (2), index data (4) and chunk info (6).  The file is scanned once from front to back; the index records are
skipped, so an unindexed bag reads like an indexed one.  Messages are ROS1-serialised: little-endian, ``string`` = u32 length +
bytes, ``T[]`` = u32 count + elements, ``T[n]`` = n elements, ``time`` = u32 sec + u32 nsec.
"""
import bz2
import struct
from collections import namedtuple

import numpy as np

MAGIC = b"#ROSBAG V2.0\n"
OP_MESSAGE, OP_BAG_HEADER, OP_INDEX, OP_CHUNK, OP_CHUNK_INFO, OP_CONNECTION = 2, 3, 4, 5, 6, 7

# sensor_msgs/PointField datatypes
INT8, UINT8, INT16, UINT16, INT32, UINT32, FLOAT32, FLOAT64 = 1, 2, 3, 4, 5, 6, 7, 8
DATATYPE_DTYPES = {INT8: "<i1", UINT8: "<u1", INT16: "<i2", UINT16: "<u2", INT32: "<i4", UINT32: "<u4", FLOAT32: "<f4", FLOAT64: "<f8"}

Connection = namedtuple("Connection", "conn topic type md5sum message_definition")
Message = namedtuple("Message", "conn topic type time data")  # time: (sec, nsec) of the record; data: the serialised message
PointField = namedtuple("PointField", "name offset datatype count")
PointCloud2 = namedtuple("PointCloud2", "stamp frame_id height width fields is_bigendian point_step row_step data is_dense")
Image = namedtuple("Image", "stamp frame_id height width encoding is_bigendian step data")
CompressedImage = namedtuple("CompressedImage", "stamp frame_id format data")
CameraInfo = namedtuple("CameraInfo", "stamp frame_id height width distortion_model D K R P binning_x binning_y roi")


def valid_bag(path):
    """The file starts with the 13 bytes ``#ROSBAG V2.0\\n``; anything unreadable is not a bag."""
    try:
        with open(path, "rb") as f:
            return f.read(len(MAGIC)) == MAGIC
    except OSError:
        return False


def _parse_header(buf, start, end, where):
    """``{name: value bytes}`` of the header fields in ``buf[start:end]``"""
    fields = {}
    pos = start
    while pos < end:
        if pos + 4 > end:
            raise ValueError(f"{where}: truncated header field length at byte offset {pos}")
        (flen,) = struct.unpack_from("<I", buf, pos)
        pos += 4
        if pos + flen > end:
            raise ValueError(f"{where}: truncated header field at byte offset {pos}")
        field = bytes(buf[pos : pos + flen])
        eq = field.find(b"=")
        if eq < 0:
            raise ValueError(f"{where}: header field without '=' at byte offset {pos}")
        fields[field[:eq].decode("ascii", "replace")] = field[eq + 1 :]
        pos += flen
    return fields


def _records(buf, base, where):
    """``(header fields, data memoryview, byte offset)`` of every record in ``buf``; offsets are reported relative to ``base``
    (the position of ``buf`` in the file, or of a chunk's data)."""
    pos, end = 0, len(buf)
    while pos < end:
        if pos + 4 > end:
            raise ValueError(f"{where}: truncated record (header length) at byte offset {base + pos}")
        (hlen,) = struct.unpack_from("<I", buf, pos)
        if pos + 4 + hlen + 4 > end:
            raise ValueError(f"{where}: truncated record (header) at byte offset {base + pos}")
        header = _parse_header(buf, pos + 4, pos + 4 + hlen, where)
        (dlen,) = struct.unpack_from("<I", buf, pos + 4 + hlen)
        dpos = pos + 8 + hlen
        if dpos + dlen > end:
            raise ValueError(f"{where}: truncated record (data) at byte offset {base + pos}")
        yield header, buf[dpos : dpos + dlen], base + pos
        pos = dpos + dlen


def _value(header, name, fmt, where, offset):
    if name not in header or len(header[name]) != struct.calcsize(fmt):
        raise ValueError(f"{where}: record at byte offset {offset} has no valid '{name}' field")
    return struct.unpack(fmt, header[name])


def _decompress(compression, data, size, where, offset):
    if compression == "none":
        out = data
    elif compression == "bz2":
        try:
            out = memoryview(bz2.decompress(bytes(data)))
        except (OSError, ValueError) as e:
            raise ValueError(f"{where}: bz2 chunk at byte offset {offset} does not decompress: {e}") from None
    elif compression == "lz4":
        try:
            import lz4.frame
        except ImportError:
            raise ValueError(f"{where}: chunk compression 'lz4' needs the lz4 module (import lz4.frame failed); re-compress the bag with bz2 or none") from None
        out = memoryview(lz4.frame.decompress(bytes(data)))
    else:
        raise ValueError(f"{where}: unknown chunk compression '{compression}' at byte offset {offset}")
    if len(out) != size:
        raise ValueError(f"{where}: chunk at byte offset {offset} holds {len(out)} bytes, its header says {size}")
    return out


class Bag:
    """One sequential pass over the file: ``connections`` ({conn id: Connection}) and, per ``messages(topic)``, the messages of
    the topic in ascending record time, ties in file order (``rosbag::View``).  The file is held as one ``bytes``; uncompressed
    message payloads are zero-copy views of it."""

    def __init__(self, path):
        self.path = str(path)
        with open(path, "rb") as f:
            raw = f.read()
        if raw[: len(MAGIC)] != MAGIC:
            raise ValueError(f"{self.path}: not a ROS1 bag (the file does not start with '#ROSBAG V2.0'; ROS2 bags -- sqlite3 / mcap -- are not read here)")
        self.connections = {}
        self._messages = []  # (time key, file order, conn, (sec, nsec), data)
        self.index_pos = self.conn_count = self.chunk_count = None
        buf = memoryview(raw)[len(MAGIC) :]
        for header, data, offset in _records(buf, len(MAGIC), self.path):
            op = self._op(header, offset)
            if op == OP_BAG_HEADER:
                (self.index_pos,) = _value(header, "index_pos", "<Q", self.path, offset)
                (self.conn_count,) = _value(header, "conn_count", "<I", self.path, offset)
                (self.chunk_count,) = _value(header, "chunk_count", "<I", self.path, offset)
            elif op == OP_CHUNK:
                compression = header.get("compression", b"none").decode("ascii", "replace")
                (size,) = _value(header, "size", "<I", self.path, offset)
                inner = _decompress(compression, data, size, self.path, offset)
                for h2, d2, o2 in _records(inner, 0, f"{self.path}: chunk at byte offset {offset}"):
                    self._conn_or_message(self._op(h2, o2), h2, d2, o2)
            else:
                self._conn_or_message(op, header, data, offset)
        self._messages.sort(key=lambda m: (m[0], m[1]))

    def _op(self, header, offset):
        if "op" not in header or len(header["op"]) != 1:
            raise ValueError(f"{self.path}: record at byte offset {offset} has no 'op' field")
        return header["op"][0]

    def _conn_or_message(self, op, header, data, offset):
        if op == OP_CONNECTION:
            (conn,) = _value(header, "conn", "<I", self.path, offset)
            info = _parse_header(data, 0, len(data), self.path)
            topic = info.get("topic", header.get("topic", b"")).decode("utf-8", "replace")
            if conn not in self.connections:
                self.connections[conn] = Connection(conn, topic, info.get("type", b"").decode("ascii", "replace"), info.get("md5sum", b"").decode("ascii", "replace"),
                                                    info.get("message_definition", b"").decode("utf-8", "replace"))
        elif op == OP_MESSAGE:
            (conn,) = _value(header, "conn", "<I", self.path, offset)
            sec, nsec = _value(header, "time", "<II", self.path, offset)
            self._messages.append(((sec, nsec), len(self._messages), conn, (sec, nsec), data))
        # index data, chunk info and anything else: skipped

    def topics_and_types(self):
        return [(c.topic, c.type) for _, c in sorted(self.connections.items())]

    def messages(self, topic=None):
        """``Message`` tuples in ascending record time (ties in file order), of one topic -- over all its connections -- or of all"""
        for _, _, conn, stamp, data in self._messages:
            c = self.connections.get(conn)
            if c is None:
                raise ValueError(f"{self.path}: a message names connection {conn}, which the bag does not define")
            if topic is None or c.topic == topic:
                yield Message(conn, c.topic, c.type, stamp, data)

    def first_message(self, topic, type_substring=None):
        """The first message of the topic whose connection type contains ``type_substring`` (``get_first_message<T>``,
        src/preprocess_ros1.cpp:53-72: the first message that instantiates as T), or ``None``"""
        for m in self.messages(topic):
            if type_substring is None or m.type.endswith("/" + type_substring) or m.type == type_substring:
                return m
        return None


def topics_and_types(path):
    """``(topic, type)`` per connection, in connection-id order"""
    return Bag(path).topics_and_types()


# ---------------------------------------------------------------------------------------------- ROS1 message decoding
class _Reader:
    def __init__(self, data, what):
        self.buf = data if isinstance(data, memoryview) else memoryview(data)
        self.pos = 0
        self.what = what

    def take(self, n):
        if n < 0 or self.pos + n > len(self.buf):
            raise ValueError(f"{self.what}: truncated message ({n} bytes wanted at byte offset {self.pos} of {len(self.buf)})")
        out = self.buf[self.pos : self.pos + n]
        self.pos += n
        return out

    def unpack(self, fmt):
        return struct.unpack("<" + fmt, self.take(struct.calcsize("<" + fmt)))

    def u8(self):
        return self.unpack("B")[0]

    def u32(self):
        return self.unpack("I")[0]

    def string(self):
        return bytes(self.take(self.u32())).decode("utf-8", "replace")

    def header(self):
        """std_msgs/Header -> (stamp (sec, nsec), frame_id)"""
        _seq, sec, nsec = self.unpack("III")
        return (sec, nsec), self.string()


def stamp_to_sec(stamp):
    """``ros::Time::toSec``: sec + 1e-9 * nsec"""
    return float(stamp[0]) + 1e-9 * float(stamp[1])


def decode_pointcloud2(data):
    """sensor_msgs/PointCloud2; ``data`` of the result is a zero-copy uint8 view of the message's point records"""
    r = _Reader(data, "sensor_msgs/PointCloud2")
    stamp, frame_id = r.header()
    height, width = r.unpack("II")
    fields = []
    for _ in range(r.u32()):
        name = r.string()
        offset, datatype, count = r.unpack("IBI")
        fields.append(PointField(name, offset, datatype, count))
    is_bigendian = r.u8()
    point_step, row_step = r.unpack("II")
    payload = np.frombuffer(r.take(r.u32()), dtype=np.uint8)
    is_dense = r.u8()
    return PointCloud2(stamp, frame_id, height, width, fields, is_bigendian, point_step, row_step, payload, is_dense)


def decode_points(type_name, data, **kw):
    """The message of a points topic by its connection type -- ``sensor_msgs/PointCloud2``, ``velodyne_msgs/VelodyneScan`` (decoded on
    the GPU) or ``livox_ros_driver/CustomMsg`` (a view) -- as a ``PointCloud2`` tuple; ``None`` for any other type
    (``lidar_messages.decode_points`` lists the keywords)"""
    from . import lidar_messages

    return lidar_messages.decode_points(type_name, data, cdr=False, **kw)


def batch_points(messages, **kw):
    """The messages of a points topic with its ``ouster_ros/PacketMsg`` messages -- one UDP packet each -- grouped into one message per
    scan, which ``decode_points`` takes; every other message passes through untouched (``lidar_messages.batch_points``)"""
    from . import lidar_messages

    return lidar_messages.batch_points(messages, cdr=False, **kw)


def decode_string(data):
    """std_msgs/String"""
    return _Reader(data, "std_msgs/String").string()


def decode_image(data):
    """sensor_msgs/Image; ``data`` is a zero-copy uint8 view"""
    r = _Reader(data, "sensor_msgs/Image")
    stamp, frame_id = r.header()
    height, width = r.unpack("II")
    encoding = r.string()
    is_bigendian = r.u8()
    step = r.u32()
    payload = np.frombuffer(r.take(r.u32()), dtype=np.uint8)
    return Image(stamp, frame_id, height, width, encoding, is_bigendian, step, payload)


def decode_compressed_image(data):
    r = _Reader(data, "sensor_msgs/CompressedImage")
    stamp, frame_id = r.header()
    fmt = r.string()
    return CompressedImage(stamp, frame_id, fmt, r.take(r.u32()))


def decode_camera_info(data):
    r = _Reader(data, "sensor_msgs/CameraInfo")
    stamp, frame_id = r.header()
    height, width = r.unpack("II")
    model = r.string()
    D = list(r.unpack(f"{r.u32()}d"))
    K, R, P = list(r.unpack("9d")), list(r.unpack("9d")), list(r.unpack("12d"))
    binning_x, binning_y = r.unpack("II")
    roi = r.unpack("IIIIB")
    return CameraInfo(stamp, frame_id, height, width, model, D, K, R, P, binning_x, binning_y, roi)


def camera_from_info(info):
    """src/preprocess_ros1.cpp:114-124: ``(distortion_model, [K[0], K[4], K[2], K[5]], D)``"""
    return info.distortion_model, [info.K[0], info.K[4], info.K[2], info.K[5]], list(info.D)


_COLOR_ORDER = {"bgr8": (2, 1, 0), "rgb8": (0, 1, 2), "bgra8": (2, 1, 0), "rgba8": (0, 1, 2)}  # channel of R, G, B


def to_mono8(image):
    """``cv_bridge::toCvCopy(image, "mono8")`` for the 8-bit encodings: ``mono8`` as stored; ``bgr8`` / ``rgb8`` / ``bgra8`` /
    ``rgba8`` through OpenCV's 8-bit fixed-point luma ``(4899 R + 9617 G + 1868 B + 8192) >> 14``.  Returns a contiguous (H, W)
    uint8 array; every other encoding raises ``ValueError``."""
    enc = image.encoding
    if enc == "mono8":
        ch = 1
    elif enc in _COLOR_ORDER:
        ch = len(enc) - 1
    else:
        raise ValueError(f"sensor_msgs/Image encoding '{enc}' is not converted here (mono8, bgr8, rgb8, bgra8 and rgba8 are)")
    h, w, step = int(image.height), int(image.width), int(image.step)
    if step < w * ch or len(image.data) < h * step:
        raise ValueError(f"sensor_msgs/Image: {len(image.data)} data bytes for {h} rows of step {step} ({w} x {ch} bytes per row)")
    rows = np.frombuffer(image.data, dtype=np.uint8, count=h * step).reshape(h, step)[:, : w * ch]
    if ch == 1:
        return np.ascontiguousarray(rows)
    px = rows.reshape(h, w, ch)
    r, g, b = (px[:, :, k].astype(np.int64) for k in _COLOR_ORDER[enc])
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


def image_to_mono8(image, device=0, where="sensor_msgs/Image"):
    """``cv_bridge::toCvCopy(image, "mono8")`` for every encoding converted here.  The five 8-bit encodings are ``to_mono8``'s, on the
    host, with the bytes they always had.  Bayer mosaics (``bayer_rggb8`` ... ``bayer_grbg16``), packed YUV 4:2:2 (``yuv422`` /
    ``uyvy``, ``yuv422_yuy2`` / ``yuyv``), ``mono16`` and ``rgb16`` / ``bgr16`` / ``rgba16`` / ``bgra16`` are converted on GPU
    ``device`` (``nidreg_image_to_mono8``, which states the rules; unpinned against OpenCV and cv_bridge) from a zero-copy view of
    ``image.data``, wherever it lies.  Everything else -- ``8UC1``, ``16UC1``, ``32FC1``, ``nv21`` ... -- and an image whose size,
    step or data length is out of range raises ``ValueError`` before the device is touched; ``where`` names the message in it."""
    import ctypes

    from . import _lib

    if image.encoding == "mono8" or image.encoding in _COLOR_ORDER:
        return to_mono8(image)
    h, w = int(image.height), int(image.width)
    data = np.frombuffer(image.data, dtype=np.uint8)
    out = np.empty((min(h, 16384), min(w, 16384)), dtype=np.uint8)  # (a size beyond the library's range is refused by it below)
    lib = _lib.load()
    rc = lib.nidreg_image_to_mono8(int(device), data.ctypes.data, data.size, w, h, int(image.step), image.encoding.encode(), int(image.is_bigendian),
                                   out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), w)
    if rc == _lib.NIDREG_ERR_INVALID:
        raise ValueError(f"{where}: {_lib.last_error()}")
    _lib.check(rc, "nidreg_image_to_mono8")
    return out


def compressed_to_mono8(image, where="sensor_msgs/CompressedImage", device=0):
    """``cv_bridge::toCvCopy(msg, "mono8")`` of a compressed image: a PNG payload through ``dataset.decode_png_gray``; a baseline JPEG
    payload -- what ``image_transport`` publishes on ``.../compressed`` by default -- decoded on GPU ``device`` to BGR and taken
    through OpenCV's luma (``dataset.decode_jpeg_gray`` in BGR mode; cv_bridge passes ``IMREAD_UNCHANGED``, so no EXIF orientation
    is applied).  A JPEG outside the decoder's scope is refused with the reason."""
    from . import dataset

    payload = bytes(image.data)
    if payload[:8] != dataset.PNG_SIGNATURE:
        if payload[:2] == b"\xff\xd8" or "jpeg" in image.format.lower() or "jpg" in image.format.lower():
            return dataset.decode_jpeg_gray(payload, dataset.JPEG_GRAY_BGR, device=device, path=where)
        raise ValueError(f"error: failed to load image {where}: format '{image.format}' is not a PNG or JPEG payload")
    return dataset.decode_png_gray(payload, where)


# ---------------------------------------------------------------------------------------------- PointCloud2 fields
def field_table(cloud):
    """``{name: PointField}``; a name listed twice keeps its LAST entry (extract_raw_points overwrites, ros_cloud_converter.hpp:87-95)"""
    return {f.name: f for f in cloud.fields}


def num_points(cloud):
    return int(cloud.width) * int(cloud.height)


def read_field(cloud, field, index):
    """One value of ``field`` at the point indices ``index`` (array-like), as float64, from the raw bytes (no alignment assumed)"""
    dt = np.dtype(DATATYPE_DTYPES[field.datatype])
    idx = np.asarray(index, dtype=np.int64).reshape(-1)
    pos = idx * int(cloud.point_step) + int(field.offset)
    raw = cloud.data[(pos[:, None] + np.arange(dt.itemsize)[None, :]).reshape(-1)]
    return raw.view(dt).astype(np.float64)


def read_field_all(cloud, field):
    """The whole column of ``field`` as float64: a strided gather over the raw bytes"""
    dt = np.dtype(DATATYPE_DTYPES[field.datatype])
    n, step = num_points(cloud), int(cloud.point_step)
    if n == 0:
        return np.zeros(0)
    cols = np.lib.stride_tricks.as_strided(cloud.data[int(field.offset) :], shape=(n, dt.itemsize), strides=(step, 1))
    return np.ascontiguousarray(cols).view(dt).reshape(n).astype(np.float64)
