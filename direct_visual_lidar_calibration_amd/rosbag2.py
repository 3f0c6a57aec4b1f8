"""A reader of ROS2 bags -- sqlite3 and MCAP storage -- and of the four CDR-serialised message types ``preprocess`` needs, in pure
Python: there is no ROS, no ``rosbag2_cpp``, no Fast-CDR and no libmcap here.  It has the surface ``preprocess_ros1`` uses of
``rosbag1`` and shares that module's tuples, constants and helpers, so everything downstream of a decoded message is the same code.

==============================================  =========================================================
here                                            reference (through rosbag2_cpp / rclcpp, neither in the tree)
==============================================  =========================================================
``valid_bag(path)``                             ``rosbag2_cpp::Reader::open`` succeeding (src/preprocess_ros2.cpp:84-93)
``Bag(path).topics_and_types()``                ``reader.get_all_topics_and_types()`` (:95-104)
``Bag(path).messages(topic)``                   ``reader.set_filter({topic})`` + ``read_next`` (:28-50, :59-82)
``decode_pointcloud2 / _image / _compressed_image / _camera_info``   ``rclcpp::Serialization<T>::deserialize_message``
==============================================  =========================================================

A bag is a directory with ``metadata.yaml`` (``storage_identifier`` sqlite3 or mcap, ``relative_file_paths`` read one after the other in
list order, ``compression_format`` / ``compression_mode``), a bare sqlite3 file with the tables ``topics`` and ``messages``, or a bare MCAP
file.

sqlite3: ``topics(id, name, type, serialization_format, ...)`` and ``messages(id, topic_id, timestamp, data)``; the columns are selected
by name, so the schema's later additions do not matter.  The file is opened read-only and the messages come from a cursor, ``ORDER BY
timestamp, id``: memory does not grow with the bag.

MCAP (the public specification): the magic ``\\x89MCAP0\\r\\n``, records ``u8 opcode, u64 length, body``, the magic again; little-endian,
strings and byte arrays ``u32``-prefixed.  One pass from the front over Header (1), Schema (3), Channel (4), Message (5) and Chunk (6) up to
DataEnd (15); the summary section, the index records and every other opcode are skipped, so an unindexed file reads like an indexed
one.  The file is mapped, not read; what is kept per message is its time and position.

CDR (plain CDR version 1 as the DDS-RTPS and DDS-XTYPES specifications describe it, what ROS2 writes): a 4-byte encapsulation header
``00 01 xx xx`` (little-endian), then the fields, each primitive aligned to its own size COUNTED FROM THE BYTE AFTER THE HEADER;
``string`` = u32 length including the NUL, bytes; ``T[]`` = u32 count, elements; ``T[n]`` = elements; ``builtin_interfaces/Time`` =
int32 sec, uint32 nanosec.  Big-endian CDR and the PL_CDR / CDR2 encapsulations are refused by name.

Every read is bounds-checked: a truncated file, record, chunk or message is a ``ValueError`` with the path and the byte offset.

This reader is written from the format descriptions alone and is UNPINNED against ``rosbag2_cpp``, Fast-CDR and libmcap: its tests read
bytes spelled out by hand from those descriptions and bags from a writer that shares no code with it, not a real recording.
"""
import mmap
import os
import sqlite3
import struct
import tempfile
import urllib.parse
import zlib

import numpy as np

from .rosbag1 import (DATATYPE_DTYPES, FLOAT32, FLOAT64, INT8, INT16, INT32, UINT8, UINT16, UINT32,  # noqa: F401 (the shared surface)
                      CameraInfo, CompressedImage, Image, Message, PointCloud2, PointField, camera_from_info, compressed_to_mono8, field_table, image_to_mono8, num_points,
                      read_field, read_field_all, stamp_to_sec, to_mono8)

SQLITE_MAGIC = b"SQLite format 3\x00"
MCAP_MAGIC = b"\x89MCAP0\r\n"
OP_HEADER, OP_SCHEMA, OP_CHANNEL, OP_MESSAGE, OP_CHUNK, OP_DATA_END = 0x01, 0x03, 0x04, 0x05, 0x06, 0x0F
METADATA = "metadata.yaml"


# ---------------------------------------------------------------------------------------------- what is a bag
def _metadata(path):
    """``(storage_identifier, [files], compression_format, compression_mode)`` of a bag directory; ``ValueError`` if it is none"""
    import yaml

    name = os.path.join(path, METADATA)
    try:
        with open(name, "rb") as f:
            doc = yaml.safe_load(f)
    except (OSError, yaml.YAMLError, UnicodeDecodeError) as e:
        raise ValueError(f"{path}: not a ROS2 bag directory ({METADATA} does not read: {e})") from None
    info = doc.get("rosbag2_bagfile_information") if isinstance(doc, dict) else None
    files = info.get("relative_file_paths") if isinstance(info, dict) else None
    if not isinstance(files, list) or not files or not all(isinstance(f, str) for f in files):
        raise ValueError(f"{path}: not a ROS2 bag directory ({METADATA} has no rosbag2_bagfile_information.relative_file_paths)")
    files = [os.path.join(path, f) for f in files]
    for f in files:
        if not os.path.isfile(f):
            raise ValueError(f"{path}: {METADATA} lists {f}, which does not exist")
    mode = str(info.get("compression_mode") or "")
    return str(info.get("storage_identifier") or ""), files, str(info.get("compression_format") or ""), "" if mode.upper() == "NONE" else mode


def _sqlite_uri(path):
    return "file:" + urllib.parse.quote(os.path.abspath(path)) + "?mode=ro"


def _sqlite_tables(path):
    db = sqlite3.connect(_sqlite_uri(path), uri=True)
    try:
        return {row[0] for row in db.execute("SELECT name FROM sqlite_master WHERE type = 'table'")}
    finally:
        db.close()


def _bare_kind(path):
    """``"mcap"`` / ``"sqlite3"`` of a bare storage file, or ``None``"""
    with open(path, "rb") as f:
        head = f.read(16)
    if head[: len(MCAP_MAGIC)] == MCAP_MAGIC:
        return "mcap"
    if head == SQLITE_MAGIC and {"topics", "messages"} <= _sqlite_tables(path):
        return "sqlite3"
    return None


def valid_bag(path):
    """A directory with a ``metadata.yaml`` whose files all exist, a sqlite3 file with the tables ``topics`` and ``messages``, or a
    file that starts with the MCAP magic.  Anything else -- a ROS1 bag, an unreadable file -- is not a bag; nothing is raised."""
    try:
        if os.path.isdir(path):
            _metadata(str(path))
            return True
        return _bare_kind(path) is not None
    except (OSError, ValueError, sqlite3.Error):
        return False


# ---------------------------------------------------------------------------------------------- compression
def _zstd():
    """``bytes -> bytes`` of whichever zstd module imports, or ``None``"""
    try:
        from compression import zstd  # Python >= 3.14

        return zstd.decompress
    except ImportError:
        pass
    try:
        import zstandard

        return lambda data: zstandard.ZstdDecompressor().decompressobj().decompress(data)
    except ImportError:
        pass
    try:
        import zstd

        return zstd.decompress
    except ImportError:
        return None


def _lz4():
    try:
        import lz4.frame

        return lz4.frame.decompress
    except ImportError:
        return None


def _bag_decompressor(fmt, mode, where):
    """The decompressor of a bag whose ``metadata.yaml`` names a ``compression_mode`` (FILE: every storage file; MESSAGE: every payload)"""
    if mode.upper() not in ("FILE", "MESSAGE"):
        raise ValueError(f"{where}: unknown compression_mode '{mode}' (compression_format '{fmt}')")
    decompress = _zstd() if fmt.lower() == "zstd" else None
    if decompress is None:
        raise ValueError(f"{where}: compression_mode '{mode}' with compression_format '{fmt}' needs a {fmt or 'decompression'} module, and none imports; "
                         "re-record the bag or convert it uncompressed (ros2 bag convert)")
    return decompress


# ---------------------------------------------------------------------------------------------- sqlite3 storage
class _Sqlite3Store:
    """One ``.db3`` file.  ``topics``: [(id, name, type, serialization_format)] in id order."""

    def __init__(self, path, where, unpack=None):
        self.where, self.unpack = where, unpack
        try:
            self.db = sqlite3.connect(_sqlite_uri(path), uri=True)
            columns = {row[1] for row in self.db.execute("PRAGMA table_info(topics)")}
            message_columns = {row[1] for row in self.db.execute("PRAGMA table_info(messages)")}
            if not {"id", "name", "type", "serialization_format"} <= columns or not {"id", "topic_id", "timestamp", "data"} <= message_columns:
                raise ValueError(f"{where}: not a rosbag2 sqlite3 file (no table topics(id, name, type, serialization_format) or messages(id, topic_id, timestamp, data))")
            self.topics = [(int(i), str(n), str(t), str(s)) for i, n, t, s in self.db.execute("SELECT id, name, type, serialization_format FROM topics ORDER BY id")]
        except sqlite3.Error as e:
            raise ValueError(f"{where}: sqlite3 does not read the file: {e}") from None

    def messages(self, topic):
        by_id = {t[0]: t for t in self.topics}
        ids = [t[0] for t in self.topics if topic is None or t[1] == topic]  # a name listed twice: all its ids
        for t in self.topics:
            if topic is not None and t[1] == topic and t[3] != "cdr":
                raise ValueError(f"{self.where}: topic '{topic}' is serialised as '{t[3]}'; only cdr is read")
        if not ids:
            return
        sql = "SELECT topic_id, timestamp, data FROM messages" + ("" if topic is None else f" WHERE topic_id IN ({', '.join('?' * len(ids))})") + " ORDER BY timestamp, id"
        try:
            for topic_id, stamp, data in self.db.execute(sql, [] if topic is None else ids):
                t = by_id.get(topic_id)
                if t is None:
                    raise ValueError(f"{self.where}: a message names topic id {topic_id}, which the table topics does not define")
                if t[3] != "cdr":
                    raise ValueError(f"{self.where}: topic '{t[1]}' is serialised as '{t[3]}'; only cdr is read")
                if not isinstance(data, bytes) or not isinstance(stamp, int):
                    raise ValueError(f"{self.where}: a message of topic '{t[1]}' has no BLOB data or no integer timestamp")
                if self.unpack is not None:
                    data = self.unpack(data)
                yield Message(topic_id, t[1], t[2], divmod(stamp, 1000000000), memoryview(data))
        except sqlite3.Error as e:
            raise ValueError(f"{self.where}: sqlite3 does not read the messages: {e}") from None


# ---------------------------------------------------------------------------------------------- MCAP storage
class _Bytes:
    """Bounds-checked little-endian reads of ``buf[pos:end]``; offsets are reported relative to ``base`` in ``where``"""

    def __init__(self, buf, pos, end, where, base=0):
        self.buf, self.pos, self.end, self.where, self.base = buf, pos, end, where, base

    def need(self, n, what):
        if n < 0 or self.pos + n > self.end:
            raise ValueError(f"{self.where}: truncated {what} ({n} bytes wanted at byte offset {self.base + self.pos}, {self.end - self.pos} left)")

    def unpack(self, fmt, what):
        n = struct.calcsize(fmt)
        self.need(n, what)
        out = struct.unpack_from(fmt, self.buf, self.pos)
        self.pos += n
        return out

    def take(self, n, what):
        self.need(n, what)
        self.pos += n
        return self.buf[self.pos - n : self.pos]

    def string(self, what):
        return bytes(self.take(self.unpack("<I", what)[0], what)).decode("utf-8", "replace")


class _McapStore:
    """One MCAP file, scanned once.  ``schemas`` {id: name}, ``channels`` {id: (schema_id, topic, message_encoding)}; ``_index``:
    per message ``(log_time, file order, channel, chunk offset or -1, payload start, payload end)`` -- positions, not payloads."""

    def __init__(self, buf, where, unpack=None):
        self.buf, self.where, self.unpack = buf, where, unpack
        self.profile = self.library = None
        self.schemas, self.channels, self._index = {}, {}, []
        self._chunks = {}  # compressed chunks: {offset: (compression, start, end of the stored bytes, uncompressed size)}
        self._cached = (None, None)  # the last compressed chunk that was decoded: (offset, memoryview)
        n = len(buf)
        if n < len(MCAP_MAGIC) or bytes(buf[: len(MCAP_MAGIC)]) != MCAP_MAGIC:
            raise ValueError(f"{where}: not an MCAP file (it does not start with the MCAP magic, byte offset 0)")
        closed = n >= 2 * len(MCAP_MAGIC) and bytes(buf[n - len(MCAP_MAGIC) :]) == MCAP_MAGIC
        self._scan(buf, len(MCAP_MAGIC), n - len(MCAP_MAGIC) if closed else n, where, 0, -1)
        if not closed:
            raise ValueError(f"{where}: truncated MCAP file: it does not end with the MCAP magic (file of {n} bytes, byte offset {max(0, n - len(MCAP_MAGIC))})")
        self._index.sort(key=lambda m: (m[0], m[1]))

    def _scan(self, buf, pos, end, where, base, chunk, top=True):
        """The records of ``buf[pos:end]``: the file's (``top``) or a chunk's, where only schemas, channels and messages count.  ``chunk``:
        -1 when ``buf`` is the file itself, else the file offset of the compressed chunk ``buf`` is the decoded content of"""
        while pos < end:
            r = _Bytes(buf, pos, end, where, base)
            op, length = r.unpack("<BQ", "record (opcode and length)")
            r.need(length, f"record 0x{op:02x} at byte offset {base + pos}")
            body = _Bytes(buf, r.pos, r.pos + length, where, base)
            pos = r.pos + length
            if op == OP_MESSAGE:
                channel, _sequence, log_time, _publish_time = body.unpack("<HIQQ", "message record")
                self._index.append((log_time, len(self._index), channel, chunk, body.pos, body.end))
            elif op == OP_CHANNEL:
                cid, schema_id = body.unpack("<HH", "channel record")
                topic, encoding = body.string("channel record"), body.string("channel record")
                body.take(body.unpack("<I", "channel record")[0], "channel record (metadata)")
                self.channels.setdefault(cid, (schema_id, topic, encoding))
            elif op == OP_SCHEMA:
                (sid,) = body.unpack("<H", "schema record")
                name, _encoding = body.string("schema record"), body.string("schema record")
                body.take(body.unpack("<I", "schema record")[0], "schema record (data)")
                self.schemas.setdefault(sid, name)
            elif op == OP_HEADER and top:
                self.profile, self.library = body.string("header record"), body.string("header record")
            elif op == OP_CHUNK and top:
                offset = base + body.pos - 9
                _start, _end, size, crc = body.unpack("<QQQI", "chunk record")
                compression = body.string("chunk record")
                (stored,) = body.unpack("<Q", "chunk record")
                body.need(stored, "chunk record (records)")
                if compression == "":
                    if stored != size:
                        raise ValueError(f"{where}: the chunk at byte offset {offset} holds {stored} bytes, its header says {size}")
                    self._check_crc(buf[body.pos : body.pos + stored], crc, offset)
                    self._scan(buf, body.pos, body.pos + stored, where, base, -1, top=False)  # zero-copy: positions in the file itself
                else:
                    inner = self._inflate(offset, compression, buf[body.pos : body.pos + stored], size, crc)
                    self._scan(inner, 0, len(inner), f"{where}: chunk at byte offset {offset}", 0, offset, top=False)
                    self._chunks[offset] = (compression, body.pos, body.pos + stored, size)
            elif op == OP_DATA_END and top:
                return  # the summary section and the footer are not read
            # message index, chunk index, attachment, statistics, metadata, summary offset, footer and anything unknown: skipped

    def _check_crc(self, data, crc, offset):
        if crc != 0 and zlib.crc32(data) != crc:
            raise ValueError(f"{self.where}: the chunk at byte offset {offset} has CRC {zlib.crc32(data):#010x}, its header says {crc:#010x}")

    def _inflate(self, offset, compression, data, size, crc=0):
        decompress = {"lz4": _lz4, "zstd": _zstd}.get(compression, lambda: None)()
        if decompress is None:
            raise ValueError(f"{self.where}: the chunk at byte offset {offset} is compressed with '{compression}', which needs a module that does not import here; "
                             "re-record the file or convert it uncompressed (mcap compress --compression none, ros2 bag convert)")
        try:
            out = memoryview(decompress(bytes(data)))
        except Exception as e:
            raise ValueError(f"{self.where}: the {compression} chunk at byte offset {offset} does not decompress: {e}") from None
        if len(out) != size:
            raise ValueError(f"{self.where}: the chunk at byte offset {offset} holds {len(out)} bytes, its header says {size}")
        self._check_crc(out, crc, offset)
        return out

    def _payload(self, chunk, start, end):
        if chunk < 0:
            return self.buf[start:end]
        if self._cached[0] != chunk:  # messages come nearly chunk after chunk: one decoded chunk is kept, not all
            compression, lo, hi, size = self._chunks[chunk]
            self._cached = (chunk, self._inflate(chunk, compression, self.buf[lo:hi], size))
        return self._cached[1][start:end]

    @property
    def topics(self):
        return [(cid, topic, self.schemas.get(schema_id, ""), encoding) for cid, (schema_id, topic, encoding) in sorted(self.channels.items())]

    def messages(self, topic):
        for log_time, _, cid, chunk, start, end in self._index:
            c = self.channels.get(cid)
            if c is None:
                raise ValueError(f"{self.where}: a message names channel {cid}, which the file does not define")
            if topic is not None and c[1] != topic:
                continue
            if c[2] != "cdr":
                raise ValueError(f"{self.where}: topic '{c[1]}' is serialised as '{c[2]}'; only cdr is read")
            data = self._payload(chunk, start, end)
            if self.unpack is not None:
                data = memoryview(self.unpack(bytes(data)))
            yield Message(cid, c[1], self.schemas.get(c[0], ""), divmod(log_time, 1000000000), data)


def _map_file(path):
    with open(path, "rb") as f:
        try:
            return memoryview(mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ))
        except ValueError:  # an empty file cannot be mapped
            return memoryview(b"")


# ---------------------------------------------------------------------------------------------- the bag
class Bag:
    """A ROS2 bag: a directory with ``metadata.yaml``, or one bare ``.db3`` / ``.mcap`` file.  ``messages(topic)`` gives the topic's
    ``Message`` tuples (``rosbag1.Message``; ``conn`` is the topic id or channel id, ``time`` the (sec, nsec) of the storage's
    timestamp, ``data`` a zero-copy view of the CDR blob) in ascending time, ties in storage order, file after file."""

    def __init__(self, path):
        self.path = str(path)
        self.compression_format = self.compression_mode = ""
        try:
            if os.path.isdir(self.path):
                self.storage, files, self.compression_format, self.compression_mode = _metadata(self.path)
            else:
                self.storage, files = _bare_kind(self.path), [self.path]
        except (OSError, sqlite3.Error) as e:
            raise ValueError(f"{self.path}: not a ROS2 bag ({e})") from None
        if self.storage not in ("sqlite3", "mcap"):
            raise ValueError(f"{self.path}: not a ROS2 bag this reader knows (storage '{self.storage}'; sqlite3 and mcap are read)" if self.storage else
                             f"{self.path}: not a ROS2 bag (no directory with {METADATA}, no sqlite3 file with the tables topics and messages, no MCAP magic; ROS1 bags are read by rosbag1)")
        unpack_file = unpack_message = None
        if self.compression_mode:
            unpack = _bag_decompressor(self.compression_format, self.compression_mode, self.path)
            unpack_file, unpack_message = (unpack, None) if self.compression_mode.upper() == "FILE" else (None, unpack)
        self._keep = []  # the temporary files of a FILE-compressed sqlite3 bag
        self._stores = []
        for f in files:
            if self.storage == "mcap":
                buf = _map_file(f) if unpack_file is None else memoryview(unpack_file(open(f, "rb").read()))
                self._stores.append(_McapStore(buf, f, unpack_message))
            else:
                if unpack_file is not None:
                    tmp = tempfile.NamedTemporaryFile(suffix=".db3")
                    tmp.write(unpack_file(open(f, "rb").read()))
                    tmp.flush()
                    self._keep.append(tmp)
                self._stores.append(_Sqlite3Store(f if unpack_file is None else tmp.name, f, unpack_message))

    def topics_and_types(self):
        """``(topic, type)`` per topic row or channel in id order; a later file of a split bag adds only what the earlier ones lack"""
        out = []
        for k, store in enumerate(self._stores):
            out += [(t[1], t[2]) for t in store.topics if k == 0 or (t[1], t[2]) not in out]
        return out

    def messages(self, topic=None):
        for store in self._stores:
            yield from store.messages(topic)

    def first_message(self, topic, type_substring=None):
        """The first message of the topic whose recorded type is ``type_substring`` (``.../msg/<type_substring>``), or ``None``"""
        for m in self.messages(topic):
            if type_substring is None or m.type.endswith("/" + type_substring) or m.type == type_substring:
                return m
        return None


def topics_and_types(path):
    return Bag(path).topics_and_types()


# ---------------------------------------------------------------------------------------------- CDR message decoding
ENCAPSULATIONS = {b"\x00\x00": "CDR_BE (big-endian plain CDR)", b"\x00\x02": "PL_CDR_BE", b"\x00\x03": "PL_CDR_LE", b"\x00\x06": "CDR2_BE", b"\x00\x07": "CDR2_LE",
                  b"\x00\x08": "D_CDR2_BE", b"\x00\x09": "D_CDR2_LE", b"\x00\x0a": "PL_CDR2_BE", b"\x00\x0b": "PL_CDR2_LE"}


class _Cdr:
    def __init__(self, data, what):
        self.buf = data if isinstance(data, memoryview) else memoryview(data)
        self.what = what
        self.pos = 0
        kind = bytes(self.take(4)[:2])
        if kind != b"\x00\x01":
            raise ValueError(f"{what}: the encapsulation header {kind.hex()} is {ENCAPSULATIONS.get(kind, 'unknown')}; only 0001, little-endian plain CDR, is read")

    def take(self, n, align=1):
        pos = self.pos + (4 - self.pos) % align  # alignment counts from byte 4, the first after the encapsulation header
        if n < 0 or pos + n > len(self.buf):
            raise ValueError(f"{self.what}: truncated message ({n} bytes wanted at byte offset {pos} of {len(self.buf)})")
        self.pos = pos + n
        return self.buf[pos : pos + n]

    def u8(self):
        return self.take(1)[0]

    def u32(self):
        return struct.unpack("<I", self.take(4, 4))[0]

    def u32s(self, n):
        return struct.unpack(f"<{n}I", self.take(4 * n, 4))

    def f64s(self, n):
        return list(struct.unpack(f"<{n}d", self.take(8 * n, 8))) if n else []

    def string(self):
        raw = bytes(self.take(self.u32()))
        return (raw[:-1] if raw.endswith(b"\x00") else raw).decode("utf-8", "replace")

    def header(self):
        """std_msgs/msg/Header -> (stamp (sec, nanosec), frame_id)"""
        sec, nsec = struct.unpack("<iI", self.take(8, 4))
        return (sec, nsec), self.string()

    def octets(self):
        return self.take(self.u32())


def decode_pointcloud2(data):
    """sensor_msgs/msg/PointCloud2; ``data`` of the result is a zero-copy uint8 view of the blob's point records, at whatever byte
    offset the header and the field table leave them"""
    r = _Cdr(data, "sensor_msgs/msg/PointCloud2")
    stamp, frame_id = r.header()
    height, width = r.u32s(2)
    fields = []
    for _ in range(r.u32()):
        name = r.string()
        offset, datatype, count = r.u32(), r.u8(), r.u32()
        fields.append(PointField(name, offset, datatype, count))
    is_bigendian = r.u8()
    point_step, row_step = r.u32s(2)
    payload = np.frombuffer(r.octets(), dtype=np.uint8)
    is_dense = r.u8()
    return PointCloud2(stamp, frame_id, height, width, fields, is_bigendian, point_step, row_step, payload, is_dense)


def decode_points(type_name, data, **kw):
    """``rosbag1.decode_points`` for CDR blobs: ``sensor_msgs/msg/PointCloud2``, ``velodyne_msgs/msg/VelodyneScan`` (packets 1216 bytes
    apart) or ``livox_ros_driver2/msg/CustomMsg`` (points 20 bytes apart) as a ``PointCloud2`` tuple; ``None`` for any other type"""
    from . import lidar_messages

    return lidar_messages.decode_points(type_name, data, cdr=True, **kw)


def batch_points(messages, **kw):
    """``rosbag1.batch_points`` for CDR blobs (``ouster_msgs/msg/PacketMsg``, ``ouster_sensor_msgs/msg/PacketMsg``)"""
    from . import lidar_messages

    return lidar_messages.batch_points(messages, cdr=True, **kw)


def decode_string(data):
    """std_msgs/msg/String"""
    return _Cdr(data, "std_msgs/msg/String").string()


def decode_image(data):
    """sensor_msgs/msg/Image; ``data`` is a zero-copy uint8 view"""
    r = _Cdr(data, "sensor_msgs/msg/Image")
    stamp, frame_id = r.header()
    height, width = r.u32s(2)
    encoding = r.string()
    is_bigendian = r.u8()
    step = r.u32()
    return Image(stamp, frame_id, height, width, encoding, is_bigendian, step, np.frombuffer(r.octets(), dtype=np.uint8))


def decode_compressed_image(data):
    r = _Cdr(data, "sensor_msgs/msg/CompressedImage")
    stamp, frame_id = r.header()
    fmt = r.string()
    return CompressedImage(stamp, frame_id, fmt, r.octets())


def decode_camera_info(data):
    r = _Cdr(data, "sensor_msgs/msg/CameraInfo")
    stamp, frame_id = r.header()
    height, width = r.u32s(2)
    model = r.string()
    D = r.f64s(r.u32())
    K, R, P = r.f64s(9), r.f64s(9), r.f64s(12)
    binning_x, binning_y = r.u32s(2)
    roi = r.u32s(4) + (r.u8(),)
    return CameraInfo(stamp, frame_id, height, width, model, D, K, R, P, binning_x, binning_y, roi)
