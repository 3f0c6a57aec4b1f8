"""A small ROS2 bag WRITER (test infrastructure, not a test): CDR serialisation of the message types the preprocessing reads, sqlite3
and MCAP storage files and ``metadata.yaml``, written with explicit ``struct.pack`` calls in the order the message definitions list
their fields.  It shares no code with direct_visual_lidar_calibration_amd/rosbag2.py -- the reader under test."""
import os
import sqlite3
import struct
import zlib

import numpy as np

MCAP_MAGIC = b"\x89MCAP0\r\n"
DATATYPE = {"i1": 1, "u1": 2, "i2": 3, "u2": 4, "i4": 5, "u4": 6, "f4": 7, "f8": 8}  # numpy code -> sensor_msgs/msg/PointField datatype
PC2, IMG, CIMG, INFO = "sensor_msgs/msg/PointCloud2", "sensor_msgs/msg/Image", "sensor_msgs/msg/CompressedImage", "sensor_msgs/msg/CameraInfo"


# ---- CDR (little-endian plain CDR; the alignment origin is the byte after the 4-byte encapsulation header)
class Cdr:
    def __init__(self, encapsulation=b"\x00\x01\x00\x00"):
        self.out = bytearray(encapsulation)

    def pad(self, size):
        while (len(self.out) - 4) % size:
            self.out.append(0)
        return self

    def u8(self, v):
        self.out += struct.pack("<B", v)
        return self

    def u32(self, *values):
        self.pad(4)
        self.out += struct.pack(f"<{len(values)}I", *values)
        return self

    def i32(self, v):
        self.pad(4)
        self.out += struct.pack("<i", v)
        return self

    def f64(self, *values):
        if values:
            self.pad(8)
            self.out += struct.pack(f"<{len(values)}d", *values)
        return self

    def string(self, s):
        b = s.encode() if isinstance(s, str) else bytes(s)
        self.u32(len(b) + 1)  # the length counts the terminating NUL
        self.out += b + b"\x00"
        return self

    def octets(self, data):
        self.u32(len(data))
        self.out += data
        return self

    def header(self, stamp, frame_id):
        return self.i32(stamp[0]).u32(stamp[1]).string(frame_id)

    def bytes(self):
        return bytes(self.out)


def pointcloud2(stamp, fields, point_step, data, width=None, height=1, frame_id="lidar", is_bigendian=0, is_dense=1):
    """``fields``: [(name, offset, datatype, count)]; ``data``: the records' bytes"""
    data = bytes(data)
    width = len(data) // point_step if width is None else width
    c = Cdr().header(stamp, frame_id).u32(height, width).u32(len(fields))
    for name, offset, datatype, count in fields:
        c.string(name).u32(offset).u8(datatype).u32(count)
    return c.u8(is_bigendian).u32(point_step, point_step * width).octets(data).u8(is_dense).bytes()


def cloud_from_struct(stamp, records, **kw):
    """A numpy structured array (packed or padded, any offsets) -> a PointCloud2 blob with one field per named column"""
    dt = records.dtype
    fields = [(name, dt.fields[name][1], DATATYPE[dt.fields[name][0].str[1:]], 1) for name in dt.names if not name.startswith("pad")]
    return pointcloud2(stamp, fields, dt.itemsize, records.tobytes(), **kw)


def data_offset(blob, data):
    """Byte offset in ``blob`` at which the PointCloud2 blob's ``data`` bytes start (they are followed by ``is_dense`` alone)"""
    return len(blob) - 1 - len(data)


def image(stamp, array, encoding, frame_id="camera", step=None):
    a = np.ascontiguousarray(array, dtype=np.uint8)
    h, w = a.shape[:2]
    row = a.reshape(h, -1)
    step = row.shape[1] if step is None else step
    rows = np.zeros((h, step), dtype=np.uint8)
    rows[:, : row.shape[1]] = row
    return Cdr().header(stamp, frame_id).u32(h, w).string(encoding).u8(0).u32(step).octets(rows.tobytes()).bytes()


def compressed_image(stamp, fmt, payload, frame_id="camera"):
    return Cdr().header(stamp, frame_id).string(fmt).octets(bytes(payload)).bytes()


def camera_info(stamp, width, height, model, D, K, R=None, P=None, frame_id="camera"):
    R = [1, 0, 0, 0, 1, 0, 0, 0, 1] if R is None else R
    P = [K[0], K[1], K[2], 0, K[3], K[4], K[5], 0, K[6], K[7], K[8], 0] if P is None else P
    c = Cdr().header(stamp, frame_id).u32(height, width).string(model).u32(len(D)).f64(*D).f64(*K).f64(*R).f64(*P)
    return c.u32(0, 0).u32(0, 0, 0, 0).u8(0).bytes()


def nanoseconds(stamp):
    return stamp[0] * 1000000000 + stamp[1]


# ---- sqlite3 storage
def write_sqlite3(path, topics, messages, schema="new"):
    """``topics``: [(id, name, type)] or [(id, name, type, serialization_format)]; ``messages``: [(topic id, timestamp [ns], payload)],
    inserted in the order given.  ``schema``: "old" (foxy: four topic columns) or "new" (iron and later: more columns, more tables)."""
    if os.path.exists(path):
        os.remove(path)
    db = sqlite3.connect(str(path))
    if schema == "old":
        db.execute("CREATE TABLE topics(id INTEGER PRIMARY KEY, name TEXT NOT NULL, type TEXT NOT NULL, serialization_format TEXT NOT NULL)")
    else:
        db.execute("CREATE TABLE schema(schema_version INTEGER PRIMARY KEY, ros_distro TEXT NOT NULL)")
        db.execute("INSERT INTO schema VALUES (4, 'jazzy')")
        db.execute("CREATE TABLE metadata(id INTEGER PRIMARY KEY, metadata_version INTEGER NOT NULL, metadata TEXT NOT NULL)")
        db.execute("CREATE TABLE topics(id INTEGER PRIMARY KEY, name TEXT NOT NULL, type TEXT NOT NULL, serialization_format TEXT NOT NULL, offered_qos_profiles TEXT NOT NULL, "
                   "type_description_hash TEXT NOT NULL)")
    db.execute("CREATE TABLE messages(id INTEGER PRIMARY KEY, topic_id INTEGER NOT NULL, timestamp INTEGER NOT NULL, data BLOB NOT NULL)")
    db.execute("CREATE INDEX timestamp_idx ON messages (timestamp ASC)")
    for t in topics:
        row = (t[0], t[1], t[2], t[3] if len(t) > 3 else "cdr")
        db.execute("INSERT INTO topics VALUES (?, ?, ?, ?)" if schema == "old" else "INSERT INTO topics VALUES (?, ?, ?, ?, '', 'RIHS01_00')", row)
    for topic_id, stamp, payload in messages:
        db.execute("INSERT INTO messages(topic_id, timestamp, data) VALUES (?, ?, ?)", (topic_id, stamp, bytes(payload)))
    db.commit()
    db.close()


def write_metadata(directory, storage, files, compression_format="", compression_mode=""):
    """``metadata.yaml`` of a bag directory (version 5 layout, the keys the reader needs and a few it does not)"""
    lines = ["rosbag2_bagfile_information:", "  version: 5", f"  storage_identifier: {storage}", "  relative_file_paths:"]
    lines += [f"    - {f}" for f in files]
    lines += ["  duration:", "    nanoseconds: 0", "  starting_time:", "    nanoseconds_since_epoch: 0", "  message_count: 0", "  topics_with_message_count: []",
              f'  compression_format: "{compression_format}"', f'  compression_mode: "{compression_mode}"']
    with open(os.path.join(directory, "metadata.yaml"), "w") as f:
        f.write("\n".join(lines) + "\n")


def write_sqlite3_dir(directory, topics, messages, split=None, **kw):
    """A bag directory of one ``.db3`` file, or of two with the messages cut at index ``split``"""
    os.makedirs(directory, exist_ok=True)
    name = os.path.basename(str(directory))
    parts = [messages] if split is None else [messages[:split], messages[split:]]
    files = [f"{name}_{k}.db3" for k in range(len(parts))]
    for f, part in zip(files, parts):
        write_sqlite3(os.path.join(directory, f), topics, part, **kw)
    write_metadata(directory, "sqlite3", files)


# ---- MCAP storage
def _str(s):
    b = s.encode()
    return struct.pack("<I", len(b)) + b


def record(op, body):
    return struct.pack("<BQ", op, len(body)) + body


def header_record(profile="ros2", library="rosbag2_fixture"):
    return record(0x01, _str(profile) + _str(library))


def footer_record(summary_start=0, summary_offset_start=0, summary_crc=0):
    return record(0x02, struct.pack("<QQI", summary_start, summary_offset_start, summary_crc))


def schema_record(schema_id, name, encoding="ros2msg", data=b"# definition"):
    return record(0x03, struct.pack("<H", schema_id) + _str(name) + _str(encoding) + struct.pack("<I", len(data)) + data)


def channel_record(channel_id, schema_id, topic, message_encoding="cdr", metadata=(("offered_qos_profiles", ""),)):
    meta = b"".join(_str(k) + _str(v) for k, v in metadata)
    return record(0x04, struct.pack("<HH", channel_id, schema_id) + _str(topic) + _str(message_encoding) + struct.pack("<I", len(meta)) + meta)


def message_record(channel_id, sequence, log_time, payload, publish_time=None):
    return record(0x05, struct.pack("<HIQQ", channel_id, sequence, log_time, log_time if publish_time is None else publish_time) + bytes(payload))


def chunk_record(records, start=0, end=0, compression="", stored=None, crc=None, size=None):
    """``stored``: the chunk's bytes for a compression this module does not write itself; ``crc`` = None: the right one"""
    crc = zlib.crc32(records) if crc is None else crc
    data = records if stored is None else stored
    return record(0x06, struct.pack("<QQQI", start, end, len(records) if size is None else size, crc) + _str(compression) + struct.pack("<Q", len(data)) + data)


def message_index_record(channel_id, entries):
    body = b"".join(struct.pack("<QQ", t, off) for t, off in entries)
    return record(0x07, struct.pack("<H", channel_id) + struct.pack("<I", len(body)) + body)


def data_end_record(crc=0):
    return record(0x0F, struct.pack("<I", crc))


def write_mcap(path, channels, messages, chunk_size=None, summary=False, unknown=False):
    """``channels``: [(channel id, topic, type)] or [(channel id, topic, type, message_encoding)]; ``messages``: [(channel id, log_time [ns],
    payload)] in the FILE order wanted.  ``chunk_size`` = None writes schema, channel and message records at the top level; else chunks
    of that many messages, each preceded inside its chunk by the schema and channel records it uses for the first time.  ``summary=True``
    adds message-index records after every chunk, and a summary section (schemas, channels, statistics, a summary offset) between
    DataEnd and the footer.  ``unknown=True`` sprinkles records with opcodes the specification does not define (0x80, 0xFE).
    Returns the byte offsets at which a top-level record starts, the footer's and the closing magic's included."""
    out, bounds = bytearray(MCAP_MAGIC), []
    schema_of = {}
    for c in channels:
        schema_of.setdefault(c[2], len(schema_of) + 1)

    def add(rec):
        bounds.append(len(out))
        out.extend(rec)

    def definitions(c):
        return schema_record(schema_of[c[2]], c[2]) + channel_record(c[0], schema_of[c[2]], c[1], c[3] if len(c) > 3 else "cdr")

    add(header_record())
    by_id = {c[0]: c for c in channels}
    if chunk_size is None:
        for c in channels:
            add(schema_record(schema_of[c[2]], c[2]))
            add(channel_record(c[0], schema_of[c[2]], c[1], c[3] if len(c) > 3 else "cdr"))
        for k, (cid, t, payload) in enumerate(messages):
            if unknown and k % 2 == 0:
                add(record(0x80, b"private record"))
            add(message_record(cid, k, t, payload))
    else:
        seen = set()
        for s in range(0, len(messages), chunk_size):
            inner, entries = b"", {}
            for k, (cid, t, payload) in enumerate(messages[s : s + chunk_size]):
                if cid not in seen:
                    seen.add(cid)
                    inner += definitions(by_id[cid])
                if unknown:
                    inner += record(0xFE, b"")
                entries.setdefault(cid, []).append((t, len(inner)))
                inner += message_record(cid, s + k, t, payload)
            times = [t for e in entries.values() for t, _ in e]
            add(chunk_record(inner, min(times), max(times)))
            if summary:
                for cid, e in entries.items():
                    add(message_index_record(cid, e))
            if unknown:
                add(record(0x80, b"private record"))
    add(data_end_record())
    summary_start = 0
    if summary:
        summary_start = len(out)
        for c in channels:
            add(schema_record(schema_of[c[2]], c[2]))
            add(channel_record(c[0], schema_of[c[2]], c[1], c[3] if len(c) > 3 else "cdr"))
        counts = b"".join(struct.pack("<HQ", c[0], sum(1 for m in messages if m[0] == c[0])) for c in channels)
        times = [m[1] for m in messages] or [0]
        add(record(0x0B, struct.pack("<QHIIIIQQ", len(messages), len(schema_of), len(channels), 0, 0, 0, min(times), max(times)) + struct.pack("<I", len(counts)) + counts))
        add(record(0x0E, struct.pack("<BQQ", 0x03, summary_start, 1)))
    add(footer_record(summary_start))
    bounds.append(len(out))
    out.extend(MCAP_MAGIC)
    with open(path, "wb") as f:
        f.write(bytes(out))
    return bounds
