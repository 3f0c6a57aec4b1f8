"""Ouster lidar packet, PacketMsg and metadata WRITERS (test infrastructure, not a test): the three packet profiles with explicit
``struct.pack`` calls in the order the sensor's manual lists the fields, ``ouster_ros/PacketMsg`` ROS1-serialised and in CDR, ``std_msgs/String``,
the metadata JSON in the flat shape of firmware 2 and the grouped shape of firmware 3, and a scene-to-packets generator.  They share no
code with direct_visual_lidar_calibration_amd/lidar_messages.py, the kernel or tests/ouster_oracle.py."""
import json
import struct

import numpy as np

import rosbag1_fixture as fx1
import rosbag2_fixture as fx2

LEGACY, RNG19, RNG15 = "LEGACY", "RNG19_RFL8_SIG16_NIR16", "RNG15_RFL8_NIR8"
PACKET1, PACKET2, PACKET2_SENSOR = "ouster_ros/PacketMsg", "ouster_msgs/msg/PacketMsg", "ouster_sensor_msgs/msg/PacketMsg"
STRING1, STRING2 = "std_msgs/String", "std_msgs/msg/String"
OS1_TRANSFORM = [-1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 36.18, 0.0, 0.0, 0.0, 1.0]
VALID = {LEGACY: 0xFFFFFFFF, RNG19: 1, RNG15: 1}  # the status of a valid column


class Column:
    """One column: ``timestamp`` [ns], ``measurement_id``, ``status`` (LEGACY: the trailing uint32; else the header's uint16) and per
    pixel the RAW fields as the packet holds them -- ``range`` the whole uint32 (RNG15: uint16) with the bits above the mask, ``reflectivity``,
    ``signal``, ``near_ir``.  ``unused``: the byte written where the layout has none of these."""

    def __init__(self, timestamp, measurement_id, status, range_, reflectivity, signal, near_ir, unused=0, encoder=0):
        self.timestamp, self.measurement_id, self.status, self.unused, self.encoder = int(timestamp), int(measurement_id), int(status), int(unused), int(encoder)
        self.range, self.reflectivity, self.signal, self.near_ir = ([int(v) for v in a] for a in (range_, reflectivity, signal, near_ir))


def encode_packet(profile, columns, frame_id, unused=0):
    """The bytes of one lidar packet of ``len(columns)`` columns"""
    out = bytearray()
    if profile != LEGACY:  # packet header: packet_type, frame_id, init_id (3 bytes), serial number (5 bytes), 20 reserved
        out += struct.pack("<HH", 1, frame_id) + bytes([unused]) * 28
    for col in columns:
        if profile == LEGACY:
            out += struct.pack("<QHHI", col.timestamp, col.measurement_id, frame_id, col.encoder)
            for r, f, s, n in zip(col.range, col.reflectivity, col.signal, col.near_ir):
                out += struct.pack("<IHHH", r, f, s, n) + bytes([col.unused]) * 2
            out += struct.pack("<I", col.status)
        else:
            out += struct.pack("<QHH", col.timestamp, col.measurement_id, col.status)
            for r, f, s, n in zip(col.range, col.reflectivity, col.signal, col.near_ir):
                if profile == RNG19:
                    out += struct.pack("<IBBHH", r, f, col.unused, s, n) + bytes([col.unused]) * 2
                else:
                    out += struct.pack("<HBB", r, f, n)
    if profile != LEGACY:
        out += bytes([unused]) * 32  # footer
    return bytes(out)


def place_packets(packets, stride, lead=0):
    """The packets ``stride`` bytes apart in one uint8 array, starting ``lead`` bytes into it; the gaps hold 0xA5.  Returns
    ``(array, view)``: ``view`` starts at the first packet."""
    size = len(packets[0]) if packets else 0
    buf = np.full(lead + stride * len(packets), 0xA5, dtype=np.uint8)
    for k, p in enumerate(packets):
        buf[lead + k * stride : lead + k * stride + size] = np.frombuffer(p, dtype=np.uint8)
    return buf, buf[lead:]


# ---- messages
def packet_msg_ros1(buf):
    return struct.pack("<I", len(buf)) + bytes(buf)


def packet_msg_cdr(buf):
    return fx2.Cdr().octets(bytes(buf)).bytes()


def string_ros1(s):
    return fx1._string(s)


def string_cdr(s):
    return fx2.Cdr().string(s).bytes()


# ---- metadata
def metadata(profile, H, W, C, altitude, azimuth, n_mm=15.806, transform=OS1_TRANSFORM, shape="flat"):
    """The sensor's metadata JSON.  ``shape``: ``flat`` (firmware 2: every key at the top level; LEGACY leaves ``udp_profile_lidar`` out) or
    ``nested`` (firmware 3: the groups beam_intrinsics, lidar_data_format, lidar_intrinsics, config_params)"""
    if shape == "flat":
        doc = {"prod_line": f"OS-1-{H}", "lidar_mode": f"{W}x10", "beam_altitude_angles": list(altitude), "beam_azimuth_angles": list(azimuth),
               "lidar_origin_to_beam_origin_mm": n_mm, "lidar_to_sensor_transform": list(transform), "pixels_per_column": H, "columns_per_frame": W, "columns_per_packet": C,
               "imu_to_sensor_transform": [1, 0, 0, 6.253, 0, 1, 0, -11.775, 0, 0, 1, 7.645, 0, 0, 0, 1]}
        if profile != LEGACY:
            doc["udp_profile_lidar"] = profile
    else:
        doc = {"sensor_info": {"prod_line": f"OS-1-{H}", "build_rev": "v3.0.1"},
               "beam_intrinsics": {"beam_altitude_angles": list(altitude), "beam_azimuth_angles": list(azimuth), "lidar_origin_to_beam_origin_mm": n_mm,
                                   "beam_to_lidar_transform": [1, 0, 0, n_mm, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]},
               "lidar_data_format": {"pixels_per_column": H, "columns_per_frame": W, "columns_per_packet": C, "udp_profile_lidar": profile, "udp_profile_imu": "LEGACY",
                                     "pixel_shift_by_row": [0] * H, "column_window": [0, W - 1]},
               "lidar_intrinsics": {"lidar_to_sensor_transform": list(transform)},
               "config_params": {"lidar_mode": f"{W}x10", "udp_profile_lidar": profile, "udp_port_lidar": 7502}}
    return json.dumps(doc)


def os_angles(H, spread=22.5):
    """(altitude, azimuth) [deg] of a sensor of H beams: the altitudes evenly from +spread to -spread, the azimuths the staggered four-value pattern"""
    altitude = [spread - 2.0 * spread * i / (H - 1) for i in range(H)]
    azimuth = [(4.23, 1.41, -1.4, -4.21)[i % 4] for i in range(H)]
    return altitude, azimuth


# ---- scene to packets
def beam_directions(m, W, altitude, azimuth):
    """Unit directions (H, 3) of the beams of column ``m`` in the lidar frame"""
    theta = 2.0 * np.pi * (1.0 - m / W) - np.radians(np.asarray(azimuth))
    phi = np.radians(np.asarray(altitude))
    return np.stack([np.cos(theta) * np.cos(phi), np.sin(theta) * np.cos(phi), np.sin(phi)], axis=1)


def scan_packets(profile, H, W, C, frame_id, t0_ns, column_ns, range_mm, first_column=0, last_column=None, lost=()):
    """One turn as packets of C columns: column ``m`` is measured at ``t0_ns + m * column_ns``; ``range_mm(m, t_ns)`` gives its H ranges [mm];
    the other channels follow a formula of (m, pixel).  ``lost``: (m, pixel) pairs without a return (range 0).  Columns outside
    ``[first_column, last_column)`` are not sent (whole packets only)."""
    last_column = W if last_column is None else last_column
    packets = []
    for m0 in range(first_column, last_column, C):
        cols = []
        for m in range(m0, m0 + C):
            t = t0_ns + m * column_ns
            r = np.asarray(range_mm(m, t)).astype(np.int64)
            r = np.clip(r, 1, 0x7FFF << 3 if profile == RNG15 else 0x7FFFF)
            i = np.arange(H)
            refl = (40 + 3 * i + (m % 50)) % 256
            sig = (100 + 17 * i + 5 * m) % 4000 if profile != RNG15 else 0 * i
            nir = (300 + 7 * i + m) % 4096
            for mm, ii in lost:
                if mm == m:
                    r[ii] = 0
            if profile == RNG15:
                cols.append(Column(t, m, VALID[profile], r >> 3, refl, sig, nir >> 4))
            else:
                cols.append(Column(t, m, VALID[profile], r, refl, sig, nir))
        packets.append(encode_packet(profile, cols, frame_id))
    return packets
