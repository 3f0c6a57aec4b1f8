"""Message packers for velodyne_msgs/VelodyneScan and livox_ros_driver(2)/CustomMsg, ROS1-serialised and in CDR (test infrastructure,
not a test), written with explicit ``struct.pack`` calls in the order the message definitions list their fields, on top of
tests/rosbag1_fixture.py and tests/rosbag2_fixture.py.  They share no code with direct_visual_lidar_calibration_amd/lidar_messages.py
-- the reader under test."""
import struct

import numpy as np

import rosbag1_fixture as fx1
import rosbag2_fixture as fx2

SCAN1, SCAN2 = "velodyne_msgs/VelodyneScan", "velodyne_msgs/msg/VelodyneScan"
LIVOX1, LIVOX1_V2, LIVOX2 = "livox_ros_driver/CustomMsg", "livox_ros_driver2/CustomMsg", "livox_ros_driver2/msg/CustomMsg"
# the 19 bytes of a livox CustomPoint
CUSTOM_POINT = np.dtype({"names": ["t", "x", "y", "z", "reflectivity", "tag", "line"], "formats": ["<u4", "<f4", "<f4", "<f4", "u1", "u1", "u1"], "offsets": [0, 4, 8, 12, 16, 17, 18],
                         "itemsize": 19})


def velodyne_scan_ros1(stamp, packets, frame_id="velodyne", seq=0):
    """``packets``: [((sec, nsec), 1206 bytes)]"""
    out = fx1._header(seq, stamp, frame_id) + struct.pack("<I", len(packets))
    for t, data in packets:
        assert len(data) == 1206
        out += struct.pack("<II", *t) + bytes(data)
    return out


def velodyne_scan_cdr(stamp, packets, frame_id="velodyne", final_padding=False):
    c = fx2.Cdr().header(stamp, frame_id).u32(len(packets))
    for t, data in packets:
        assert len(data) == 1206
        c.i32(t[0]).u32(t[1])
        c.out += bytes(data)
    if final_padding:
        c.pad(4)
    return c.bytes()


def custom_msg_ros1(stamp, points, frame_id="livox_frame", seq=0, timebase=0, lidar_id=0):
    """``points``: a CUSTOM_POINT array"""
    assert points.dtype == CUSTOM_POINT
    return (fx1._header(seq, stamp, frame_id) + struct.pack("<QIB3B", timebase, len(points), lidar_id, 0, 0, 0) + struct.pack("<I", len(points)) + points.tobytes())


def custom_msg_cdr(stamp, points, frame_id="livox_frame", timebase=0, lidar_id=0, final_padding=True):
    assert points.dtype == CUSTOM_POINT
    c = fx2.Cdr().header(stamp, frame_id)
    c.pad(8)
    c.out += struct.pack("<Q", timebase)
    c.u32(len(points)).u8(lidar_id).u8(0).u8(0).u8(0).u32(len(points))
    for k in range(len(points)):
        c.pad(4)
        c.out += points[k : k + 1].tobytes()
    if final_padding and len(points):
        c.pad(4)
    return c.bytes()
