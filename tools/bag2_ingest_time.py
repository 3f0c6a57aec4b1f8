#!/usr/bin/env python3
"""Times the ingest of one bag's PointCloud2 frames as preprocess_ros2 runs it -- open the bag, then ``integrate_bag`` into a fresh static
integrator -- against the same frames as a ROS1 bag through preprocess_ros1, in one process.  The frames have the shape
tools/bag_ingest_time.py uses (an Ouster: --points 131072 records of 48 bytes, 2 mm voxels, min_distance 1 m; its ``make_frame``), --frames
of them, written uncompressed three ways by the tests' fixture writers into a temporary directory:

    ros1      a ROS1 bag (one frame per chunk)        rosbag1.Bag reads the file into memory
    sqlite3   a bare .db3                             rosbag2.Bag: a read-only cursor, one BLOB at a time
    mcap      a bare .mcap (one frame per chunk)      rosbag2.Bag: the file mapped, the records uploaded from the mapping

The files were just written, so they come from the page cache: this is the cost of the Python reader and of the device, not of a disk.
A run is timed by the host clock in two parts: ``open`` (the constructor: for ROS1 and MCAP the scan of the whole file) and ``integrate``
(every insert ends in a device-to-host read, so the clock stops after the device has finished).  The routes alternate, --warmup runs of each
first, then --runs timed ones; the medians go to profiles/preprocess_ros2.json (--out), stamped with nidreg_kernel_build().  The last runs'
records are compared bit for bit.  Measured once, nothing tuned; a plain script, not part of the test or bench contract.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import rosbag1_fixture as fx1  # noqa: E402  (test infrastructure: the bag writers)
import rosbag2_fixture as fx2  # noqa: E402
from bag_ingest_time import CHANNEL, FIELDS, make_frame  # noqa: E402
from direct_visual_lidar_calibration_amd import _lib, preprocess, preprocess_ros1, preprocess_ros2, rosbag1, rosbag2  # noqa: E402

TOPIC = "/os_cloud_node/points"


def write_bags(directory, frames):
    stamps = [(100 + k // 10, (k % 10) * 100000000) for k in range(len(frames))]
    paths = {"ros1": os.path.join(directory, "run.bag"), "sqlite3": os.path.join(directory, "run.db3"), "mcap": os.path.join(directory, "run.mcap")}
    fx1.write_bag(paths["ros1"], [(0, TOPIC, "sensor_msgs/PointCloud2")], [(0, s, fx1.pointcloud2(s, FIELDS, 48, f)) for s, f in zip(stamps, frames)], chunk_size=1)
    fx2.write_sqlite3(paths["sqlite3"], [(1, TOPIC, fx2.PC2)], [(1, fx2.nanoseconds(s), fx2.pointcloud2(s, FIELDS, 48, f)) for s, f in zip(stamps, frames)])
    fx2.write_mcap(paths["mcap"], [(1, TOPIC, fx2.PC2)], [(1, fx2.nanoseconds(s), fx2.pointcloud2(s, FIELDS, 48, f)) for s, f in zip(stamps, frames)], chunk_size=1)
    return paths


def run_route(path, reader, args):
    integ = preprocess.StaticPointCloudIntegrator(args.voxel_resolution, args.min_distance, device=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bag = reader.Bag(path)
    t1 = time.perf_counter()
    inserted, rewound, skipped = preprocess_ros1.integrate_bag(args, bag, TOPIC, CHANNEL, integ, warn=lambda m: None, reader=reader)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, integ, (inserted, rewound, skipped)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_ros2.json"), help="'none' = print only")
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bag2_ingest_time: no GPU; there is nothing to measure without one")
    build = _lib.library_kernel_build()
    args = preprocess_ros2.build_parser().parse_args(["src", "dst"])  # the command's defaults: 2 mm voxels, min_distance 1 m
    frames = [make_frame(opts.points, k) for k in range(opts.frames)]
    n = len(frames[0]) // 48
    readers = {"ros1": rosbag1, "sqlite3": rosbag2, "mcap": rosbag2}
    times, last, meta = {r: [] for r in readers}, {}, {}
    with tempfile.TemporaryDirectory() as directory:
        paths = write_bags(directory, frames)
        sizes = {r: os.path.getsize(p) for r, p in paths.items()}
        print(f"{len(frames)} frames x {n} points written: {sizes}", flush=True)
        for k in range(opts.warmup + opts.runs):
            for r, reader in readers.items():  # alternating
                open_s, integrate_s, integ, counts = run_route(paths[r], reader, args)
                if k == opts.warmup + opts.runs - 1:
                    last[r] = integ.get_records()
                meta[r] = {"frames_inserted": counts[0], "frames_skipped": counts[1], "skipped_points": counts[2], "voxels": integ.info()["voxels"], "file_bytes": sizes[r]}
                integ.close()
                if k >= opts.warmup:
                    times[r].append((open_s, integrate_s))
                print(json.dumps({"run": k, "route": r, "open_seconds": open_s, "integrate_seconds": integrate_s, "warmup": k < opts.warmup}), flush=True)
    result = {"kernel_build": build, "device": torch.cuda.get_device_name(0), "frames": len(frames), "points_per_frame": n, "point_step": 48, "intensity_channel": CHANNEL,
              "voxel_resolution": args.voxel_resolution, "min_distance": args.min_distance, "runs": opts.runs, "warmup": opts.warmup,
              "clock": "host clock; open = the Bag constructor, integrate = integrate_bag into a fresh static integrator (every insert ends in a device-to-host read); "
                       "files from the page cache; measured once, nothing tuned"}
    for r in readers:
        o, i = np.median([t[0] for t in times[r]]), np.median([t[1] for t in times[r]])
        result[r] = dict(meta[r], open_seconds_median=float(o), integrate_seconds_median=float(i), seconds_median=float(np.median([t[0] + t[1] for t in times[r]])),
                         ms_per_frame=float(1e3 * np.median([t[0] + t[1] for t in times[r]]) / len(frames)))
    result["same_records"] = bool(all(np.array_equal(last["ros1"].view(np.uint32), last[r].view(np.uint32)) for r in ("sqlite3", "mcap")))
    if not result["same_records"]:
        raise SystemExit("bag2_ingest_time: the routes' records differ")
    print(json.dumps(result), flush=True)
    if opts.out != "none":
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print("wrote", opts.out)


if __name__ == "__main__":
    main()
