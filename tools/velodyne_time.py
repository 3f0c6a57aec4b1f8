#!/usr/bin/env python3
"""Times the Velodyne packet decode (nidreg_velodyne_decode) on one 76-packet VLP-16 message -- one turn at 10 Hz, 92 KB of packets,
29 184 records --, split into allocation + upload, kernel and copy back (nidreg_velodyne_get_timing: the host clock around each phase of
the synchronous call), against the numpy restatement of tests/velodyne_oracle.py on one host core with the same bytes; checks that both
give the same records bit for bit.  A frame this small costs its launches and copies, not bandwidth: the kernel column is launch to
idle.  Writes profiles/velodyne.json (--out), stamped with nidreg_kernel_build().  The rules are unpinned against velodyne_pointcloud
and real recordings, so there is no driver column.  A plain script, not part of the test or bench contract.

    python tools/velodyne_time.py [--calls 20] [--warmup 3] [--out profiles/velodyne.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from direct_visual_lidar_calibration_amd import _lib, lidar_messages  # noqa: E402

import velodyne_oracle as vo  # noqa: E402

PACKETS, STRIDE = 76, 1214


def make_message():
    """76 packets, 40 centidegrees a block (0.2 degrees a firing: 600 rpm), every return present, 1.33 ms apart, as they lie in a ROS1 message"""
    rng = np.random.default_rng(76)
    packets = [vo.encode_packet([((p * 12 + b) * 40) % 36000 for b in range(12)], rng.integers(500, 50000, (12, 32)), rng.integers(0, 256, (12, 32))) for p in range(PACKETS)]
    _, view = vo.place_packets(packets, STRIDE, lead=1)
    return view, np.arange(PACKETS) * 1.327e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "velodyne.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("velodyne_time: no GPU; there is nothing to measure without one")
    lib = _lib.load()
    view, times = make_message()
    model = lidar_messages.builtin_model("vlp16")
    phases, wall = [], []
    for k in range(args.warmup + args.calls):
        t0 = time.perf_counter()
        got = lidar_messages.velodyne_decode(view, PACKETS, STRIDE, times, model)
        dt = time.perf_counter() - t0
        ms = (ctypes.c_double * 3)()
        lib.nidreg_velodyne_get_timing(ms)
        if k >= args.warmup:
            phases.append(list(ms))
            wall.append(dt * 1e3)
    host = []
    for k in range(args.warmup + args.calls):
        t0 = time.perf_counter()
        want, _ = vo.decode(view, STRIDE, times, model.table, model.distance_resolution, model.firing_period, model.laser_period)
        if k >= args.warmup:
            host.append((time.perf_counter() - t0) * 1e3)
    med = np.median(np.asarray(phases), axis=0)
    result = {"kernel_build": _lib.library_kernel_build(), "device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup,
              "clock": "host clock; the phases are nidreg_velodyne_get_timing of each synchronous call, medians over the calls; total_ms is the Python call, which also allocates the "
                       "record array; the host column is the numpy restatement on one core, median over the same number of calls",
              "reference": "tests/velodyne_oracle.py; unpinned against velodyne_pointcloud and real recordings",
              "note": "measured once, nothing tuned; 76 packets are 76 workgroups of 384 threads: the call costs its launch, copies and allocations, not bandwidth",
              "packets": PACKETS, "packet_stride": STRIDE, "source_bytes": int((PACKETS - 1) * STRIDE + 1206), "records": int(got.shape[0]), "record_bytes": int(got.nbytes),
              "total_ms_median": float(np.median(wall)), "total_ms_min": float(np.min(wall)), "total_ms_max": float(np.max(wall)), "alloc_upload_ms": float(med[0]), "kernel_ms": float(med[1]),
              "copy_back_ms": float(med[2]), "host_numpy_one_core_ms_median": float(np.median(host)),
              "same_as_host_numpy": bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))}
    if not result["same_as_host_numpy"]:
        raise SystemExit(f"velodyne_time: the device's records differ from the numpy restatement: {result}")
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
