#!/usr/bin/env python3
"""Times the Ouster packet decode (nidreg_ouster_decode) on one 1024 x 64 RNG19_RFL8_SIG16_NIR16 scan -- 64 packets of 16 columns, 784 KB
of packets, 65 536 records of 32 bytes --, split into allocation + upload, kernel and copy back (nidreg_ouster_get_timing: the host clock
around each phase of the synchronous call), against the numpy restatement of tests/ouster_oracle.py on one host core with the same bytes;
checks that both give the same records bit for bit.  A scan this small costs its launches and copies, not bandwidth: the kernel column
is launch to idle.  Writes profiles/ouster.json (--out), stamped with nidreg_kernel_build().  The layouts are unpinned against ouster_ros,
the Ouster SDK and real recordings, so there is no driver column.  A plain script, not part of the test or bench contract.

    python tools/ouster_time.py [--calls 20] [--warmup 3] [--out profiles/ouster.json]
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

import ouster_fixture as ofx  # noqa: E402
import ouster_oracle as oo  # noqa: E402

PROFILE, H, W, C = ofx.RNG19, 64, 1024, 16
COLUMN_NS = 97656  # 10 Hz


def make_scan():
    """One full turn, every return present, as the batcher lays it out: 64 packets, stride = packet size"""
    rng = np.random.default_rng(64)
    packets = ofx.scan_packets(PROFILE, H, W, C, 1, 10**15, COLUMN_NS, lambda m, t: rng.integers(500, 120000, H))
    return np.frombuffer(b"".join(packets), dtype=np.uint8), len(packets)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ouster.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ouster_time: no GPU; there is nothing to measure without one")
    lib = _lib.load()
    view, n = make_scan()
    altitude, azimuth = ofx.os_angles(H)
    info = lidar_messages.ouster_info(ofx.metadata(PROFILE, H, W, C, altitude, azimuth))
    ts0 = oo.first_valid_timestamp(view, info.packet_size, n, PROFILE, H, C)
    phases, wall = [], []
    for k in range(args.warmup + args.calls):
        t0 = time.perf_counter()
        got = lidar_messages.ouster_decode(view, n, info.packet_size, info, ts0)
        dt = time.perf_counter() - t0
        ms = (ctypes.c_double * 3)()
        lib.nidreg_ouster_get_timing(ms)
        if k >= args.warmup:
            phases.append(list(ms))
            wall.append(dt * 1e3)
    host = []
    for k in range(args.warmup + args.calls):
        t0 = time.perf_counter()
        want, _ = oo.decode(view, info.packet_size, n, PROFILE, H, W, C, info.column_table, info.beam_table, info.n_mm, info.transform12, ts0)
        if k >= args.warmup:
            host.append((time.perf_counter() - t0) * 1e3)
    med = np.median(np.asarray(phases), axis=0)
    result = {"kernel_build": _lib.library_kernel_build(), "device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup,
              "clock": "host clock; the phases are nidreg_ouster_get_timing of each synchronous call, medians over the calls; total_ms is the Python call, which also allocates the "
                       "record array; the host column is the numpy restatement on one core, median over the same number of calls",
              "reference": "tests/ouster_oracle.py; unpinned against ouster_ros, the Ouster SDK and real recordings",
              "note": "measured once, nothing tuned; 64 packets x 16 columns are 1024 workgroups of 128 threads: the call costs its launch, copies and allocations, not bandwidth",
              "profile": PROFILE, "pixels_per_column": H, "columns_per_frame": W, "columns_per_packet": C, "packets": n, "packet_stride": int(info.packet_size),
              "source_bytes": int(view.size), "records": int(got.shape[0]), "record_bytes": int(got.nbytes),
              "total_ms_median": float(np.median(wall)), "total_ms_min": float(np.min(wall)), "total_ms_max": float(np.max(wall)), "alloc_upload_ms": float(med[0]), "kernel_ms": float(med[1]),
              "copy_back_ms": float(med[2]), "host_numpy_one_core_ms_median": float(np.median(host)),
              "same_as_host_numpy": bool(np.array_equal(got, oo.as_words(want)))}
    if not result["same_as_host_numpy"]:
        raise SystemExit(f"ouster_time: the device's records differ from the numpy restatement: {result}")
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
