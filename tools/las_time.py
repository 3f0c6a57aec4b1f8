#!/usr/bin/env python3
"""Times the LAS map route on one 10M-point format-3 file (34-byte records, 340 MB) at 2 mm: the file read (np.fromfile of one
chunk), then nidreg_integrator_insert_las split into upload, decode kernel and the integrator's passes (nidreg_integrator_las_timing:
the host clock around each phase of the synchronous call), against the numpy restatement of tests/las_oracle.py on one host core
followed by insert_points of its doubles; checks that both integrators hold the same records bit for bit.  The file is georeferenced
(offsets near 5e5 / 4e6) and recentred on the way in.  Writes profiles/las.json (--out), stamped with nidreg_kernel_build().  The
format is read from its public description, unpinned against laspy / PDAL and real files, so there is no column for either.  A plain
script, not part of the test or bench contract.

    python tools/las_time.py [--points 10000000] [--calls 3] [--out profiles/las.json]
"""
import argparse
import ctypes
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

from direct_visual_lidar_calibration_amd import _lib, dataset, preprocess  # noqa: E402

import las_oracle as lo  # noqa: E402

RES = 0.002
SCALE, OFFSET, ORIGIN = (0.001, 0.001, 0.001), (500000.37, 4000000.91, 123.456), (500000.0, 4000000.0, 100.0)


def make_file(path, n):
    """n points on the walls of a 60 m x 40 m x 12 m hall, millimetre integers, 16-bit intensity and colour"""
    rng = np.random.default_rng(34)
    X, Y, Z = rng.integers(-30000, 30000, n), rng.integers(-20000, 20000, n), rng.integers(-2000, 10000, n)
    wall = rng.integers(0, 3, n)
    X[wall == 0], Y[wall == 1], Z[wall == 2] = 30000, 20000, -2000
    rec = lo.pack_records(3, X, Y, Z, rng.integers(0, 65536, n), rng.integers(0, 20, n), rng.random(n) < 0.01, rng.integers(0, 65536, (n, 3)), 0, rng)
    lo.write_las(path, 3, rec, SCALE, OFFSET, minor=2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "las.json"))
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("las_time: no GPU; there is nothing to measure without one")
    lib = _lib.load()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "hall.las")
        rec = make_file(path, args.points)
        header = dataset.read_las_header(path)
        rows = []
        got = None
        for _ in range(args.calls + 1):  # the first call also allocates the buffers and grows the table: left out
            integ = preprocess.StaticPointCloudIntegrator(RES, 0.0)
            try:
                t0 = time.perf_counter()
                (raw,) = list(dataset.read_las_chunks(path, header, args.points))
                t1 = time.perf_counter()
                skipped = integ.insert_las(raw, header["record_length"], header["point_format"], header["scale"], header["offset"], ORIGIN, "intensity", (7, 18), False)
                t2 = time.perf_counter()
                ms = (ctypes.c_double * 3)()
                lib.nidreg_integrator_las_timing(ms)
                rows.append([(t1 - t0) * 1e3, ms[0], ms[1], ms[2], (t2 - t1) * 1e3])
                if got is None:
                    got = (skipped, integ.get_records(), integ.last_seq)
            finally:
                integ.close()
        host = []
        want = None
        for _ in range(2):
            integ = preprocess.StaticPointCloudIntegrator(RES, 0.0)
            try:
                t0 = time.perf_counter()
                xyz, inten, keep = lo.decode(rec, 3, SCALE, OFFSET, ORIGIN, exclude_classes=(7, 18))
                t1 = time.perf_counter()
                integ.insert_points(xyz[keep], inten[keep])
                t2 = time.perf_counter()
                host.append([(t1 - t0) * 1e3, (t2 - t1) * 1e3])
                if want is None:
                    want = (int((~keep).sum()), integ.get_records(), np.flatnonzero(keep)[integ.last_seq])
            finally:
                integ.close()
    med = np.median(np.asarray(rows[1:]), axis=0)
    hmed = np.min(np.asarray(host), axis=0)
    same = bool(got[0] == want[0] and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)) and np.array_equal(got[2], want[2]))
    result = {"kernel_build": _lib.library_kernel_build(), "device": torch.cuda.get_device_name(0), "calls": args.calls,
              "clock": "host clock; file_read_ms is np.fromfile of the one chunk (page cache warm: the file was just written); upload / decode / insert are "
                       "nidreg_integrator_las_timing of the synchronous call, medians over the calls after the first; the host column is the numpy restatement "
                       "on one core (the faster of two runs) followed by insert_points of its filtered doubles",
              "reference": "tests/las_oracle.py; unpinned against laspy / PDAL and real files",
              "note": "measured once, nothing tuned",
              "points": args.points, "point_format": 3, "record_length": 34, "file_bytes": int(header["file_size"]), "voxel_resolution": RES, "skipped": int(got[0]), "voxels": int(got[1].shape[0]),
              "file_read_ms": float(med[0]), "upload_ms": float(med[1]), "decode_kernel_ms": float(med[2]), "insert_ms": float(med[3]), "insert_las_call_ms": float(med[4]),
              "host_numpy_decode_ms": float(hmed[0]), "host_insert_points_ms": float(hmed[1]), "same_records_as_host_numpy": same}
    if not same:
        raise SystemExit(f"las_time: the device's records differ from the numpy restatement: {result}")
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
