#!/usr/bin/env python3
"""Cloud ingest on one GPU at configs[1] size (10M points, 16 B float32 records x y z intensity, the record preprocess.cpp:161-169
writes): wall time of nidreg_cloud_create on the host-widened doubles (40 B/point over PCIe) against nidreg_cloud_create_f32 on
the records (16 B/point, widened on the GPU), and the host load of a 10M-point PLY file through dataset.read_ply (widening pass)
against dataset.read_ply_float32 (views over one read of the vertex block).  Medians of 5 after one warm-up each.  Writes
profiles/ingest_f32.json (or argv[1]) stamped with nidreg_kernel_build().

    python tools/ingest_timing.py [out.json] [points]
"""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from direct_visual_lidar_calibration_amd import _lib, dataset, nid  # noqa: E402

REPEATS = 5


def timed(fn, repeats=REPEATS, after=None):
    """median wall time of fn(); `after` (untimed) receives what fn returned"""
    r = fn()  # warm-up: code-object load, first-touch of the device allocator
    if after:
        after(r)
    walls = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = fn()
        walls.append(time.perf_counter() - t0)
        if after:
            after(r)
    return statistics.median(walls), walls


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ingest_f32.json")
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
    stamp = _lib.stamp_or_refuse()
    rng = np.random.default_rng(1)
    rec = np.empty(n, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")])
    for k in ("x", "y", "z"):
        rec[k] = rng.uniform(-50.0, 50.0, n)
    rec["intensity"] = rng.random(n)
    xyz = np.ndarray((n, 3), dtype="<f4", buffer=rec, offset=0, strides=(16, 4))
    inten = np.ndarray((n,), dtype="<f4", buffer=rec, offset=12, strides=(16,))
    pts = np.ones((n, 4))
    pts[:, :3] = xyz
    ints = inten.astype(np.float64)

    # the create call alone (its allocations, copies and, for f32, the widening kernel and the staging free); destroy untimed
    up64, up64_all = timed(lambda: nid.Cloud(pts, ints), after=lambda c: c.close())
    up32, up32_all = timed(lambda: nid.Cloud.from_float32(xyz, inten), after=lambda c: c.close())

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cloud.ply")
        with open(path, "wb") as f:
            f.write(f"ply\nformat binary_little_endian 1.0\nelement vertex {n}\nproperty float x\nproperty float y\nproperty float z\nproperty float intensity\nend_header\n".encode())
            f.write(rec.tobytes())
        file_bytes = os.path.getsize(path)
        ld64, ld64_all = timed(lambda: dataset.read_ply(path))
        ld32, ld32_all = timed(lambda: dataset.read_ply_float32(path))
        raw, raw_all = timed(lambda: open(path, "rb").read())

    res = {
        "tool": "tools/ingest_timing.py",
        "kernel_build": stamp,
        "workload": {"points": n, "record_bytes": 16, "repeats": REPEATS, "statistic": "median after one warm-up"},
        "upload": {
            "nidreg_cloud_create_ms": round(up64 * 1e3, 3),
            "nidreg_cloud_create_f32_ms": round(up32 * 1e3, 3),
            "speedup": round(up64 / up32, 3),
            "bytes_f64_route": 40 * n,
            "bytes_f32_route": 16 * n,
            "all_ms": {"f64": [round(w * 1e3, 3) for w in up64_all], "f32": [round(w * 1e3, 3) for w in up32_all]},
        },
        "host_load": {
            "file_bytes": file_bytes,
            "read_ply_s": round(ld64, 4),
            "read_ply_float32_s": round(ld32, 4),
            "raw_read_s": round(raw, 4),
            "speedup": round(ld64 / ld32, 2),
            "all_s": {"read_ply": [round(w, 4) for w in ld64_all], "read_ply_float32": [round(w, 4) for w in ld32_all]},
        },
    }
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
