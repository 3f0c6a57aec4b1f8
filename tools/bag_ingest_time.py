#!/usr/bin/env python3
"""Times the integration of one bag's PointCloud2 frames into the voxel integrator, end to end as preprocess_ros1 runs it, on the
shape of an Ouster bag: --frames 290 frames x --points 131072 records of 48 bytes (float32 x y z, pad, float32 intensity, uint32 t,
uint16 reflectivity, ...), 2 mm voxels, min_distance 1 m.  Two routes over the same message bytes, per frame:

    cloud2    StaticPointCloudIntegrator.insert_cloud2: the records uploaded as they lie in the message, decoded on the GPU
    host      what the integrator offered before: a numpy structured-dtype decode and the finite filter on one host core, then
              insert_points (the float32 route: 16 bytes per kept point uploaded)

A run is the whole bag into a fresh integrator, timed by the host clock from the first insert to the return of the last (every
insert ends in a device-to-host read, so the clock stops after the device has finished); the routes alternate, --warmup runs of
each first, then --runs timed ones; the medians, their ratio and the bytes uploaded per frame go to profiles/preprocess_ros1.json
(--out), stamped with nidreg_kernel_build().  The last runs' records are compared bit for bit.  --routes cloud2 / host runs one
route alone (for a kernel trace).  A plain script, not part of the test or bench contract.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from direct_visual_lidar_calibration_amd import _lib, preprocess  # noqa: E402

OUSTER = np.dtype({"names": ["x", "y", "z", "intensity", "t", "reflectivity", "ring", "ambient", "range"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u4", "<u2", "<u2", "<u2", "<u4"],
                   "offsets": [0, 4, 8, 16, 20, 24, 26, 28, 32], "itemsize": 48})
FIELDS = [(n, OUSTER.fields[n][1], {"f4": 7, "u4": 6, "u2": 4}[OUSTER.fields[n][0].str[1:]], 1) for n in OUSTER.names]
CHANNEL = "reflectivity"


_beams = {}


def make_frame(n, k):
    """Frame k of a spinning LiDAR standing in a 12 x 9 x 3.2 m room: n beams (128 rows) over an elevation band of +-22.5 degrees,
    the range to the first wall with 2 cm of noise; 0.5 % of the returns are NaN (dropped beams)"""
    if n not in _beams:
        rows = 128
        cols = n // rows
        az = (np.arange(cols) * (2 * np.pi / cols))[None, :]
        el = np.deg2rad(np.linspace(-22.5, 22.5, rows))[:, None]
        d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], axis=-1).reshape(-1, 3)
        with np.errstate(divide="ignore"):
            r0 = (np.array([6.0, 4.5, 1.6]) / np.abs(d)).min(axis=1)
        _beams[n] = (d.astype(np.float32), r0.astype(np.float32), np.linspace(0, 1e8, len(r0)).astype(np.uint32))
    d, r0, t = _beams[n]
    rng = np.random.default_rng([77, k])
    r = r0 + rng.normal(0, 0.02, len(r0)).astype(np.float32)
    rec = np.zeros(len(r), dtype=OUSTER)
    rec["x"], rec["y"], rec["z"] = d[:, 0] * r, d[:, 1] * r, d[:, 2] * r
    rec["x"][rng.integers(0, len(r), len(r) // 200)] = np.nan
    rec["reflectivity"] = rng.integers(0, 65536, len(r), dtype=np.uint16)
    rec["intensity"] = rec["reflectivity"] * np.float32(0.0625)
    rec["t"] = t
    rec["range"] = r * np.float32(1000)
    return rec.tobytes()


def run_cloud2(frames, n, res, min_distance):
    integ = preprocess.StaticPointCloudIntegrator(res, min_distance, device=0)
    msgs = [{"fields": FIELDS, "point_step": 48, "data": np.frombuffer(b, dtype=np.uint8), "num_points": n, "is_bigendian": 0} for b in frames]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    skipped = 0
    for m in msgs:
        skipped += integ.insert_cloud2(m, CHANNEL)
    secs = time.perf_counter() - t0
    return secs, integ, skipped, 48 * n


def run_host(frames, n, res, min_distance):
    integ = preprocess.StaticPointCloudIntegrator(res, min_distance, device=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    skipped = uploaded = 0
    for b in frames:
        rec = np.frombuffer(b, dtype=OUSTER)
        xyz = np.stack([rec["x"], rec["y"], rec["z"]], axis=1)
        inten = rec[CHANNEL].astype(np.float32)  # (exact: uint16)
        ok = np.isfinite(xyz).all(axis=1)
        xyz, inten = xyz[ok], inten[ok]
        integ.insert_points(xyz, inten)
        skipped += len(ok) - len(xyz)
        uploaded += 16 * len(xyz)
    secs = time.perf_counter() - t0
    return secs, integ, skipped, uploaded / len(frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_ros1.json"), help="'none' = print only")
    ap.add_argument("--frames", type=int, default=290)
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--voxel_resolution", type=float, default=0.002)
    ap.add_argument("--min_distance", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--routes", default="cloud2,host")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bag_ingest_time: no GPU; there is nothing to measure without one")
    build = _lib.library_kernel_build()
    routes = args.routes.split(",")
    run = {"cloud2": run_cloud2, "host": run_host}
    frames = [make_frame(args.points, k) for k in range(args.frames)]
    n = len(frames[0]) // 48
    print(f"{len(frames)} frames x {n} points generated", flush=True)
    times, last = {r: [] for r in routes}, {}
    for k in range(args.warmup + args.runs):
        for r in routes:  # alternating
            secs, integ, skipped, up = run[r](frames, n, args.voxel_resolution, args.min_distance)
            info = integ.info()
            if k == args.warmup + args.runs - 1 and len(routes) == 2:
                last[r] = integ.get_records()
            integ.close()
            if k >= args.warmup:
                times[r].append(secs)
            last[r + "_meta"] = {"skipped_points": int(skipped), "bytes_uploaded_per_frame": float(up), "voxels": info["voxels"], "table_capacity": info["capacity"], "offered": info["offered"]}
            print(json.dumps({"run": k, "route": r, "seconds": secs, "warmup": k < args.warmup}), flush=True)
    result = {"kernel_build": build, "device": torch.cuda.get_device_name(0), "frames": len(frames), "points_per_frame": n, "point_step": 48, "intensity_channel": CHANNEL,
              "voxel_resolution": args.voxel_resolution, "min_distance": args.min_distance, "runs": args.runs, "warmup": args.warmup,
              "clock": "host clock around the whole bag's inserts into a fresh integrator; every insert ends in a device-to-host read"}
    for r in routes:
        t = times[r]
        result[r] = dict(last[r + "_meta"], seconds_median=float(np.median(t)), seconds_min=float(min(t)), seconds_max=float(max(t)), points_per_s=len(frames) * n / float(np.median(t)))
    if len(routes) == 2:
        same = bool(np.array_equal(last["cloud2"].view(np.uint32), last["host"].view(np.uint32)))
        result["same_records"] = same
        result["host_over_cloud2"] = result["host"]["seconds_median"] / result["cloud2"]["seconds_median"]
        if not same:
            raise SystemExit("bag_ingest_time: the two routes' records differ")
    print(json.dumps(result), flush=True)
    if args.out != "none":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print("wrote", args.out)


if __name__ == "__main__":
    main()
