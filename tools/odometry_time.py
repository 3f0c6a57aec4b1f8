#!/usr/bin/env python3
"""Times the four device stages of the dynamic integrator (preprocess_dynamic) per frame at the default shape -- frames of 131 072
points, 10 000 sampled -- against the numpy restatement of tests/odometry_oracle.py on one host core:

  knn_cov     nidreg_odom_knn_covariances: kNN (k = 20) among the sampled points, covariances and their PLANE regularisation
  model       nidreg_odom_model_insert of the sampled points into an EMPTY model: no distance test against stored points; the median
              time of creating the handle, measured separately, is subtracted
  linearize   ONE nidreg_odom_linearize (correspondences, Mahalanobis matrices, the 122 sums) + ONE nidreg_odom_error; a frame takes
              as many as the optimiser iterates ("lm_iterations" of the full frame says how many it took here)
  deskew      nidreg_odom_deskew_insert of the whole raw frame (upload, decode, per-point pose, the voxel table's three passes) into an
              EMPTY voxel table; the separately measured median time of creating the table is subtracted
  frame       DynamicPointCloudIntegrator.insert_cloud2_timed as a caller sees it: the host steps (decode, sort, sampling, the
              optimiser) included

Writes profiles/preprocess_dynamic.json (--out), stamped with nidreg_kernel_build(); README.md quotes only what that file holds.  Each
figure is the host clock around the blocking call, median of --calls after --warmup.  The scene is a synthetic room seen by a spinning
sensor that moves 5 cm and yaws 0.02 rad per frame.  A plain script, not part of the test or bench contract.

    python tools/odometry_time.py [--points 131072] [--sampled 10000] [--frames 4] [--calls 5] [--warmup 2] [--out profiles/preprocess_dynamic.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import odometry_oracle as oracle  # noqa: E402
from direct_visual_lidar_calibration_amd import _lib, odometry, preprocess  # noqa: E402

RECORD = np.dtype({"names": ["x", "y", "z", "intensity", "t"], "formats": ["<f4"] * 5, "offsets": [0, 4, 8, 12, 16], "itemsize": 20})
ROOM = np.array([[-10.0, -8.0, -1.5], [10.0, 8.0, 3.0]])


def make_frame(n, f):
    """n points of a box room seen from a sensor 5 cm and 0.02 rad further along per frame, columns stamped over 0.1 s"""
    rings = 128
    cols = n // rings
    az = np.repeat(2.0 * np.pi * np.arange(cols) / cols, rings)
    el = np.tile(np.deg2rad(np.linspace(-22.5, 22.5, rings)), cols)
    t = np.repeat(np.arange(cols) * (0.1 / cols), rings)
    yaw, pos = 0.2 * (0.1 * f + t), np.stack([0.5 * (0.1 * f + t), np.zeros_like(t), np.zeros_like(t)], axis=1)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1)
    dw = np.stack([np.cos(yaw) * d[:, 0] - np.sin(yaw) * d[:, 1], np.sin(yaw) * d[:, 0] + np.cos(yaw) * d[:, 1], d[:, 2]], axis=1)
    with np.errstate(divide="ignore"):
        r = np.min(np.maximum((ROOM[0] - pos) / dw, (ROOM[1] - pos) / dw), axis=1)
    rec = np.zeros(rings * cols, dtype=RECORD)
    rec["x"], rec["y"], rec["z"] = (d * r[:, None]).T
    rec["t"], rec["intensity"] = t, 100.0 + 50.0 * np.sin(az)
    return rec


def clock(f, calls, warmup):
    out = []
    for _ in range(warmup + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out[warmup:])), float(min(out[warmup:])), float(max(out[warmup:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_dynamic.json"))
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--sampled", type=int, default=10000)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("odometry_time: no GPU; there is nothing to measure without one")
    build = _lib.library_kernel_build()
    frames = [make_frame(args.points, f) for f in range(args.frames)]
    msgs = [{"fields": [(k, RECORD.fields[k][1], 7) for k in RECORD.names], "point_step": 20, "data": r.tobytes(), "num_points": r.shape[0], "is_bigendian": False} for r in frames]

    # the whole frame, as a caller sees it
    integ = odometry.DynamicPointCloudIntegrator(0.002, 1.0, 0, target_num_points=args.sampled)
    frame_s = []
    for msg in msgs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        integ.insert_cloud2_timed(msg, "intensity", (16, 7), 1.0, 0.0)
        torch.cuda.synchronize()
        frame_s.append(time.perf_counter() - t0)
    iterations, sampled, poses, info = list(integ._matcher.iterations), [s.copy() for s in integ.sampled], integ.poses(), integ.info()
    integ.close()

    # the stages, on the last frame against a model of the frames before it
    def cloud(f):
        rec, idx = frames[f], sampled[f]
        return np.ascontiguousarray(np.stack([rec["x"][idx], rec["y"][idx], rec["z"][idx]], axis=1).astype(np.float64)), rec["t"][idx].astype(np.float64)

    backend = odometry.DeviceBackend(0)
    cpu = oracle.IVox()
    for f in range(args.frames - 1):
        pts, _ = cloud(f)
        pts = pts @ poses[f][0][:3, :3].T + poses[f][0][:3, 3]
        _, _, covs = backend.knn_covariances(pts, 20)
        backend.model_insert(pts, covs)
        cpu.insert(pts, covs)
    pts, times = cloud(args.frames - 1)
    m = pts.shape[0]
    nbr, _, covs = backend.knn_covariances(pts, 20)
    table, tidx = odometry.time_table(times)
    T0, T1 = poses[-1]
    tab, d0, d1 = odometry.update_poses(T0, T1, table)
    packed, packed12 = odometry.pack_poses(tab, d0, d1), odometry.pack_poses(tab)
    backend.set_source(pts, covs, tidx)
    stages = {}
    stages["knn_cov"] = clock(lambda: backend.knn_covariances(pts, 20), args.calls, args.warmup)
    stages["linearize"] = clock(lambda: (backend.linearize(packed), backend.error(packed12)), args.calls, args.warmup)
    moved = pts @ T1[:3, :3].T + T1[:3, 3]

    def model_once():
        b = odometry.DeviceBackend(0)
        try:
            b.model_insert(moved, covs)
        finally:
            b.close()

    create = clock(lambda: odometry.DeviceBackend(0).close(), args.calls, args.warmup)
    with_create = clock(model_once, args.calls, args.warmup)
    stages["model"] = tuple(max(0.0, a - b) for a, b in zip(with_create, (create[0],) * 3))  # into a FRESH model (the handle's creation subtracted)
    layout = preprocess.cloud2_layout(msgs[-1], "intensity")

    def deskew_once():
        grid = preprocess.StaticPointCloudIntegrator(0.002, 1.0, 0)
        try:
            odometry.deskew_insert(grid, layout, "intensity", (16, 7), 1.0, 0.0, float(frames[-1]["t"].max()), T0, T1)
        finally:
            grid.close()

    grid_create = clock(lambda: preprocess.StaticPointCloudIntegrator(0.002, 1.0, 0).close(), args.calls, args.warmup)
    with_grid = clock(deskew_once, args.calls, args.warmup)
    stages["deskew"] = tuple(max(0.0, a - grid_create[0]) for a in with_grid)  # into a FRESH voxel table (its creation subtracted)

    # the numpy restatement on one host core, once each
    host = {}
    t0 = time.perf_counter()
    want_nbr, _ = oracle.knn(pts, 20)
    oracle.covariances(pts, want_nbr)
    host["knn_cov"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    oracle.IVox().insert(moved, covs)
    host["model"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    lin = oracle.linearize(pts, covs, tidx, packed, cpu)
    oracle.error(pts, tidx, packed12, lin["found"], lin["target"], lin["mahal"])
    host["linearize"] = time.perf_counter() - t0
    rec = frames[-1]
    raw = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float64)
    t0 = time.perf_counter()
    out = oracle.deskew(raw, rec["t"].astype(np.float64), float(rec["t"].max()), T0, T1)
    v = np.floor(out / 0.002).astype(np.int64) + (1 << 20)
    np.unique((v[:, 0] | (v[:, 1] << 21) | (v[:, 2] << 42))[::-1], return_index=True)
    host["deskew"] = time.perf_counter() - t0
    same_sets = bool(np.array_equal(np.sort(nbr, axis=1), np.sort(want_nbr, axis=1)))

    result = {"kernel_build": build, "device": torch.cuda.get_device_name(0), "points_per_frame": args.points, "sampled": int(m), "k_neighbors": 20, "frames": args.frames,
              "calls": args.calls, "warmup": args.warmup, "time_table_entries": int(table.shape[0]), "model_points": info["model"]["points"], "model_voxels": info["model"]["voxels"],
              "lm_iterations_per_frame": iterations, "frame_host_clock_s": frame_s, "knn_sets_same_as_host": same_sets,
              "stages": {k: {"device_s_median": v[0], "device_s_min": v[1], "device_s_max": v[2], "host_numpy_one_core_s": host[k]} for k, v in stages.items()}}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
