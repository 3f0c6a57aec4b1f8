#!/usr/bin/env python3
"""Times what the LRU eviction of the CT-GICP model (nidreg_odom_set_lru) costs and shows what it bounds, at the shape of
tools/odometry_time.py (frames of 131 072 points, 12 000 sampled, the linearisation against a model of the three frames before it):

  linearize_off   ONE nidreg_odom_linearize with the eviction off: the code of the commit before the eviction (k_odom_linearize<false>
                  stores nothing new).  ``--only_linearize_off`` measures nothing else and runs in any checkout that has this script, so a
                  job may alternate this commit and its parent in one visit; ``--merge label=file.json ...`` adds such runs to the output.
  linearize_on    the same call with the eviction on: every face-neighbour voxel found is stamped
  evict_pass      the third insert of a sequence (half of the model, the other half, one far point) on a handle with lru_thresh = 1,
                  lru_cycle = 3: its pass drops the first half.  The same insert on a handle that never evicts is subtracted; the table
                  has the default 2^19 slots.  Every repeat builds both models afresh.
  walk            ``--walk_scans`` scans of a sensor that sees ``--walk_range`` m, carried down a long corridor, through ScanMatcher over
                  DeviceBackend with the default threshold (100) and with 0: the model's peak voxels and blocks in use

Each time is the host clock around blocking calls (a linearisation ends in a copy to the host): per round the median of ``--calls``
calls, and over ``--rounds`` rounds the median, the smallest and the largest of those -- the spread a comparison has to clear.  Writes
profiles/preprocess_dynamic_lru.json (--out), stamped with nidreg_kernel_build().  A plain script, not part of the test or bench contract.

    python tools/odometry_lru_time.py [--sampled 12000] [--calls 200] [--rounds 5] [--merge parent=a.json ...] [--out profiles/preprocess_dynamic_lru.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import odometry_time as base  # noqa: E402  (its synthetic room)
from direct_visual_lidar_calibration_amd import _lib, odometry  # noqa: E402


def rounds_of(f, calls, rounds, warmup=20):
    for _ in range(warmup):
        f()
    out = []
    for _ in range(rounds):
        t = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            t.append(time.perf_counter() - t0)
        out.append(float(np.median(t)))
    return {"s_median": float(np.median(out)), "s_min_round": min(out), "s_max_round": max(out), "calls_per_round": calls, "rounds": rounds}


def scenario(args):
    """The frames through the integrator (for their poses and sampled indices), then the model of all frames but the last and the last
    frame as the source"""
    frames = [base.make_frame(args.points, f) for f in range(args.frames)]
    msgs = [{"fields": [(k, base.RECORD.fields[k][1], 7) for k in base.RECORD.names], "point_step": 20, "data": r.tobytes(), "num_points": r.shape[0], "is_bigendian": False} for r in frames]
    integ = odometry.DynamicPointCloudIntegrator(0.002, 1.0, 0, target_num_points=args.sampled)
    for msg in msgs:
        integ.insert_cloud2_timed(msg, "intensity", (16, 7), 1.0, 0.0)
    sampled, poses = [s.copy() for s in integ.sampled], integ.poses()
    integ.close()

    def cloud(f):
        rec, idx = frames[f], sampled[f]
        return np.ascontiguousarray(np.stack([rec["x"][idx], rec["y"][idx], rec["z"][idx]], axis=1).astype(np.float64)), rec["t"][idx].astype(np.float64)

    helper = odometry.DeviceBackend(0)
    model = []
    for f in range(args.frames - 1):
        pts, _ = cloud(f)
        pts = np.ascontiguousarray(pts @ poses[f][0][:3, :3].T + poses[f][0][:3, 3])
        model.append((pts, helper.knn_covariances(pts, 20)[2]))
    pts, times = cloud(args.frames - 1)
    covs = helper.knn_covariances(pts, 20)[2]
    helper.close()
    table, tidx = odometry.time_table(times)
    tab, d0, d1 = odometry.update_poses(poses[-1][0], poses[-1][1], table)
    return model, (pts, covs, tidx), odometry.pack_poses(tab, d0, d1)


def loaded(model, source, **kw):
    b = odometry.DeviceBackend(0, **kw)
    for pts, covs in model:
        b.model_insert(pts, covs)
    b.set_source(*source)
    return b


def evict_pass(model, repeats):
    pts, covs = np.concatenate([m[0] for m in model]), np.concatenate([m[1] for m in model])
    vx = np.floor(pts[:, 0])
    first = vx < np.median(vx)  # whole voxels on either side
    far = np.array([[500.5, 500.5, 500.5]])
    times = {"on": [], "off": []}
    info = None
    for _ in range(repeats):
        for name, kw in (("on", {"lru_thresh": 1, "lru_cycle": 3}), ("off", {})):
            b = odometry.DeviceBackend(0, **kw)
            b.model_insert(np.ascontiguousarray(pts[first]), np.ascontiguousarray(covs[first]))
            b.model_insert(np.ascontiguousarray(pts[~first]), np.ascontiguousarray(covs[~first]))
            before = b.model_info()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b.model_insert(far, covs[:1])
            times[name].append(time.perf_counter() - t0)
            if name == "on":
                info = {"voxels_before": before["voxels"], "points_before": before["points"], "blocks_before": before["blocks"], "after": b.model_info(), "lru": b.lru_info()}
            b.close()
    on, off = float(np.median(times["on"])), float(np.median(times["off"]))
    return {"third_insert_with_pass_s_median": on, "third_insert_without_s_median": off, "pass_s": on - off, "with_pass_s_min": min(times["on"]), "with_pass_s_max": max(times["on"]),
            "without_s_min": min(times["off"]), "without_s_max": max(times["off"]), "repeats": repeats, "table_slots": 1 << 19, **info}


def corridor_scan(f, rings, columns, max_range, speed):
    """One revolution in a corridor 6 m wide and 4 m high with a pillar every 2.5 m, seen from x = speed * time: sensor-frame points
    within ``max_range`` and their times"""
    az = np.repeat(2.0 * np.pi * np.arange(columns) / columns, rings)
    el = np.tile(np.deg2rad(np.linspace(-30.0, 30.0, rings)), columns)
    t = np.repeat(np.arange(columns) * (0.1 / columns), rings)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1)
    x = speed * (0.1 * f + t)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.minimum(3.0 / np.abs(d[:, 1]), np.where(d[:, 2] > 0, 2.5 / d[:, 2], np.where(d[:, 2] < 0, -1.5 / d[:, 2], np.inf)))
        # the pillars: planes x = 2.5 k (0.8 m deep on either wall), the nearest one ahead of (or behind) the ray
        ahead = np.where(d[:, 0] > 0, np.ceil(x / 2.5) * 2.5 - x, np.floor(x / 2.5) * 2.5 - x) / d[:, 0]
        y_at = ahead * d[:, 1]
        r = np.where(np.isfinite(ahead) & (ahead > 0) & (ahead < r) & (np.abs(y_at) > 2.2), ahead, r)
    keep = r <= max_range
    return np.ascontiguousarray((d * r[:, None])[keep]), t[keep]


def walk(args, lru_thresh):
    b = odometry.DeviceBackend(0, lru_thresh=lru_thresh)
    matcher = odometry.ScanMatcher(b, 20)
    peak = {"voxels": 0, "points": 0, "blocks": 0}
    t0 = time.perf_counter()
    for f in range(args.walk_scans):
        pts, times = corridor_scan(f, 32, 128, args.walk_range, args.walk_speed)
        matcher.insert(pts, times)
        info = b.model_info()
        peak = {k: max(peak[k], info[k]) for k in peak}
    out = {"lru_thresh": lru_thresh, "peak": peak, "final": b.model_info(), "lru": b.lru_info(), "estimated_travel_m": float(matcher.last_end[0, 3]), "wall_s": time.perf_counter() - t0}
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_dynamic_lru.json"))
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--sampled", type=int, default=12000)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7, help="of the eviction pass")
    ap.add_argument("--walk_scans", type=int, default=300)
    ap.add_argument("--walk_range", type=float, default=10.0)
    ap.add_argument("--walk_speed", type=float, default=2.0, help="m/s at 10 scans per second")
    ap.add_argument("--only_linearize_off", action="store_true")
    ap.add_argument("--merge", nargs="*", default=[], help="label=file.json of --only_linearize_off runs (of this commit or of its parent)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("odometry_lru_time: no GPU; there is nothing to measure without one")
    build = _lib.stamp_or_refuse()
    model, source, packed = scenario(args)
    off = loaded(model, source)
    result = {"kernel_build": build, "device": torch.cuda.get_device_name(0), "points_per_frame": args.points, "sampled": int(source[0].shape[0]), "time_table_entries": int(packed.shape[0]),
              "model": off.model_info(), "linearize_off": rounds_of(lambda: off.linearize(packed), args.calls, args.rounds)}
    sums_off = off.linearize(packed)
    off.close()
    if not args.only_linearize_off:
        on = loaded(model, source, lru_thresh=100)
        result["linearize_on"] = rounds_of(lambda: on.linearize(packed), args.calls, args.rounds)
        result["linearize_on_same_bits_as_off"] = bool(np.array_equal(on.linearize(packed), sums_off))
        on.close()
        result["evict_pass"] = evict_pass(model, args.repeats)
        result["walk"] = {"scans": args.walk_scans, "range_m": args.walk_range, "speed_m_per_s": args.walk_speed, "on": walk(args, 100), "off": walk(args, 0)}
        result["merged_linearize_off_runs"] = []
        for item in args.merge:
            label, path = item.split("=", 1)
            with open(path) as f:
                other = json.load(f)
            result["merged_linearize_off_runs"].append({"label": label, "kernel_build": other["kernel_build"], "model": other["model"], "linearize_off": other["linearize_off"]})
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
