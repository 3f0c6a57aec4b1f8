#!/usr/bin/env python3
"""Times the voxel integrator (nidreg_integrator_insert_f32 + nidreg_integrator_get, one frame into a fresh integrator) on
float32 clouds from synth at map resolution (2 mm) and at 5 cm, against a numpy restatement on one host core -- np.unique over
the packed voxel keys with last-occurrence selection.  Writes profiles/preprocess_map.json (--out), stamped with
nidreg_kernel_build(); README.md and DESIGN.md quote only what that file holds.

The device figure is the time between two HIP events around the two calls as a caller sees them (upload of the frame, check
pass, claim + payload passes, table growth, compaction, sort, gather, copy back), median of --calls calls after --warmup calls,
every call on a fresh integrator; the host clock around the same calls is recorded next to it.  "bytes streamed" = 16 bytes per
input point + 24 bytes (record + sequence number) per voxel returned.  A plain script, not part of the test or bench contract.

    python tools/voxel_time.py [--points 1000000,10000000] [--resolutions 0.002,0.05] [--calls 5] [--warmup 3]
                               [--host_max 10000000] [--out profiles/preprocess_map.json]

Cases already in --out from the same kernel build are kept (the 50M-point shape is run on its own, last).
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

from direct_visual_lidar_calibration_amd import _lib, preprocess, synth  # noqa: E402


def make_records(n):
    """(n, 4) float32 records x y z intensity of a synth scene (built on the GPU)"""
    scene = synth.make_scene("pinhole_1080p", num_points=n, seed=50, device="cuda")
    rec = np.empty((n, 4), dtype=np.float32)
    rec[:, :3] = scene.points[:, :3]
    rec[:, 3] = scene.intensities
    return rec


def numpy_last_per_voxel(rec, res):
    """The restatement on one host core: indices of the last point of every voxel, ascending"""
    v = np.floor(rec[:, :3].astype(np.float64) / res).astype(np.int64) + (1 << 20)
    keys = v[:, 0] | (v[:, 1] << 21) | (v[:, 2] << 42)
    _, first_in_reversed = np.unique(keys[::-1], return_index=True)
    return np.sort(len(keys) - 1 - first_in_reversed)


def device_once(rec, res):
    integ = preprocess.StaticPointCloudIntegrator(res, 0.0, device=0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    integ.insert_points(rec[:, :3], rec[:, 3])
    out = integ.get_records()
    e1.record()
    e1.synchronize()
    wall = time.perf_counter() - t0
    info, seq = integ.info(), integ.last_seq
    integ.close()
    return 1e-3 * e0.elapsed_time(e1), wall, out, seq, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_map.json"))
    ap.add_argument("--points", default="1000000,10000000")
    ap.add_argument("--resolutions", default="0.002,0.05")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host_max", type=int, default=10_000_000, help="largest shape the numpy restatement is timed (and compared) on")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("voxel_time: no GPU; there is nothing to measure without one")
    build = _lib.library_kernel_build()
    result = {"kernel_build": build, "device": torch.cuda.get_device_name(0), "cases": []}
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = json.load(f)
        if old.get("kernel_build") == build:
            result["cases"] = old.get("cases", [])
    device_once(make_records(100_000), 0.05)  # code objects, allocator
    for n in [int(v) for v in args.points.split(",")]:
        rec = make_records(n)
        for res in [float(v) for v in args.resolutions.split(",")]:
            runs = [device_once(rec, res) for _ in range(args.warmup + args.calls)][args.warmup:]
            secs = float(np.median([r[0] for r in runs]))
            _, _, out, seq, info = runs[-1]
            m = out.shape[0]
            streamed = 16 * n + 24 * m
            case = {"points": n, "voxel_resolution": res, "voxels": m, "table_capacity": info["capacity"], "calls": args.calls, "warmup": args.warmup, "device_s_median": secs,
                    "device_s_min": float(min(r[0] for r in runs)), "device_s_max": float(max(r[0] for r in runs)), "host_clock_s_median": float(np.median([r[1] for r in runs])),
                    "points_per_s": n / secs, "bytes_streamed": streamed, "bytes_streamed_per_s": streamed / secs}
            if n <= args.host_max:
                t0 = time.perf_counter()
                last = numpy_last_per_voxel(rec, res)
                host = time.perf_counter() - t0
                same = bool(np.array_equal(last, seq) and np.array_equal(rec[last].view(np.uint32), out.view(np.uint32)))
                case.update(host_numpy_one_core_s=host, host_points_per_s=n / host, same_as_host=same, speedup_over_host=host / secs)
                if not same:
                    raise SystemExit(f"voxel_time: the device's voxels differ from the numpy restatement's at {n} points, resolution {res}")
            else:
                case.update(host_numpy_one_core_s=None, note="numpy restatement not measured at this size")
            result["cases"] = [c for c in result["cases"] if (c["points"], c["voxel_resolution"]) != (n, res)] + [case]
            print(json.dumps(case), flush=True)
    result["cases"].sort(key=lambda c: (c["points"], -c["voxel_resolution"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
