#!/usr/bin/env python3
"""Measures what ``evaluate`` rests on, once, with nothing tuned:

* one ``nid.Cloud.fold`` at 10M points -- fold 3 of 8 alone and its complement, spatial blocks of 1 m, indices included -- against the
  route the library offered before: ``Cloud.get`` (the cloud back to the host), a numpy gather, a new ``Cloud`` upload.  The fold ids
  of the old route come from the numpy restatement of the rule, outside the timed part; the two index lists must be equal.
* one whole ``evaluate`` with its defaults on the synthetic 1M-point VGA scene (``synth.make_scene("pinhole_vga", 1_000_000, seed=41)``,
  one bag, so no leave-one-out), section by section, with what the spread, the agreeing share and the sweep minima come to.  Those
  are findings on a SYNTHETIC scene; on real data they are unmeasured.

Writes profiles/evaluate.json (--out), stamped with nidreg_kernel_build().  Host clock around synchronous calls, median of --calls
calls after --warmup.  A plain script, not part of the test or bench contract.

    python tools/evaluate_time.py [--points 10000000] [--calls 5] [--warmup 2] [--out profiles/evaluate.json]
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

from direct_visual_lidar_calibration_amd import _lib, dataset, evaluate, nid, synth  # noqa: E402

U = np.uint64


def fold_ids_numpy(points, seed, num_folds, cell):
    """the rule of include/nidreg.h (cell > 0, every point inside the packing: asserted)"""
    c = np.floor(points[:, :3] / cell)
    assert np.isfinite(c).all() and (np.abs(c) < (1 << 20)).all()
    ci = c.astype(np.int64) + (1 << 20)
    key = ci[:, 0].astype(U) | (ci[:, 1].astype(U) << U(21)) | (ci[:, 2].astype(U) << U(42))
    with np.errstate(over="ignore"):
        z = U(seed) + U(0x9E3779B97F4A7C15) * (key + U(1))
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        z = z ^ (z >> U(31))
        return (((z >> U(32)) * U(num_folds)) >> U(32)).astype(np.int32)


def timed(f, calls, warmup):
    out, secs = None, []
    for k in range(warmup + calls):
        t0 = time.perf_counter()
        out = f()
        if k >= warmup:
            secs.append(time.perf_counter() - t0)
    return out, {"median_s": float(np.median(secs)), "min_s": float(min(secs)), "max_s": float(max(secs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate.json"))
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_time: no GPU; there is nothing to measure without one")
    result = {"kernel_build": _lib.stamp_or_refuse(), "device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup,
              "clock": "host clock around the synchronous calls", "not_measured": "spread, agreeing share and sweep minima on real data"}

    # ---- one fold at --points
    n, seed, K, k, cell = args.points, 7, 8, 3, 1.0
    scene = synth.make_scene("pinhole_1080p", num_points=n, seed=50, device="cuda")
    cloud = nid.Cloud(scene.points, scene.intensities)
    ids = fold_ids_numpy(scene.points, seed, K, cell)
    fold = {"points": n, "num_folds": K, "fold": k, "cell": cell, "bytes_per_point": 40}
    for name, complement in (("subset", False), ("complement", True)):
        def device():
            sub, idx = cloud.fold(seed, K, k, complement=complement, cell=cell, return_indices=True)
            sub.close()
            return idx

        def device_no_indices():
            cloud.fold(seed, K, k, complement=complement, cell=cell).close()

        def before():
            pts, inten = cloud.get()
            idx = np.flatnonzero((ids == k) != complement).astype(np.int32)
            nid.Cloud(np.ascontiguousarray(pts[idx]), np.ascontiguousarray(inten[idx])).close()
            return idx

        idx_d, t_d = timed(device, args.calls, args.warmup)
        _, t_n = timed(device_no_indices, args.calls, args.warmup)
        idx_b, t_b = timed(before, max(args.calls // 2, 2), 1)
        if not np.array_equal(idx_d, idx_b):
            raise SystemExit(f"evaluate_time: the {name}'s indices differ between the device and the host route")
        fold[name] = {"selected": int(len(idx_d)), "cloud_fold_with_indices": t_d, "cloud_fold": t_n, "before_get_numpy_gather_upload": t_b, "indices_equal": True,
                      "speedup_cloud_fold_over_before": t_b["median_s"] / t_n["median_s"]}
    _, fold["fold_ids_with_sizes"] = timed(lambda: cloud.fold_ids(seed, K, cell), args.calls, args.warmup)
    cloud.close()
    result["fold_10M" if n == 10_000_000 else f"fold_{n}"] = fold
    del scene, ids

    # ---- one whole evaluate, defaults, the synthetic 1M-point VGA scene
    s = synth.make_scene("pinhole_vga", num_points=1_000_000, seed=41)
    with tempfile.TemporaryDirectory() as d:
        dataset.write_preprocessed(d, (s.model, s.intrinsics, s.distortion), [("bag0", s.image_u8, s.points, s.intensities)],
                                   init_T_lidar_camera_tum=dataset.T_camera_lidar_to_tum(s.T_camera_lidar_init))
        lines = []
        t0 = time.perf_counter()
        out = evaluate.run(evaluate.build_parser().parse_args([d]), log=lines.append)
        total = time.perf_counter() - t0
    calibrations = 1 + len(out["folds"]["replicates"]) + len(out["restarts"]["replicates"])
    result["evaluate_defaults_synthetic_1M"] = {
        "scene": "synth.make_scene('pinhole_vga', 1_000_000, seed=41), one bag, initial guess = the scene's perturbed pose", "synthetic": True,
        "total_s_including_the_directory_read": total, "calibrations": calibrations,
        "seconds": {k: out[k]["seconds"] for k in ("upload", "full", "folds", "restarts", "sweeps")},
        "full": {k: out["full"][k] for k in ("final_cost", "evaluations", "outer_iterations")},
        "folds": {k: out["folds"][k] for k in ("mode", "num_folds", "cell", "sizes", "se", "mean_d", "max_trans", "max_rot")},
        "restarts": {"count": len(out["restarts"]["replicates"]), **{k: out["restarts"][k] for k in ("agree_share", "max_trans", "max_rot", "trans", "rot_deg")}},
        "sweeps": {name: {"argmin_delta": ax["delta"][ax["argmin"]], "interior": ax["interior"], "cost_at_minimum": ax["cost"][ax["argmin"]]} for name, ax in out["sweeps"]["axes"].items()},
        "leave_one_out": "one bag: skipped", "log": [ln for ln in lines if not ln.startswith("saved to")]}  # (that line names a temporary directory)
    print(json.dumps(result, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
