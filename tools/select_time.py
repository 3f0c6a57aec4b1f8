#!/usr/bin/env python3
"""Times the device-side selection behind ``--mask`` / ``--min_range`` / ``--max_range`` (nid.Cloud.select: launch_cull, k_select_flags,
k_select_scan, k_select_scatter) at 10M points onto 1920 x 1080:

* one ``Cloud.select``, cull included, with a mask (a bonnet and a timestamp box, margin 2) and with none;
* the same index list obtained with what the library offered before: ``nidreg_view_culling`` (uploads the cloud, compacts the flags
  on the host), the pixel of every survivor through ``nidreg_project_model``, a numpy mask test on a numpy erosion, and a new
  ``Cloud`` upload of the selected points -- the indices that differ from the device's are counted;
* ``calibrate_pairs``' ``build_s`` of ONE outer iteration (one pair, one BFGS iteration) through the select route with an all-valid
  mask against the fused ``cull=`` route: the select route pays one extra gather of 40 B per surviving point.

Writes profiles/cloud_select.json (--out), stamped with nidreg_kernel_build(); README.md quotes only what that file holds.  All
figures are the host clock around the synchronous calls, median of --calls calls after --warmup.  Not measured: real masks on real
data.  A plain script, not part of the test or bench contract.

    python tools/select_time.py [--points 10000000] [--calls 5] [--warmup 2] [--out profiles/cloud_select.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from direct_visual_lidar_calibration_amd import _lib, calibrate, calibration, nid, se3, synth  # noqa: E402


def timed(f, calls, warmup):
    out, secs = None, []
    for k in range(warmup + calls):
        t0 = time.perf_counter()
        out = f()
        if k >= warmup:
            secs.append(time.perf_counter() - t0)
    return out, {"median_s": float(np.median(secs)), "min_s": float(min(secs)), "max_s": float(max(secs))}


def erode_numpy(mask, R):
    """the erosion of nidreg_mask_create as shifted minima (window clipped to the image)"""
    out = mask.copy()
    H, W = mask.shape
    for d in range(1, R + 1):
        out[:, d:] = np.minimum(out[:, d:], mask[:, : W - d])
        out[:, : W - d] = np.minimum(out[:, : W - d], mask[:, d:])
    rows = out.copy()
    for d in range(1, R + 1):
        out[d:, :] = np.minimum(out[d:, :], rows[: H - d, :])
        out[: H - d, :] = np.minimum(out[: H - d, :], rows[d:, :])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_select.json"))
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("select_time: no GPU; there is nothing to measure without one")
    n = args.points
    scene = synth.make_scene("pinhole_1080p", num_points=n, seed=50, device="cuda")
    W, H = scene.width, scene.height
    proj = nid.create_camera(scene.model, scene.intrinsics, scene.distortion)
    x7 = scene.T_camera_lidar_init
    T = se3.to_matrix(x7)
    min_z = math.cos(nid.estimate_camera_fov(proj, (W, H)))
    mask_u8 = np.full((H, W), 255, dtype=np.uint8)
    mask_u8[int(0.8 * H) :, :] = 0   # the bonnet
    mask_u8[20:60, 40:520] = 0       # a burnt-in timestamp
    result = {"kernel_build": _lib.library_kernel_build(), "device": torch.cuda.get_device_name(0), "points": n, "width": W, "height": H, "camera": "pinhole_1080p", "calls": args.calls,
              "warmup": args.warmup, "clock": "host clock around the synchronous calls", "select_tile": _lib.SELECT_TILE, "not_measured": "real masks on real data"}

    t0 = time.perf_counter()
    cloud = nid.Cloud(scene.points, scene.intensities)
    result["cloud_upload_s"] = time.perf_counter() - t0  # (the first call in the process: includes loading the code objects)
    mask, result["mask_create_margin2"] = timed(lambda: nid.Mask(mask_u8, margin=2), args.calls, args.warmup)

    def select(m, indices=False):
        out = cloud.select(proj, (W, H), T, min_z, True, mask=m, return_indices=indices)
        sub = out[0] if indices else out
        counts, size = dict(sub.select_counts), sub.num_points
        sub.close()
        return (counts, size, out[1]) if indices else (counts, size)

    (counts, size), result["select_no_mask"] = timed(lambda: select(None), args.calls, args.warmup)
    result["select_no_mask"].update(selected=size, **counts)
    (counts, size), result["select_with_mask"] = timed(lambda: select(mask), args.calls, args.warmup)
    result["select_with_mask"].update(selected=size, **counts)
    (_, _, idx_device), result["select_with_mask_and_indices"] = timed(lambda: select(mask, True), args.calls, args.warmup)

    # ---- the same result with what the library offered before
    culling = nid.ViewCulling(proj, (W, H), min_z=min_z)
    parts = {}

    def before():
        t0 = time.perf_counter()
        keep = culling.cull(scene.points, T)
        t1 = time.perf_counter()
        pc = scene.points[keep, :3] @ T[:3, :3].T + T[:3, 3]
        uv = proj.project(pc)
        valid = erode_numpy(mask_u8, 2)[uv[:, 1].astype(np.int64), uv[:, 0].astype(np.int64)] != 0
        idx = keep[valid]
        t2 = time.perf_counter()
        sub = nid.Cloud(np.ascontiguousarray(scene.points[idx]), np.ascontiguousarray(scene.intensities[idx]))
        sub.close()
        t3 = time.perf_counter()
        parts.setdefault("view_culling_s", []).append(t1 - t0)
        parts.setdefault("project_and_numpy_mask_s", []).append(t2 - t1)
        parts.setdefault("gather_and_upload_s", []).append(t3 - t2)
        return idx

    idx_before, result["before_view_culling_numpy_mask_upload"] = timed(before, max(args.calls // 2, 2), 1)
    result["before_view_culling_numpy_mask_upload"].update({k: float(np.median(v[1:])) for k, v in parts.items()})
    # (the host projects with a BLAS product, the cull with Eigen's summation order: a point within an ulp of a pixel boundary may differ)
    result["before_view_culling_numpy_mask_upload"]["indices_differing_from_select"] = int(len(np.setxor1d(idx_before, idx_device)))
    result["speedup_select_with_mask_over_before"] = result["before_view_culling_numpy_mask_upload"]["median_s"] / result["select_with_mask"]["median_s"]
    mask.close()
    cloud.close()

    # ---- build_s of one outer iteration: the select route with an all-valid mask against the fused cull= route
    params = calibration.VisualCameraCalibrationParams(max_outer_iterations=1, bfgs_max_iterations=1, nid_bins=16)
    pairs = [(scene.image_u8, scene.points, scene.intensities)]
    sel = {"masks": [np.full((H, W), 255, dtype=np.uint8)], "margin": 2, "min_range": 0.0, "max_range": math.inf}

    def build_s(selection):
        stats = {}
        calibrate.calibrate_pairs(proj, pairs, x7, params, stats=stats, **({} if selection is None else {"selection": selection}))
        return stats["build_s"]

    fused = [build_s(None) for _ in range(args.warmup + args.calls)][args.warmup :]
    selected = [build_s(sel) for _ in range(args.warmup + args.calls)][args.warmup :]
    result["build_s_one_outer_iteration"] = {"fused_cull_route_median_s": float(np.median(fused)), "select_route_all_valid_mask_median_s": float(np.median(selected)),
                                             "fused_all_s": fused, "select_all_s": selected, "bins": 16, "registration_type": "nid_bfgs"}
    print(json.dumps(result, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
