#!/usr/bin/env python3
"""Times one draw of the headless viewer's point-splat renderer (nidreg_splat_draw: key reset, k_splat_depth, k_splat_resolve, copy
back of the RGB and index images) at 10M points onto 1920 x 1080, radius 0, 1 and 2, against the numpy restatement of
tests/viewer_oracle.py on one host core, and checks that the two pictures are the same bytes.  At radius 0 it also times
generate_lidar_image on the same inputs, for reference only: that call uploads the cloud every time and keeps an fp64 depth, so it is
shown next to "upload + colours + draw" rather than next to the draw alone.  Writes profiles/viewer.json (--out), stamped with
nidreg_kernel_build(); README.md and DESIGN.md quote only what that file holds.

All device figures are the host clock around the synchronous calls (the renderer runs on a stream of its own and returns when the
images are in host memory), median of --calls calls after --warmup calls.  A plain script, not part of the test or bench contract.

    python tools/splat_time.py [--points 10000000] [--size 1920x1080] [--radii 0,1,2] [--calls 5] [--warmup 2]
                               [--host_max 10000000] [--out profiles/viewer.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from direct_visual_lidar_calibration_amd import _lib, nid, render, se3, synth  # noqa: E402

import viewer_oracle  # noqa: E402  (the restatement the tests compare with; its projection is the CPU oracle's)


def timed(f, calls, warmup):
    out, secs = None, []
    for k in range(warmup + calls):
        t0 = time.perf_counter()
        out = f()
        if k >= warmup:
            secs.append(time.perf_counter() - t0)
    return out, secs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viewer.json"))
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--radii", default="0,1,2")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host_max", type=int, default=10_000_000, help="largest cloud the numpy restatement is timed (and compared) on")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("splat_time: no GPU; there is nothing to measure without one")
    W, H = (int(v) for v in args.size.lower().split("x"))
    n = args.points
    scene = synth.make_scene("pinhole_1080p", num_points=n, seed=50, device="cuda")
    proj = nid.create_camera(scene.model, scene.intrinsics, scene.distortion)
    T = se3.to_matrix(scene.T_camera_lidar_true)
    rgba = render.quantize_colors(render.colormap_turbo(scene.intensities))
    min_nz = math.cos(nid.estimate_camera_fov(proj, (W, H)) + 0.5 * math.pi / 180.0)
    result = {"kernel_build": _lib.library_kernel_build(), "device": torch.cuda.get_device_name(0), "points": n, "width": W, "height": H, "camera": "pinhole_1080p", "calls": args.calls,
              "warmup": args.warmup, "clock": "host clock around the synchronous calls", "cases": []}

    t0 = time.perf_counter()
    r = render.SplatRenderer(scene.points)
    r.set_colors(rgba)
    result["upload_points_and_colors_s"] = time.perf_counter() - t0  # (the first call in the process: includes loading the code objects)
    for radius in [int(v) for v in args.radii.split(",")]:
        (rgb, index), secs = timed(lambda: r.draw(proj, (W, H), T, radius=radius, min_nz=min_nz), args.calls, args.warmup)
        case = {"radius": radius, "draw_s_median": float(np.median(secs)), "draw_s_min": float(min(secs)), "draw_s_max": float(max(secs)), "points_per_s": n / float(np.median(secs)),
                "pixels_covered": int((index >= 0).sum())}
        if n <= args.host_max:
            t0 = time.perf_counter()
            want = viewer_oracle.draw(scene.model, scene.intrinsics, scene.distortion, scene.points, rgba, T, W, H, min_nz, radius=radius)
            host = time.perf_counter() - t0
            same = bool(np.array_equal(rgb, want[0]) and np.array_equal(index, want[1]))
            case.update(host_numpy_one_core_s=host, same_as_host=same, speedup_over_host=host / case["draw_s_median"])
            if not same:
                raise SystemExit(f"splat_time: the device's picture differs from the numpy restatement's at radius {radius}")
        else:
            case.update(host_numpy_one_core_s=None, note="numpy restatement not measured at this size")
        if radius == 0:
            def fresh():
                h = render.SplatRenderer(scene.points)
                h.set_colors(rgba)
                out = h.draw(proj, (W, H), T, radius=0, min_nz=min_nz)
                h.close()
                return out
            _, secs = timed(fresh, args.calls, args.warmup)
            (_, lidar_index), lsecs = timed(lambda: render.generate_lidar_image(proj, (W, H), T, scene.points, scene.intensities, min_z=min_nz), args.calls, args.warmup)
            case.update(upload_colors_draw_s_median=float(np.median(secs)), generate_lidar_image_s_median=float(np.median(lsecs)),
                        generate_lidar_image_note="for reference only: uploads the cloud per call, fp64 depth, two passes over the points, double intensity image",
                        index_pixels_differing_from_generate_lidar_image=int((lidar_index != index).sum()))
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
    r.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
