#!/usr/bin/env python3
"""Times the raw image encodings (nidreg_image_to_mono8) on one 1920 x 1080 bayer_rggb8 frame and one 1920 x 1080 mono16 frame, split
into allocation + upload, kernel and copy back (nidreg_image_get_timing: the host clock around each phase of the synchronous call),
against the numpy restatement of tests/raw_image_oracle.py on one host core with the same bytes; checks that both give the same
bytes.  Writes profiles/raw_image.json (--out), stamped with nidreg_kernel_build(); README.md quotes only what that file holds.  The
rules are unpinned against OpenCV and cv_bridge, so there is no OpenCV column.  A plain script, not part of the test or bench contract.

    python tools/raw_image_time.py [--calls 20] [--warmup 3] [--out profiles/raw_image.json]
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

from direct_visual_lidar_calibration_amd import _lib, synth  # noqa: E402

import raw_image_oracle as ro  # noqa: E402


def make_frames():
    """``{encoding: (bytes as a uint8 array, width, height, step)}``: the synthetic 1080p scene's image as a mosaic and at 16 bits"""
    scene = synth.make_scene("pinhole_1080p", num_points=1000, seed=50)
    raw = np.ascontiguousarray(scene.image_u8)
    h, w = raw.shape
    yy, xx = np.mgrid[0:h, 0:w]
    deep = (raw.astype(np.int64) * 257 + (xx * 7 + yy * 3) % 257 - 128).clip(0, 65535).astype("<u2")
    return {"bayer_rggb8": (raw.reshape(-1), w, h, w), "mono16": (deep.view(np.uint8).reshape(-1), w, h, 2 * w)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw_image.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("raw_image_time: no GPU; there is nothing to measure without one")
    lib = _lib.load()
    result = {"kernel_build": _lib.library_kernel_build(), "device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup,
              "clock": "host clock; the phases are nidreg_image_get_timing of each synchronous call, medians over the calls; the host column is the numpy restatement on one core, "
                       "median over the same number of calls", "reference": "tests/raw_image_oracle.py; unpinned against OpenCV and cv_bridge", "encodings": {}}
    for encoding, (data, width, height, step) in make_frames().items():
        out = np.empty((height, width), dtype=np.uint8)
        p = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        phases, wall = [], []
        for k in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            _lib.check(lib.nidreg_image_to_mono8(0, data.ctypes.data, data.size, width, height, step, encoding.encode(), 0, p, width), "nidreg_image_to_mono8")
            dt = time.perf_counter() - t0
            ms = (ctypes.c_double * 3)()
            lib.nidreg_image_get_timing(ms)
            if k >= args.warmup:
                phases.append(list(ms))
                wall.append(dt * 1e3)
        host = []
        for k in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            want = ro.to_mono8(data, width, height, step, encoding)
            if k >= args.warmup:
                host.append((time.perf_counter() - t0) * 1e3)
        med = np.median(np.asarray(phases), axis=0)
        case = {"width": width, "height": height, "step": step, "source_bytes": int(data.size), "total_ms_median": float(np.median(wall)), "total_ms_min": float(np.min(wall)),
                "total_ms_max": float(np.max(wall)), "alloc_upload_ms": float(med[0]), "kernel_ms": float(med[1]), "copy_back_ms": float(med[2]),
                "host_numpy_one_core_ms_median": float(np.median(host)), "same_as_host_numpy": bool(np.array_equal(out, want))}
        if not case["same_as_host_numpy"]:
            raise SystemExit(f"raw_image_time: the device's image differs from the numpy restatement for {encoding}: {case}")
        result["encodings"][encoding] = case
        print(json.dumps({encoding: case}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
