#!/usr/bin/env python3
"""Times the baseline JPEG decoder (nidreg_jpeg_decode_gray) on one 1920 x 1080 4:2:0 quality-90 frame in both gray modes, split
into host entropy decode, allocation + upload, kernels and copy back (nidreg_jpeg_get_timing: the host clock around each phase
of the synchronous call), against the numpy restatement of tests/jpeg_oracle.py on one host core and, where Pillow is installed,
against Pillow's libjpeg-turbo decode of the same bytes; checks that all of them give the same bytes.  Writes profiles/jpeg.json
(--out), stamped with nidreg_kernel_build(); README.md quotes only what that file holds.  A plain script, not part of the test or
bench contract.

    python tools/jpeg_time.py [--stream frame.jpg] [--calls 10] [--warmup 2] [--out profiles/jpeg.json]

Without --stream the frame is the synthetic 1080p scene's image, tinted, encoded here with Pillow (which is then required).
"""
import argparse
import ctypes
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from direct_visual_lidar_calibration_amd import _lib, dataset, synth  # noqa: E402

import jpeg_oracle as jo  # noqa: E402


def make_frame():
    from PIL import Image

    scene = synth.make_scene("pinhole_1080p", num_points=1000, seed=50)
    raw = (scene.image_u8 // 2 + 40).astype(np.int64)
    yy, xx = np.mgrid[0 : raw.shape[0], 0 : raw.shape[1]]
    rgb = np.clip(np.stack([raw + xx * 60 // raw.shape[1] - 30, raw + 10 - yy * 40 // raw.shape[0], raw + (xx + yy) % 64 - 32], axis=2), 0, 255).astype(np.uint8)
    out = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(out, "JPEG", quality=90, subsampling="4:2:0")
    return out.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg.json"))
    ap.add_argument("--stream", help="a JPEG file to time instead of the generated frame")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_time: no GPU; there is nothing to measure without one")
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if args.stream:
        with open(args.stream, "rb") as f:
            data = f.read()
    elif Image is None:
        raise SystemExit("jpeg_time: Pillow is not installed, so the frame cannot be encoded here; pass --stream")
    else:
        data = make_frame()
    width, height, components, subsampling, _ = dataset.jpeg_info(data)
    lib = _lib.load()
    result = {"kernel_build": _lib.library_kernel_build(), "device": torch.cuda.get_device_name(0), "width": width, "height": height, "components": components,
              "subsampling": ["gray", "4:4:4", "4:2:2", "4:2:0"][subsampling], "stream_bytes": len(data), "calls": args.calls, "warmup": args.warmup,
              "clock": "host clock; the phases are nidreg_jpeg_get_timing of each synchronous call, medians over the calls", "modes": {}}

    # the numpy restatement on one host core: the entropy decode is a pure-Python loop, the arithmetic is numpy
    t0 = time.perf_counter()
    s, blocks = jo.coefficients(data)
    t1 = time.perf_counter()
    planes = [jo.idct_blocks(b, s.qt[c["tq"]])[: c["dh"], : c["dw"]] for b, c in zip(blocks, s.comps)]
    t2 = time.perf_counter()
    want = {dataset.JPEG_GRAY_LUMA: planes[0], dataset.JPEG_GRAY_BGR: planes[0]}
    host_color = 0.0
    if len(planes) == 3:
        cb, cr = (jo.upsample(p, s.hmax, s.vmax)[: s.height, : s.width] for p in planes[1:])
        want[dataset.JPEG_GRAY_BGR] = jo.cv_luma(jo.ycc_to_rgb(planes[0], cb, cr))
        host_color = time.perf_counter() - t2
    result["host_numpy_one_core"] = {"entropy_python_s": t1 - t0, "idct_all_components_s": t2 - t1, "upsample_colour_luma_s": host_color}

    for label, mode in (("luma", dataset.JPEG_GRAY_LUMA), ("bgr", dataset.JPEG_GRAY_BGR)):
        out = np.empty((height, width), dtype=np.uint8)
        p = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        phases, wall = [], []
        for k in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            _lib.check(lib.nidreg_jpeg_decode_gray(0, data, len(data), mode, p, width), "nidreg_jpeg_decode_gray")
            dt = time.perf_counter() - t0
            ms = (ctypes.c_double * 4)()
            lib.nidreg_jpeg_get_timing(ms)
            if k >= args.warmup:
                phases.append(list(ms))
                wall.append(dt * 1e3)
        med = np.median(np.asarray(phases), axis=0)
        case = {"total_ms_median": float(np.median(wall)), "entropy_host_ms": float(med[0]), "alloc_upload_ms": float(med[1]), "kernels_ms": float(med[2]), "copy_back_ms": float(med[3]),
                "same_as_host_numpy": bool(np.array_equal(out, want[mode]))}
        if Image is not None:
            secs = []
            for k in range(args.warmup + args.calls):
                t0 = time.perf_counter()
                im = Image.open(io.BytesIO(data))
                if mode == dataset.JPEG_GRAY_LUMA:
                    im.draft("L", im.size)
                    ref = np.asarray(im)
                else:
                    ref = jo.cv_luma(np.asarray(im.convert("RGB")))
                if k >= args.warmup:
                    secs.append(time.perf_counter() - t0)
            case.update(pillow_ms_median=float(np.median(secs) * 1e3), same_as_pillow=bool(np.array_equal(out, ref)),
                        pillow_note="libjpeg-turbo SIMD on one host core" + ("" if mode == dataset.JPEG_GRAY_LUMA else "; includes the numpy luma of the RGB image"))
        if not case["same_as_host_numpy"] or not case.get("same_as_pillow", True):
            raise SystemExit(f"jpeg_time: the device's image differs from a reference in mode {label}: {case}")
        result["modes"][label] = case
        print(json.dumps({label: case}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
