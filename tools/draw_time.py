"""Times the match picture (draw.py / nidreg_draw) on the GPU and writes profiles/match_picture.json (--out): one measurement, nothing
tuned; README.md and DESIGN.md quote only what that file holds.  There is no earlier path to compare against and no bar to meet.

Workloads: a 1920 x 1080 camera image beside a 1024 x 1024 LiDAR image with
  match_picture  2048 + 2048 rings of radius 3 and 300 lines from a camera keypoint to a LiDAR keypoint (what find_matches --picture draws at its defaults);
  lines_65536    the same canvas with 65 536 such lines.
Recorded per workload: the time of one ``draw.draw`` call (upload, kernels, copy back; median of --calls), the kernels alone from HIP
events (tools/draw_kernel_time.hip, the same kernels and launch shapes outside the library, built with hipcc when its binary is
missing), and tests/draw_oracle.py on one host core next to them.  Register and LDS use: the compiler's resource remarks (--resources
compiles the kernels once more with -Rpass-analysis=kernel-resource-usage; no GPU needed).

    python tools/draw_time.py [--out profiles/match_picture.json] [--calls 20] [--warmup 3] [--skip_host]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
TOOLS = os.path.join(ROOT, "tools")
SRC, EXE = os.path.join(TOOLS, "draw_kernel_time.hip"), os.path.join(TOOLS, "draw_kernel_time.bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CW, CH, LW, LH = 1920, 1080, 1024, 1024


def build_exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(os.path.join(ROOT, "direct_visual_lidar_calibration_amd", "csrc", "nid_draw_kernels.hpp"))):
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", SRC, "-o", EXE])
    return EXE


def kernel_resources():
    """VGPRs, SGPRs, scratch, LDS and occupancy of the two kernels from the compiler's remarks"""
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Rpass-analysis=kernel-resource-usage", "-c", SRC, "-o", os.path.join(tmp, "x.o")], capture_output=True, text=True,
                           check=True)
    out, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: +(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = "k_draw_prims" if "k_draw_prims" in m.group(2) else "k_draw_compose" if "k_draw_compose" in m.group(2) else None
            if name:
                out[name] = {}
        elif name:
            out[name][m.group(1).split(" [")[0]] = int(m.group(2))
    return out


def workloads():
    from direct_visual_lidar_calibration_amd import draw

    rng = np.random.default_rng(0)
    camera = rng.integers(0, 256, (CH, CW), dtype=np.uint8)
    lidar = rng.integers(0, 256, (LH, LW), dtype=np.uint8)

    def result(n0, n1, matched):
        k0 = np.stack([rng.integers(0, CW, n0), rng.integers(0, CH, n0)], axis=1)
        k1 = np.stack([rng.integers(0, LW, n1), rng.integers(0, LH, n1)], axis=1)
        matches = np.full(n0, -1)
        rows = rng.choice(n0, size=matched, replace=False)
        matches[rows] = rng.integers(0, n1, matched)
        conf = np.where(matches >= 0, 1.0 - rng.integers(0, 65, n0) / 256.0, 0.0)
        return {"kpts0": k0.reshape(-1).tolist(), "kpts1": k1.reshape(-1).tolist(), "matches": matches.tolist(), "confidence": conf.tolist()}

    picture = draw.match_primitives(result(2048, 2048, 300), camera.shape, lidar.shape)
    many = [p for p in draw.match_primitives(result(65536, 2048, 65536), camera.shape, lidar.shape) if p[0] == draw.LINE]
    return camera, lidar, {"match_picture": picture, "lines_65536": many}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_picture.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip_host", action="store_true")
    ap.add_argument("--resources", action="store_true", help="only print the kernels' register and LDS use (no GPU)")
    args = ap.parse_args()
    if args.resources:
        print(json.dumps(kernel_resources(), indent=1))
        return 0
    import draw_oracle
    from direct_visual_lidar_calibration_amd import _lib, draw

    exe = build_exe()
    camera, lidar, cases = workloads()
    out = {"tool": "tools/draw_time.py", "library": _lib.load().nidreg_version().decode(), "canvas": [2 * CW, CH], "camera": [CW, CH], "lidar": [LW, LH], "calls": args.calls,
           "note": "one measurement, nothing tuned; no earlier path to compare against", "kernel_resources": kernel_resources(), "cases": {}}
    for name, prims in cases.items():
        for _ in range(args.warmup):
            got = draw.draw(camera, lidar, prims)
        times = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            got = draw.draw(camera, lidar, prims)
            times.append((time.perf_counter() - t0) * 1e3)
        case = {"primitives": len(prims), "lines": sum(1 for p in prims if p[0] == draw.LINE), "rings": sum(1 for p in prims if p[0] == draw.RING),
                "call_ms_median": float(np.median(times)), "call_ms_min": float(np.min(times))}
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "prims.bin")
            np.asarray(prims, dtype=np.int32).tofile(path)
            case["kernels_hip_events"] = json.loads(subprocess.check_output([exe, str(CW), str(CH), str(LW), str(LH), path, str(args.calls)], timeout=120).decode())
        if not args.skip_host:
            t0 = time.perf_counter()
            want = draw_oracle.draw(camera, lidar, prims)
            case["oracle_one_host_core_ms"] = (time.perf_counter() - t0) * 1e3
            case["equal_to_oracle"] = bool(np.array_equal(got, want))
        out["cases"][name] = case
        print(json.dumps({name: case}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
