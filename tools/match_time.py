#!/usr/bin/env python3
"""Times nidreg_features_detect (a 1920 x 1080 image) and nidreg_features_match (2048 x 2048 and 8192 x 8192 descriptors) against the
numpy restatement of tests/matching_oracle.py on one host core, and measures find_matches end to end on the scene of
tests/find_matches_scene.py.  Writes profiles/find_matches.json (--out); README.md and DESIGN.md quote only what that file holds.

Timing: the host clock around each blocking call -- upload, kernels, copy back, as a caller sees it: median of --calls calls
(default 50) after --warmup calls.  A plain script, not part of the test or bench contract.

End to end (--skip_e2e leaves it out): the matcher's counts at the defaults (keypoints, accepted, correct = within
--ransac_error_thresh of the 3D point's projection under the true pose) and over a small grid around them; the pose error
initial_guess_auto reaches from the matcher's file and from GROUND-TRUTH matches of the same LiDAR keypoints (the yardstick);
where calibrate ends from three starts (ground-truth-match guess, the scene's own initial guess, the matcher's guess).

    python tools/match_time.py [--out profiles/find_matches.json] [--calls 50] [--warmup 3] [--skip_host] [--skip_e2e]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import find_matches_scene as fms  # noqa: E402  (test infrastructure: the scene and its bookkeeping)
import matching_oracle as mo  # noqa: E402  (test infrastructure: the host restatement)
from direct_visual_lidar_calibration_amd import find_matches, matching, se3, synth  # noqa: E402


def timed(fn, calls, warmup):
    secs = []
    for k in range(warmup + calls):
        t0 = time.perf_counter()
        out = fn()
        if k >= warmup:
            secs.append(time.perf_counter() - t0)
    return out, {"ms_median": 1e3 * float(np.median(secs)), "ms_min": 1e3 * float(np.min(secs)), "ms_max": 1e3 * float(np.max(secs)), "calls": calls}


def timing(args):
    out = {"calls": args.calls, "warmup": args.warmup, "cases": []}
    img = synth.make_scene("pinhole_1080p", num_points=1000, seed=3).image_u8
    (k, d), t = timed(lambda: matching.detect_features(img, max_keypoints=2048), args.calls, args.warmup)
    case = {"what": "detect 1920x1080, 8 levels, 2048 keypoints kept", "keypoints": int(k.shape[0]), "device_call": t}
    if not args.skip_host:
        t0 = time.perf_counter()
        kh, dh = mo.detect(img, max_keypoints=2048)
        case.update(host_numpy_one_core_ms=1e3 * (time.perf_counter() - t0), equal_to_host=bool(np.array_equal(k, kh) and np.array_equal(d, dh)))
    out["cases"].append(case)
    print(json.dumps(case))
    rng = np.random.default_rng(5)
    for n in (2048, 8192):
        d1 = rng.integers(0, 2**32, (n, 8), dtype=np.uint64).astype(np.uint32)
        d0 = d1[rng.permutation(n)] ^ (np.uint32(1) << rng.integers(0, 32, (n, 8)).astype(np.uint32))  # every row 8 bits from one column
        (m, b, s), t = timed(lambda: matching.match_features(d0, d1), args.calls, args.warmup)
        case = {"what": f"match {n} x {n} descriptors", "accepted": int((m >= 0).sum()), "device_call": t}
        if not args.skip_host:
            t0 = time.perf_counter()
            mh, bh, sh = mo.match(d0, d1, max_distance=matching.MAX_DISTANCE, ratio_num=4, ratio_den=5)
            case.update(host_numpy_one_core_ms=1e3 * (time.perf_counter() - t0), equal_to_host=bool(np.array_equal(m, mh) and np.array_equal(b, bh) and np.array_equal(s, sh)))
        out["cases"].append(case)
        print(json.dumps(case))
    return out


def counts(s, idx, result):
    k0, k1, m = np.array(result["kpts0"]).reshape(-1, 2), np.array(result["kpts1"]).reshape(-1, 2), np.array(result["matches"])
    sel = np.flatnonzero(m >= 0)
    err = fms.reprojection_error(s, k0[sel], s.points[idx[k1[m[sel], 1], k1[m[sel], 0]]])
    return {"camera_keypoints": int(len(k0)), "lidar_keypoints": int(len(k1)), "accepted": int(len(sel)), "correct": int((err < fms.RANSAC_THRESH).sum())}


def end_to_end():
    s = fms.scene()
    inten, idx = fms.render_lidar(s, device=0)
    lid = fms.intensities_u8(inten)
    out = {"scene": {"camera": fms.CAMERA, "seed": fms.SEED, "points": fms.NUM_POINTS, "lidar_image": [fms.LIDAR_SIZE, fms.LIDAR_SIZE], "lidar_fov_deg": fms.LIDAR_FOV_DEG,
                     "blank_fraction": float((idx < 0).mean())},
           "correct_within_px": fms.RANSAC_THRESH,
           "defaults": {"fast_threshold": matching.FAST_THRESHOLD, "max_distance": matching.MAX_DISTANCE, "ratio": matching.RATIO, "max_keypoints": matching.MAX_KEYPOINTS,
                        "nms_radius": matching.NMS_RADIUS, "levels": matching.LEVELS, "fill_passes": matching.FILL_PASSES}}
    grid = []
    for thr in (10, 20, 40):
        for maxd in (48, 64, 96):
            for ratio in (0.7, 0.8, 0.9):
                r = matching.find_matches(s.image_u8, lid, idx >= 0, fast_threshold=thr, max_distance=maxd, ratio=ratio)
                grid.append(dict(fast_threshold=thr, max_distance=maxd, ratio=ratio, **counts(s, idx, r)))
    out["grid"] = grid
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "data")
        fms.write_directory(d, s, inten, idx)
        find_matches.main([d])
        result = fms.read_matches(d)
        host = matching.find_matches(s.image_u8, lid, idx >= 0, detect=mo.detect, match=mo.match)
        out["at_defaults"] = dict(counts(s, idx, result), equal_to_host=bool(host == result))
        g = fms.initial_guess(d, s)
        out["matcher"] = {"dt_m": g["dt"], "dr_rad": g["dr"], "correspondences": int(len(g["err"])), "ransac_inliers": int(g["inliers"].sum()),
                          "ransac_inliers_incorrect": int((g["err"][g["inliers"]] >= fms.RANSAC_THRESH).sum()), "worst_inlier_error_px": float(g["err"][g["inliers"]].max())}
        x_matcher = g["x"]
        fms.write_matches(d, fms.ground_truth_matches(s, idx, np.array(result["kpts1"]).reshape(-1, 2)))
        y = fms.initial_guess(d, s)
        out["yardstick_ground_truth_matches"] = {"dt_m": y["dt"], "dr_rad": y["dr"], "correspondences": int(len(y["err"])), "ransac_inliers": int(y["inliers"].sum())}
        t0 = time.perf_counter()
        x_gt = fms.run_calibrate(d)  # calib.json holds the ground-truth-match guess now
        out["calibrate_seconds"] = time.perf_counter() - t0
        fms.set_manual_guess(d, s.T_camera_lidar_init)
        x_init = fms.run_calibrate(d)
        fms.set_manual_guess(d, x_matcher)
        x_m = fms.run_calibrate(d)
        names = {"from_ground_truth_guess": x_gt, "from_scene_init": x_init, "from_matcher_guess": x_m}
        out["calibrate"] = {k: dict(zip(("dt_truth_m", "dr_truth_rad"), se3.delta_trans_rot(s.T_camera_lidar_true, v))) for k, v in names.items()}
        out["calibrate"]["existing_code_distance"] = dict(zip(("dt_m", "dr_rad"), se3.delta_trans_rot(x_gt, x_init)))
        out["calibrate"]["matcher_to_ground_truth_distance"] = dict(zip(("dt_m", "dr_rad"), se3.delta_trans_rot(x_gt, x_m)))
    print(json.dumps({k: v for k, v in out.items() if k != "grid"}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "find_matches.json"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip_host", action="store_true")
    ap.add_argument("--skip_e2e", action="store_true")
    args = ap.parse_args()
    if args.calls < 50:
        ap.error("--calls must be at least 50")
    result = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            result = json.load(f)  # (the hand-written notes of the file -- the bars and their reasons -- are kept)
    result["timing"] = timing(args)
    if not args.skip_e2e:
        result["end_to_end"] = end_to_end()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
