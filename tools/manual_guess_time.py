#!/usr/bin/env python3
"""Measures the headless initial_guess_manual on the scene of tests/find_matches_scene.py (pinhole_vga, 1M points, a 512 x 512 ``lidar``
sheet) and writes profiles/initial_guess_manual.json (--out); README.md and DESIGN.md quote only what that file holds.

* the pose error against the truth of the estimate from the 24 hand picks of tests/manual_guess_scene.py (ground-truth projections
  rounded to integer pixels), and with one of them moved 200 px -- next to the bound the test holds them to, the matcher's guess error
  recorded in profiles/find_matches.json;
* the wall time of ``--candidates`` (24 culls, overlays and NIDs of the 1M points) and of one ``--sheets`` call (one view): the host
  clock around the command's ``run``, files included, once each.

Measured once, nothing tuned.  A plain script, not part of the test or bench contract.

    python tools/manual_guess_time.py [--out profiles/initial_guess_manual.json]
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
import manual_guess_scene as mgs  # noqa: E402  (test infrastructure: the 24 picks)
from direct_visual_lidar_calibration_amd import initial_guess_manual as igm, se3  # noqa: E402


def estimate(d, s, picks):
    assert igm.run(igm.parse_args([d] + [a for p in picks for a in ("--pick", p)]), log=lambda *_: None) == 0
    with open(os.path.join(d, "manual", "report.json")) as f:
        report = json.load(f)
    dt, dr = se3.delta_trans_rot(s.T_camera_lidar_true, se3.from_matrix(np.array(report["T_camera_lidar"]).reshape(4, 4)))
    residuals = [p["residual_px"] for p in report["picks"]]
    return {"dt_m": dt, "dr_rad": dr, "picks": len(residuals), "ransac_inliers": report["num_inliers"], "worst_inlier_residual_px": max(r for r, p in zip(residuals, report["picks"]) if p["ransac_inlier"]),
            "worst_residual_px": max(residuals)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "initial_guess_manual.json"))
    args = ap.parse_args()

    s = fms.scene()
    inten, idx = fms.render_lidar(s, device=0)
    with open(os.path.join(ROOT, "profiles", "find_matches.json")) as f:
        bound = json.load(f)["end_to_end"]["matcher"]
    out = {"scene": {"camera": fms.CAMERA, "seed": fms.SEED, "points": fms.NUM_POINTS, "lidar_image": [fms.LIDAR_SIZE, fms.LIDAR_SIZE]},
           "bound_matcher_guess": {"dt_m": bound["dt_m"], "dr_rad": bound["dr_rad"]}}
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "data")
        fms.write_directory(d, s, inten, idx)
        cam, lid, _ = mgs.grid_picks(s, idx)
        out["from_24_picks"] = estimate(d, s, mgs.pick_texts(cam, lid))
        out["with_one_pick_moved_200px"] = estimate(d, s, mgs.pick_texts(mgs.with_outlier(s, cam), lid))
        for name, action in (("sheets_one_view", ["--sheets"]), ("candidates", ["--candidates"])):
            parsed = igm.parse_args([d] + action)
            t0 = time.perf_counter()
            assert igm.run(parsed, log=lambda *_: None) == 0
            out[name + "_seconds"] = time.perf_counter() - t0
        with open(os.path.join(d, "manual", "candidates.json")) as f:
            entries = json.load(f)["candidates"]
        # reported, not claimed: where the mounting nearest the truth (candidate 0 on this scene) stands among the 24 by NID
        order = sorted(entries, key=lambda e: (e["nid_mean"] != e["nid_mean"], e["nid_mean"], e["k"]))
        out["candidates_by_nid"] = [{"k": e["k"], "facing": e["facing"], "roll": e["roll"], "nid_mean": e["nid_mean"] if e["nid_mean"] == e["nid_mean"] else None} for e in order]
    out["notes"] = ("No kernel is new: culling, the splat renderer, the NID and the rotation RANSAC are the ones the viewer and initial_guess_auto use. Wall times are the host clock "
                    "around the command, files included, once each. Measured once, nothing tuned. Picks made by a person on real data: unmeasured.")
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "candidates_by_nid"}, indent=1))


if __name__ == "__main__":
    main()
