#!/usr/bin/env python3
"""Writes tests/golden/eval_stage_parent_bits.npz: what the evaluation's serial stages (histogram flush, k_entropy, the gradient
kernel's prologue, the finalising workgroup) return for small clouds, BIT FOR BIT, as computed by the library this script is run
with.  Run it on the GPU with the build of the commit whose bits are to be kept (check that commit out and build it, or point
NIDREG_LIB at its libnidreg.so); tests/test_eval_stages_gpu.py then holds every later build to those bits.

The fixture carries its own inputs (float32 points and intensities, one 64x48 8-bit image, the cameras, the poses) and, for every
case, pose and want_grad: cost, 7-gradient, ok, inlier count and SHA-256 digests of the raw histogram words (the fixed-point joint
table of nidreg_get_hist_fixed and the three double arrays of nidreg_get_hist; the words themselves would be 0.5 MB per 256-bin
evaluation).  Multi-pair groups: the summed cost / gradient of nidreg_eval_multi (its gradient follows the group's chunk table).

Usage: make_eval_stage_golden.py [--out FILE] [--inputs-only]"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 64, 48
POINT_COUNTS = (1, 63, 64, 65, 257, 1023, 4097)
BINS = (16, 64, 256, 300)
CAMERAS = {
    "plumb_bob": ([40.0, 40.0, 32.0, 24.0], [-0.05, 0.01, 0.001, -0.001, 0.0]),
    "fisheye": ([45.0, 45.0, 32.0, 24.0], [0.01, -0.002, 0.0005, 0.0]),
}
# the order of the seven evaluations a handle runs in the test: pose index, want_grad
SEQUENCE = ((0, 1), (1, 0), (2, 1), (0, 1), (1, 0), (2, 0), (1, 1))
# pairs of cases evaluated as one multi-pair group (same camera, image size and bins)
MULTI = (("mixed_plumb_bob_b16_n1023", "mixed_plumb_bob_b16_n257"), ("mixed_plumb_bob_b256_n4097", "mixed_plumb_bob_b256_n1023"),
         ("mixed_plumb_bob_b64_n1023", "onecol_plumb_bob_b64_n1023"))


def case_list():
    cases = []
    for b in BINS:
        for n in POINT_COUNTS:
            cases.append(("mixed", "plumb_bob", b, n))
    cases += [("mixed", "fisheye", 16, 1023), ("mixed", "fisheye", 256, 1023), ("mixed", "fisheye", 64, 4097)]
    cases += [("inside", "plumb_bob", 16, 1023), ("inside", "plumb_bob", 256, 1023)]
    cases += [("none", "plumb_bob", 16, 257), ("none", "plumb_bob", 64, 257), ("none", "plumb_bob", 256, 257)]
    cases += [("onecol", "plumb_bob", 16, 1023), ("onecol", "plumb_bob", 64, 1023), ("onecol", "plumb_bob", 256, 1023), ("onecol", "plumb_bob", 256, 4097)]
    return [{"name": f"{s}_{m}_b{b}_n{n}", "scenario": s, "model": m, "bins": b, "n": n} for s, m, b, n in cases]


def build_inputs():
    """Seeded float32 clouds in the camera's frame (the poses are small perturbations of the identity)."""
    rng = np.random.default_rng(20240611)
    hx, hy = 32.0 / 40.0, 24.0 / 40.0  # half extents of the image in normalised plumb_bob coordinates

    def cloud(n, fx_lo, fx_hi, fy_lo, fy_hi):
        z = rng.uniform(2.0, 10.0, n)
        x = rng.uniform(fx_lo, fx_hi, n) * z
        y = rng.uniform(fy_lo, fy_hi, n) * z
        return np.stack([x, y, z], axis=1).astype(np.float32)

    n_max = max(POINT_COUNTS)
    head = cloud(65, -0.8 * hx, 0.8 * hx, -0.8 * hy, 0.8 * hy)  # the smallest clouds hold inliers
    rest = cloud(n_max - 65, -1.054 * hx, 1.054 * hx, -1.054 * hy, 1.054 * hy)  # about 10 % of these project outside the image
    levels = rng.integers(0, 256, n_max)
    yy, xx = np.mgrid[0:H, 0:W]
    image = np.clip(96.0 + 1.5 * xx + 1.0 * yy + 40.0 * np.sin(0.35 * xx) * np.cos(0.27 * yy) + rng.normal(0.0, 12.0, (H, W)), 0, 255).astype(np.uint8)
    poses = []
    for _ in range(3):
        q = rng.uniform(-0.01, 0.01, 3)
        poses.append(np.concatenate([q, [np.sqrt(1.0 - float(q @ q))], rng.uniform(-0.02, 0.02, 3)]))
    inp = {
        "image": image,
        "poses": np.array(poses, dtype=np.float64),
        "pts_mixed": np.concatenate([head, rest]),
        "int_mixed": (levels / 255.0).astype(np.float32),
        "pts_inside": cloud(1023, -0.8 * hx, 0.8 * hx, -0.8 * hy, 0.8 * hy),
        "int_inside": (rng.integers(0, 256, 1023) / 255.0).astype(np.float32),
        "pts_none": cloud(257, 3.0, 4.0, -0.5, 0.5),  # far to the right of the image for every pose
        "int_none": (rng.integers(0, 256, 257) / 255.0).astype(np.float32),
    }
    for m, (intr, dist) in CAMERAS.items():
        inp[f"cam_{m}_intr"] = np.array(intr, dtype=np.float64)
        inp[f"cam_{m}_dist"] = np.array(dist, dtype=np.float64)
    return inp


def make_cost(nid, inp, case, **tuning):
    """The handle of one case from the fixture's own inputs (shared with the test)."""
    n = case["n"]
    m = case["model"]
    proj = nid.create_camera(m, list(inp[f"cam_{m}_intr"]), list(inp[f"cam_{m}_dist"]))
    pts = np.ones((n, 4), dtype=np.float64)
    if case["scenario"] == "onecol":  # the mixed cloud with every point in one intensity column
        pts[:, :3] = inp["pts_mixed"][:n].astype(np.float64)
        ints = np.full(n, float(np.float32(128.0 / 255.0)))
    else:
        pts[:, :3] = inp[f"pts_{case['scenario']}"][:n].astype(np.float64)
        ints = inp[f"int_{case['scenario']}"][:n].astype(np.float64)
    img = inp["image"].astype(np.float64) * (1.0 / 255.0)
    return nid.NIDCost(proj, img, pts, ints, case["bins"], device=0, **tuning)


def hist_record(cost):
    """(inlier count, digest of the fixed-point joint words, digest of the double histograms) of the handle's last evaluation."""
    joint_fixed, inliers, frac = cost.histogram_fixed()
    joint, hi, hp = cost.histograms()
    d_fixed = hashlib.sha256(np.ascontiguousarray(joint_fixed).tobytes() + bytes([frac & 0xFF])).digest()
    d_f64 = hashlib.sha256(np.ascontiguousarray(joint).tobytes() + np.ascontiguousarray(hi).tobytes() + np.ascontiguousarray(hp).tobytes()).digest()
    return int(inliers), np.frombuffer(d_fixed, dtype=np.uint8), np.frombuffer(d_f64, dtype=np.uint8)


def evaluate(cost, x, want_grad):
    """One synchronous evaluation -> (cost, grad7 (zeros when not asked for), ok, inliers, digest, digest)."""
    ok, c, g = cost(x, want_grad=bool(want_grad))
    inl, d_fixed, d_f64 = hist_record(cost)
    return np.float64(c), (np.asarray(g, dtype=np.float64) if want_grad else np.zeros(7)), bool(ok), inl, d_fixed, d_f64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "eval_stage_parent_bits.npz"))
    ap.add_argument("--inputs-only", action="store_true", help="build and print the inputs' shapes, evaluate nothing (needs no GPU)")
    args = ap.parse_args()
    inp = build_inputs()
    cases = case_list()
    if args.inputs_only:
        print({k: (v.shape, str(v.dtype)) for k, v in inp.items()}, len(cases), "cases")
        return
    from direct_visual_lidar_calibration_amd import _lib, nid

    out = dict(inp)
    out["cases"] = np.array(json.dumps(cases))
    out["multi"] = np.array(json.dumps(MULTI))
    out["kernel_build"] = np.array(_lib.library_kernel_build())
    by_name = {c["name"]: c for c in cases}
    # results, indexed [case][pose][want_grad]
    C = len(cases)
    r_cost, r_grad = np.zeros((C, 3, 2)), np.zeros((C, 3, 2, 7))
    r_ok, r_inl = np.zeros((C, 3, 2), dtype=np.int8), np.zeros((C, 3, 2), dtype=np.int64)
    r_dfixed, r_df64 = np.zeros((C, 3, 2, 32), dtype=np.uint8), np.zeros((C, 3, 2, 32), dtype=np.uint8)
    for i, case in enumerate(cases):
        cost = make_cost(nid, inp, case)
        for p in range(3):
            for wg in (1, 0):
                r_cost[i, p, wg], r_grad[i, p, wg], r_ok[i, p, wg], r_inl[i, p, wg], r_dfixed[i, p, wg], r_df64[i, p, wg] = evaluate(cost, inp["poses"][p], wg)
        cost.close()
    out.update(r_cost=r_cost, r_grad=r_grad, r_ok=r_ok, r_inl=r_inl, r_dfixed=r_dfixed, r_df64=r_df64)
    # multi-pair groups, indexed [group][pose][want_grad]
    m_cost, m_grad, m_ok = np.zeros((len(MULTI), 3, 2)), np.zeros((len(MULTI), 3, 2, 7)), np.zeros((len(MULTI), 3, 2), dtype=np.int8)
    for i, (a, b) in enumerate(MULTI):
        hs = [make_cost(nid, inp, by_name[a]), make_cost(nid, inp, by_name[b])]
        multi = nid.MultiNIDCost(None)
        for h_ in hs:
            multi.add(h_)
        for p in range(3):
            for wg in (1, 0):
                ok, c, g = multi(inp["poses"][p], want_grad=bool(wg))
                m_cost[i, p, wg], m_ok[i, p, wg] = c, int(ok)
                if wg:
                    m_grad[i, p, wg] = g
        for h_ in hs:
            h_.close()
    out.update(m_cost=m_cost, m_grad=m_grad, m_ok=m_ok)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(cases)} cases, kernel build {out['kernel_build']}")


if __name__ == "__main__":
    main()
