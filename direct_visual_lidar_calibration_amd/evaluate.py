"""``evaluate``: how repeatable is the result of ``calibrate`` on this data?  (An extension: the reference has no such tool, and at
13.8-15.1 s a calibration on the CPU it could not afford one.)

    python -m direct_visual_lidar_calibration_amd.evaluate <data_path> [calibrate's options] [--dst_path DIR] [--seed 0]
        [--folds 8] [--fold_cell 1.0] [--fold_mode jackknife|subset] [--restarts 16] [--restart_trans 0.05] [--restart_rot_deg 1.0]
        [--agree_trans 0.01] [--agree_rot_deg 0.1] [--no_leave_one_out] [--sweep_steps 41] [--sweep_trans 0.05] [--sweep_rot_deg 1.0]

Reads the directory and the initial guess as ``calibrate`` does, uploads every pair once and recalibrates a few dozen times on the
device-resident clouds; writes ``evaluate.json`` to ``--dst_path`` and never touches ``calib.json``.

* ``full``: the calibration ``calibrate`` would run.  ``stored_vs_full``: its distance to ``results.T_lidar_camera``, if stored.
* ``folds``: every pair's cloud is cut into K folds on the device (``nid.Cloud.fold``: a hash of the point's ``--fold_cell`` cube, or
  of its index with ``--fold_cell 0``; pair ``p`` uses seed ``--seed + p``).  Replicate k calibrates, from the same initial guess, on
  everything but fold k (``jackknife``) or on fold k alone (``subset``).  ``d`` of a replicate = [translation of its
  ``T_lidar_camera`` minus ``full``'s, rotation vector of ``R_full^T R_k``].  In jackknife mode ``se`` = sqrt((K-1)/K sum_k (d_k -
  mean d)^2) per component.  Folds of unequal size make the jackknife approximate, and the points of a map are spatially correlated:
  block folds reduce that, they do not remove it, so ``se`` is a LOWER BOUND on the error, not the error.
* ``leave_one_out``: one replicate per bag, on the other bags' clouds (needs two bags).
* ``restarts``: replicate r starts from ``Exp(rho u, phi w) * T_camera_lidar(full)`` -- the pose with translation ``rho u`` and
  rotation ``exp(phi w)`` applied on the left, in the camera frame -- with ``u``, ``w`` the normalised halves of
  ``default_rng([seed, r]).standard_normal(6)``; reported is where each ends and the share that ends within ``--agree_trans`` /
  ``--agree_rot_deg`` of ``full``.
* ``sweeps``: the cost along tx ty tz rx ry rz of such a left perturbation around ``full``, on cost objects built once at ``full`` by
  the factory of the outer iterations; per axis the deltas, the costs, the index of the minimum and whether it is interior.  No plot.

Every section carries its wall time under ``seconds``; apart from those keys two runs with the same arguments write the same file.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

from . import _lib, calibrate, dataset, se3

AXES = ("tx", "ty", "tz", "rx", "ry", "rz")
CAVEAT = ("folds of unequal size make the jackknife approximate; points of a map are spatially correlated: block folds reduce that, they do not remove it, "
          "so se is a lower bound on the error, not the error")


def build_parser():
    p = argparse.ArgumentParser(prog="evaluate", description="repeatability of a calibration over folds, bags and restarts")
    p.add_argument("data_path", help="directory that contains preprocessed data")
    p.add_argument("--first_n_bags", type=int, default=None, help="use only the first N bags")
    p.add_argument("--disable_culling", action="store_true", help="disable depth buffer-based hidden points removal")
    p.add_argument("--nid_bins", type=int, default=16, help="Number of histogram bins for NID")
    p.add_argument("--registration_type", default="nid_bfgs", help="nid_bfgs or nid_nelder_mead")
    p.add_argument("--nelder_mead_init_step", type=float, default=1e-3, help="Nelder-mead initial step size")
    p.add_argument("--nelder_mead_convergence_criteria", type=float, default=1e-8, help="Nelder-mead convergence criteria")
    dataset.add_selection_options(p)
    p.add_argument("--dst_path", default=None, help="where evaluate.json goes (default: data_path)")
    p.add_argument("--seed", type=int, default=0, help="seed of the folds and the restarts")
    p.add_argument("--folds", type=int, default=8, help="folds per cloud, 2..64 (0: skip)")
    p.add_argument("--fold_cell", type=float, default=1.0, help="edge of the cubes that are folded as one [m] (0: per-point folds)")
    p.add_argument("--fold_mode", default="jackknife", choices=["jackknife", "subset"], help="calibrate on everything but fold k, or on fold k alone")
    p.add_argument("--restarts", type=int, default=16, help="recalibrations from perturbed starts (0: skip)")
    p.add_argument("--restart_trans", type=float, default=0.05, help="translation of a restart's perturbation [m]")
    p.add_argument("--restart_rot_deg", type=float, default=1.0, help="rotation of a restart's perturbation [deg]")
    p.add_argument("--agree_trans", type=float, default=0.01, help="a restart agrees with the full calibration within this [m] ...")
    p.add_argument("--agree_rot_deg", type=float, default=0.1, help="... and this [deg]")
    p.add_argument("--no_leave_one_out", action="store_true", help="skip the leave-one-bag-out replicates")
    p.add_argument("--sweep_steps", type=int, default=41, help="samples per axis of the cost sweeps, odd and >= 3 (0: skip)")
    p.add_argument("--sweep_trans", type=float, default=0.05, help="half width of the translation sweeps [m]")
    p.add_argument("--sweep_rot_deg", type=float, default=1.0, help="half width of the rotation sweeps [deg]")
    p.add_argument("--device", type=int, default=None, help="put every pair on this GPU (default: pair k on GPU k mod the visible ones, as calibrate)")
    return p


def check_args(args):
    """Host checks, before a device is touched (SystemExit with one line each)."""
    if args.folds != 0 and not 2 <= args.folds <= 64:
        raise SystemExit("error: --folds must be 0 or lie in [2, 64]")
    if not (args.fold_cell >= 0.0) or math.isinf(args.fold_cell):
        raise SystemExit("error: --fold_cell must be finite and >= 0")
    if args.sweep_steps != 0 and (args.sweep_steps < 3 or args.sweep_steps % 2 == 0):
        raise SystemExit("error: --sweep_steps must be 0 or odd and >= 3")
    if args.restarts < 0:
        raise SystemExit("error: --restarts must be >= 0")
    for name in ("restart_trans", "restart_rot_deg", "agree_trans", "agree_rot_deg", "sweep_trans", "sweep_rot_deg"):
        v = getattr(args, name)
        if not (v >= 0.0) or math.isinf(v):
            raise SystemExit(f"error: --{name} must be finite and >= 0")
    if args.device is not None and args.device < 0:
        raise SystemExit("error: --device must be >= 0")


# ---- poses
def left_perturbed(x, trans, rotvec):
    """``Exp(trans, rotvec) * x``: the 7-vector ``x`` (``T_camera_lidar``) with the rotation ``exp(rotvec)`` and then the translation
    ``trans`` applied on the left, in the camera frame"""
    d = np.concatenate([se3.so3_exp_quat(np.asarray(rotvec, dtype=np.float64)), np.asarray(trans, dtype=np.float64)])
    return se3.compose(d, np.asarray(x, dtype=np.float64))


def restart_direction(seed, r):
    """``(u, w)``: the normalised first and second triple of ``default_rng([seed, r]).standard_normal(6)``"""
    g = np.random.default_rng([int(seed), int(r)]).standard_normal(6)
    return g[:3] / np.linalg.norm(g[:3]), g[3:] / np.linalg.norm(g[3:])


def restart_pose(x_full, seed, r, trans, rot_deg):
    u, w = restart_direction(seed, r)
    return left_perturbed(x_full, trans * u, math.radians(rot_deg) * w)


def sweep_deltas(steps, amplitude):
    """``delta_j = (j - (S - 1) / 2) * 2 A / (S - 1)``: symmetric, the centre sample exactly 0"""
    return [(j - (steps - 1) // 2) * (2.0 * amplitude / (steps - 1)) for j in range(steps)]


def sweep_pose(x_full, axis, delta):
    if delta == 0.0:  # the centre sample is the pose itself, not its re-normalised product with the identity
        return np.asarray(x_full, dtype=np.float64).copy()
    v = np.zeros(6)
    v[axis] = delta
    return left_perturbed(x_full, v[:3], v[3:])


def pose_delta(x_full, x):
    """``d`` = [translation of ``T_lidar_camera(x)`` minus ``T_lidar_camera(x_full)``'s, rotation vector of ``R_full^T R``] (6 floats)"""
    a, b = se3.to_matrix(se3.inverse(np.asarray(x_full, dtype=np.float64))), se3.to_matrix(se3.inverse(np.asarray(x, dtype=np.float64)))
    return [float(v) for v in np.concatenate([b[:3, 3] - a[:3, 3], se3.rot3_logmap(a[:3, :3].T @ b[:3, :3])])]


# ---- summaries
def maxima(ds):
    """largest |d| in translation and in rotation over the replicates' ``d`` (None entries: failed replicates, left out)"""
    ds = np.array([d for d in ds if d is not None], dtype=np.float64).reshape(-1, 6)
    if len(ds) == 0:
        return None, None
    return float(np.linalg.norm(ds[:, :3], axis=1).max()), float(np.linalg.norm(ds[:, 3:], axis=1).max())


def jackknife_se(ds):
    """``(mean d, se)`` per component: ``se = sqrt((K - 1) / K * sum_k (d_k - mean d)^2)``"""
    ds = np.array(ds, dtype=np.float64).reshape(-1, 6)
    K = len(ds)
    mean = ds.mean(axis=0)
    se = np.sqrt((K - 1) / K * ((ds - mean) ** 2).sum(axis=0))
    return [float(v) for v in mean], [float(v) for v in se]


# ---- the run
def _replicate(proj, images, clouds, start_x, params, sel, x_full, log, what, after=None):
    """one calibration on ``clouds`` (the caller's); a replicate that cannot be evaluated is reported, not fatal"""
    entry = {}
    pairs = [(im, None, None) for im in images]
    try:
        x, cal = calibrate.calibrate_pairs(proj, pairs, start_x, params, selection=sel, clouds=clouds, after=after)
    except RuntimeError as e:
        entry.update(T_lidar_camera=None, d=None, final_cost=None, evaluations=0, error=str(e))
        log(f"{what}: failed: {e}")
        return None, entry
    entry.update(T_lidar_camera=dataset.T_camera_lidar_to_tum(x), final_cost=float(cal.log[-1]["final_cost"]), evaluations=int(sum(e.get("evaluations", 0) for e in cal.log)),
                 outer_iterations=len(cal.log))
    if x_full is not None:
        entry["d"] = pose_delta(x_full, x)
        log(f"{what}: cost {entry['final_cost']:.6f}, {entry['evaluations']} evaluations, |dt| {np.linalg.norm(entry['d'][:3]):.5f} m, "
            f"|dr| {math.degrees(np.linalg.norm(entry['d'][3:])):.4f} deg from full")
    return x, entry


def _sub_selection(sel, keep):
    if sel is None:
        return None
    return dict(sel, masks=[sel["masks"][k] for k in keep])


def run(args, log=print):
    check_args(args)
    config, bags, proj, init_x, params, sel = calibrate.prepare(args, log)
    dst = args.dst_path or args.data_path
    ndev = _lib.load().nidreg_device_count()
    if ndev <= 0:
        raise SystemExit("error: no MI355X / HIP device visible (the NID core has no CPU fallback)")
    if args.device is not None and args.device >= ndev:
        raise SystemExit(f"error: --device {args.device}: {ndev} device(s) visible")
    images = [b.image for b in bags]
    t0 = time.perf_counter()
    clouds = [calibrate._upload(*((b.xyz_f32, b.intensities_f32) if b.xyz_f32 is not None else (b.points, b.intensities)), args.device if args.device is not None else k % ndev)
              for k, b in enumerate(bags)]
    out = {
        "arguments": {k: v for k, v in sorted(vars(args).items())},
        "bags": [b.bag_name for b in bags],
        "points": [c.num_points for c in clouds],
        "initial_guess": dataset.T_camera_lidar_to_tum(init_x),
        "upload": {"seconds": time.perf_counter() - t0},
    }

    # ---- full (and, inside it, the sweeps: on cost objects the factory of the outer iterations builds at the result)
    sweeps = {}

    def sweep(x_full, cal):
        if args.sweep_steps == 0:
            return
        t1 = time.perf_counter()
        T = se3.to_matrix(x_full)
        costs = [cal.fused_nid_factory(k, T, params.nid_bins) for k in range(len(clouds))]
        multi = calibrate._Multi(x_full, costs)
        ok, centre, _ = multi(x_full, want_grad=False)
        sweeps.update(steps=args.sweep_steps, centre_ok=bool(ok), centre_cost=float(centre), axes={})
        for a, name in enumerate(AXES):
            deltas = sweep_deltas(args.sweep_steps, args.sweep_trans if a < 3 else math.radians(args.sweep_rot_deg))
            vals = [multi(sweep_pose(x_full, a, d), want_grad=False) for d in deltas]
            cost = [float(v[1]) if v[0] and math.isfinite(v[1]) else None for v in vals]  # None: outside the trust gate / not finite
            valid = [j for j, c in enumerate(cost) if c is not None]
            j_min = min(valid, key=lambda j: cost[j]) if valid else None
            sweeps["axes"][name] = {"delta": deltas, "cost": cost, "argmin": j_min, "interior": j_min is not None and 0 < j_min < args.sweep_steps - 1}
            log(f"sweep {name}: minimum at delta {deltas[j_min]:+.5f} ({'interior' if sweeps['axes'][name]['interior'] else 'at the edge'})" if valid else f"sweep {name}: no valid sample")
        for c in costs:
            c.close()
        sweeps["seconds"] = time.perf_counter() - t1

    t0 = time.perf_counter()
    x_full, full = _replicate(proj, images, clouds, init_x, params, sel, None, log, "full", after=sweep)
    if x_full is None:
        raise SystemExit(f"error: the full calibration failed: {full['error']}")
    full["seconds"] = time.perf_counter() - t0 - sweeps.get("seconds", 0.0)
    log(f"full: cost {full['final_cost']:.6f}, {full['evaluations']} evaluations in {full['outer_iterations']} outer iterations")
    out["full"] = full
    stored = config.get("results", {}).get("T_lidar_camera")
    out["stored_vs_full"] = None
    if stored is not None:
        d = pose_delta(x_full, dataset.tum_to_T_camera_lidar(stored))
        out["stored_vs_full"] = {"d": d, "trans": float(np.linalg.norm(d[:3])), "rot": float(np.linalg.norm(d[3:]))}

    # ---- folds
    out["folds"] = None
    if args.folds:
        t0 = time.perf_counter()
        K, jack = args.folds, args.fold_mode == "jackknife"
        sec = {"mode": args.fold_mode, "num_folds": K, "cell": args.fold_cell, "note": CAVEAT,
               "sizes": [[int(v) for v in c.fold_ids(args.seed + p, K, args.fold_cell)[1]] for p, c in enumerate(clouds)], "replicates": []}
        for k in range(K):
            subs = [c.fold(args.seed + p, K, k, complement=jack, cell=args.fold_cell) for p, c in enumerate(clouds)]
            _, entry = _replicate(proj, images, subs, init_x, params, sel, x_full, log, f"fold {k} ({'without' if jack else 'only'}, {sum(s.num_points for s in subs)} points)")
            sec["replicates"].append(dict(fold=k, points=[s.num_points for s in subs], **entry))
            for s in subs:
                s.close()
        ds = [r["d"] for r in sec["replicates"]]
        sec["mean_d"], sec["se"] = jackknife_se(ds) if jack and all(d is not None for d in ds) else (None, None)
        sec["max_trans"], sec["max_rot"] = maxima(ds)
        sec["seconds"] = time.perf_counter() - t0
        out["folds"] = sec

    # ---- leave one bag out
    out["leave_one_out"] = None
    if not args.no_leave_one_out:
        if len(bags) < 2:
            log("leave one bag out: needs at least two bags, skipped")
        else:
            t0 = time.perf_counter()
            sec = {"replicates": []}
            for j, b in enumerate(bags):
                keep = [k for k in range(len(bags)) if k != j]
                _, entry = _replicate(proj, [images[k] for k in keep], [clouds[k] for k in keep], init_x, params, _sub_selection(sel, keep), x_full, log, f"without {b.bag_name}")
                sec["replicates"].append(dict(left_out=b.bag_name, **entry))
            sec["max_trans"], sec["max_rot"] = maxima([r["d"] for r in sec["replicates"]])
            sec["seconds"] = time.perf_counter() - t0
            out["leave_one_out"] = sec

    # ---- restarts
    out["restarts"] = None
    if args.restarts:
        t0 = time.perf_counter()
        sec = {"trans": args.restart_trans, "rot_deg": args.restart_rot_deg, "replicates": []}
        for r in range(args.restarts):
            start = restart_pose(x_full, args.seed, r, args.restart_trans, args.restart_rot_deg)
            _, entry = _replicate(proj, images, clouds, start, params, sel, x_full, log, f"restart {r}")
            d = entry["d"]
            agrees = d is not None and bool(np.linalg.norm(d[:3]) <= args.agree_trans and np.linalg.norm(d[3:]) <= math.radians(args.agree_rot_deg))
            sec["replicates"].append(dict(r=r, start_T_lidar_camera=dataset.T_camera_lidar_to_tum(start), agrees=agrees, **entry))
        sec["agree_share"] = sum(r["agrees"] for r in sec["replicates"]) / args.restarts
        sec["max_trans"], sec["max_rot"] = maxima([r["d"] for r in sec["replicates"]])
        sec["seconds"] = time.perf_counter() - t0
        log(f"restarts: {sec['agree_share'] * 100:.0f} % end within {args.agree_trans} m / {args.agree_rot_deg} deg of full")
        out["restarts"] = sec

    out["sweeps"] = sweeps or None
    for c in clouds:
        c.close()
    os.makedirs(dst, exist_ok=True)
    path = os.path.join(dst, "evaluate.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=2, sort_keys=True)
        f.write("\n")
    log(f"saved to {path}")
    return out


def main(argv=None):
    run(build_parser().parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
