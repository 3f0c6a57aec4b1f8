"""``viewer`` without a window: pictures and numbers that show whether the transform in ``calib.json`` is right.

    python -m direct_visual_lidar_calibration_amd.viewer <data_path> [--dst_path <data_path>/viewer]
        [--transformation last|all|result|init_manual|init_auto] [--blend_weight 0.7] [--point_radius 1] [--alpha 178]
        [--orbit_deg -30,-15,15,30] [--view_size 1280x720] [--view_fov 60] [--first_n_bags N] [--disable_culling]
        [--nid_bins 16] [--save_ply] [--device 0] [--mask PATH|auto] [--mask_margin 2] [--min_range 0] [--max_range inf]

The reference's sixth executable (src/viewer.cpp, ``VisualLiDARVisualizer``, ``PointsColorUpdater``) shows the cloud coloured by the
image under ``init_T_lidar_camera_auto``, ``init_T_lidar_camera`` or ``T_lidar_camera`` in a 3-D view the user turns: a wrong
extrinsic smears image colours onto the wrong surfaces when seen from the side.  Here the same comes out as files, per bag and per
selected transform:

* ``<bag>_<label>_overlay.png``   the camera image (grey) with the points the cost sees (``ViewCulling`` under that transform) drawn
  over it through the camera's own model, coloured by ``colormap_turbo(intensity)``;
* ``<bag>_<label>_orbit<k>.png``  the cloud coloured by ``PointsColorUpdater.update(T, blend_weight)``, seen by a distortion-free
  pinhole turned by the k-th angle of ``--orbit_deg`` about the camera's y axis through the centroid of the coloured points;
* ``<bag>_<label>_colored.ply``   (``--save_ply``) the cloud with those colours;
* ``viewer.json``                 point counts, covered pixels and the NID (``CostCalculatorNID`` on the culled cloud) per label and
  bag, and the summed NID per label -- "is the result better than the guess" as a number next to the pictures.

With ``--mask`` / ``--mask_margin`` / ``--min_range`` / ``--max_range`` (as in ``calibrate``) the overlay and the NID use the points
``nid.Cloud.select`` keeps -- cull, eroded mask at the point's pixel, range gate --, and the overlay shows the ignored pixels of the
eroded mask at half their grey value (``v >> 1``): what was left out is visible.  The orbit views keep the whole cloud.

Colouring, culling, the cost and the renderer (``render.SplatRenderer``) all run on the GPU.  Deliberate differences from the
reference: no window and no interaction; with no transform in ``calib.json`` the reference shows the identity under "NONE", this
prints the reference's error line and exits with status 1, writing nothing.
"""
import argparse
import json
import math
import os
import sys

import numpy as np

from . import dataset, nid, render

# viewer.cpp:49-74: the order the transforms are looked up in (the last one found is what the reference pre-selects, :83)
TRANSFORMS = (("init_auto", "init_T_lidar_camera_auto"), ("init_manual", "init_T_lidar_camera"), ("result", "T_lidar_camera"))
NO_TRANSFORM = "error: no transformation found in calib.json!!"  # viewer.cpp:78


def _floats(text):
    return [float(v) for v in text.split(",") if v.strip()]


def _size(text):
    w, h = text.lower().split("x")
    return int(w), int(h)


def build_parser():
    p = argparse.ArgumentParser(prog="viewer", description="viewer (headless)")
    p.add_argument("data_path", help="directory that contains preprocessed data")
    p.add_argument("--dst_path", default=None, help="where the pictures and viewer.json go (default: <data_path>/viewer)")
    p.add_argument("--transformation", default="last", choices=["last", "all"] + [t[0] for t in TRANSFORMS][::-1], help="which transform(s) of calib.json to show")
    p.add_argument("--blend_weight", type=float, default=0.7, help="weight of the image colour against the intensity colour in the orbit views")
    p.add_argument("--point_radius", type=int, default=1, help="a point covers (2 r + 1)^2 pixels")
    p.add_argument("--alpha", type=int, default=178, help="opacity (0..255) of the points over the camera image in the overlay")
    p.add_argument("--orbit_deg", type=_floats, default=[-30.0, -15.0, 15.0, 30.0], help="comma-separated angles of the orbit views")
    p.add_argument("--view_size", type=_size, default=(1280, 720), help="WxH of the orbit views")
    p.add_argument("--view_fov", type=float, default=60.0, help="horizontal field of view of the orbit views [deg]")
    p.add_argument("--first_n_bags", type=int, default=None, help="use only the first N bags")
    p.add_argument("--disable_culling", action="store_true", help="disable depth buffer-based hidden points removal")
    p.add_argument("--nid_bins", type=int, default=16, help="Number of histogram bins for NID")
    p.add_argument("--save_ply", action="store_true", help="also write the coloured cloud")
    p.add_argument("--device", type=int, default=0, help="GPU to run on")
    dataset.add_selection_options(p)
    return p


def parse_args(argv=None):
    """``build_parser().parse_args`` that also takes ``--orbit_deg -30,-15,15,30`` as written in the usage line: argparse alone reads a
    list that starts with a minus sign as an option."""
    argv = list(sys.argv[1:] if argv is None else argv)
    for i in range(len(argv) - 1):
        if argv[i] == "--orbit_deg":
            argv[i : i + 2] = ["--orbit_deg=" + argv[i + 1]]
            break
    return build_parser().parse_args(argv)


def tum_to_pose(values):
    """viewer.cpp:42-47: 4x4 pose of [tx ty tz qx qy qz qw]; the quaternion is taken as given (Eigen's toRotationMatrix)."""
    tx, ty, tz, x, y, z, w = (float(v) for v in values)
    T = np.eye(4)
    T[:3, :3] = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                 [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                 [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]
    T[:3, 3] = [tx, ty, tz]
    return T


def find_transforms(config):
    """viewer.cpp:49-74: ``[(label, T_lidar_camera 4x4), ...]`` of the transforms ``calib.json`` holds, in the reference's order."""
    res = config.get("results", {})
    return [(label, tum_to_pose(res[key])) for label, key in TRANSFORMS if key in res]


def select_transforms(found, which):
    """``last`` = the one the reference pre-selects (viewer.cpp:83), ``all``, or one label, which must be present."""
    if not found:
        raise SystemExit(NO_TRANSFORM)
    if which == "last":
        return found[-1:]
    if which == "all":
        return list(found)
    chosen = [f for f in found if f[0] == which]
    if not chosen:
        raise SystemExit(f"error: calib.json holds no '{which}' transformation (found: {', '.join(f[0] for f in found)})")
    return chosen


def view_camera(view_size, fov_deg):
    """The orbit views' camera: a distortion-free plumb_bob with the given horizontal field of view."""
    w, h = view_size
    f = 0.5 * w / math.tan(0.5 * math.radians(fov_deg))
    return nid.create_camera("plumb_bob", [f, f, 0.5 * w, 0.5 * h], [0.0, 0.0, 0.0, 0.0, 0.0])


def orbit_pose(T_camera_lidar, angle_deg, pivot_lidar):
    """``T_view_lidar`` of the camera turned by ``angle_deg`` about its own y axis through ``pivot_lidar`` (a LiDAR-frame point):
    the view keeps looking at the pivot from the same distance.  Angle 0 is the camera pose itself."""
    T = np.asarray(T_camera_lidar, dtype=np.float64).reshape(4, 4)
    if angle_deg == 0.0:
        return T.copy()
    c = T[:3, :3] @ np.asarray(pivot_lidar, dtype=np.float64)[:3] + T[:3, 3]
    a = math.radians(angle_deg)
    R = np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
    # pose of the view in the camera frame: x_camera = R (x_view - c) + c, hence x_view = R^T (x_camera - c) + c
    T_view_camera = np.eye(4)
    T_view_camera[:3, :3] = R.T
    T_view_camera[:3, 3] = c - R.T @ c
    return T_view_camera @ T


def overlay_and_nid(args, proj, bag, T_camera_lidar):
    """What one transform looks like on one bag's camera image, and its score: ``(overlay rgb (H, W, 3), its index image, the number
    of points the cost sees, NID)``.  The points are those ``ViewCulling`` keeps under the transform, drawn over the grey image through
    the camera's own model; the NID is ``CostCalculatorNID`` on the same points.  Reads ``args.disable_culling``, ``point_radius``,
    ``alpha``, ``nid_bins`` and ``device``.  ``initial_guess_manual --candidates`` shows its 24 mountings with this too.
    ``args.selection`` (``run`` sets it from the mask / range options; absent or ``None``: none given) narrows the points to
    ``nid.Cloud.select``'s and halves the grey value of the eroded mask's ignored pixels in the overlay."""
    size = (bag.image.shape[1], bag.image.shape[0])
    points, intensities = bag.points, bag.intensities
    sel = getattr(args, "selection", None)
    image = bag.image
    if sel is None:
        culling = nid.ViewCulling(proj, size, nid.ViewCullingParams(not args.disable_culling), device=args.device)
        keep = culling.cull(points, T_camera_lidar)
    else:
        mask_u8 = sel["masks"].get(bag.bag_name)
        mask = None if mask_u8 is None else nid.Mask(mask_u8, margin=sel["margin"], device=args.device)
        cloud = nid.Cloud(points, intensities, device=args.device)
        min_z = math.cos(nid.estimate_camera_fov(proj, size))  # view_culling.cpp:17, as nid.ViewCulling derives it
        sub, keep = cloud.select(proj, size, T_camera_lidar, min_z, not args.disable_culling, mask=mask, min_range=sel["min_range"], max_range=sel["max_range"], return_indices=True)
        sub.close()
        cloud.close()
        if mask is not None:
            image = np.where(mask.eroded() == 0, bag.image >> 1, bag.image).astype(np.uint8)
            mask.close()
    culled, culled_int = np.ascontiguousarray(points[keep]), np.ascontiguousarray(intensities[keep])
    grey = np.ascontiguousarray(np.repeat(image[:, :, None], 3, axis=2))
    r = render.SplatRenderer(culled, device=args.device)
    r.set_colors(render.quantize_colors(render.colormap_turbo(culled_int)))
    overlay, index = r.draw(proj, size, T_camera_lidar, radius=args.point_radius, background=grey, alpha=args.alpha)
    r.close()

    value = float("nan")  # (no point survives: there is nothing to score)
    if len(keep):
        cost = nid.CostCalculatorNID(proj, bag.image, culled, culled_int, nid.NIDCostParams(args.nid_bins), device=args.device)
        value = cost.calculate(T_camera_lidar)
        cost.close()
    return overlay, index, len(keep), value


def _bag_views(args, proj, bag, label, T_lidar_camera, dst, log):
    """The files of one bag under one transform; returns its entry of viewer.json."""
    T_camera_lidar = np.linalg.inv(T_lidar_camera)
    points, intensities = bag.points, bag.intensities
    overlay, index, num_culled, value = overlay_and_nid(args, proj, bag, T_camera_lidar)
    dataset.write_png(os.path.join(dst, f"{bag.bag_name}_{label}_overlay.png"), overlay)

    updater = render.PointsColorUpdater(proj, bag.image, points, intensities, device=args.device)
    colors = render.quantize_colors(updater.update(T_camera_lidar, args.blend_weight))
    updater.close()
    seen = colors[:, 3] > 0  # alpha 0: outside the image under this transform, not drawn
    pivot = points[seen, :3].mean(axis=0) if seen.any() else (points[:, :3].mean(axis=0) if len(points) else np.zeros(3))
    view_proj = view_camera(args.view_size, args.view_fov)
    r = render.SplatRenderer(np.ascontiguousarray(points[seen]), device=args.device)  # one upload serves every angle
    r.set_colors(colors[seen])
    for k, angle in enumerate(args.orbit_deg):
        rgb, _ = r.draw(view_proj, args.view_size, orbit_pose(T_camera_lidar, angle, pivot), radius=args.point_radius, background=None, alpha=255)
        dataset.write_png(os.path.join(dst, f"{bag.bag_name}_{label}_orbit{k}.png"), rgb)
    r.close()
    if args.save_ply:
        dataset.write_ply_colored(os.path.join(dst, f"{bag.bag_name}_{label}_colored.ply"), points, colors[:, :3])
    entry = {"points": int(len(points)), "culled": int(num_culled), "colored": int(seen.sum()), "overlay_pixels_covered": int((index >= 0).sum()), "nid": float(value)}
    log(f"{bag.bag_name} [{label}]: {entry['points']} points, {entry['culled']} after culling, {entry['overlay_pixels_covered']} overlay pixels, NID {value:.6f}")
    return entry


def run(args, log=print):
    config = dataset.read_calib(args.data_path)
    found = find_transforms(config)
    if not found:
        print(NO_TRANSFORM, file=sys.stderr)
        return 1
    for label, _ in found:
        log({"init_auto": "Automatic initial guess result found", "init_manual": "Manual initial guess result found", "result": "Calibration result found"}[label])
    selected = select_transforms(found, args.transformation)
    if not 0 <= args.alpha <= 255 or not 0 <= args.point_radius <= 8:
        raise SystemExit("error: --alpha must lie in [0, 255] and --point_radius in [0, 8]")

    sel = dataset.selection_options(args)
    config, bags = dataset.load_dataset(args.data_path, args.first_n_bags)
    model, intrinsics, distortion = dataset.camera_from_calib(config)
    proj = nid.create_camera(model, intrinsics, distortion)
    if proj is None:
        raise SystemExit(f"error: unknown camera model / wrong number of intrinsics: {model}")
    if sel is not None:
        sel["masks"] = {b.bag_name: dataset.load_mask(args.data_path, b.bag_name, sel["mask"], b.image.shape, log=log) for b in bags}
    args.selection = sel
    dst = args.dst_path or os.path.join(args.data_path, "viewer")
    os.makedirs(dst, exist_ok=True)

    report = {"data_path": args.data_path, "nid_bins": args.nid_bins, "culling": not args.disable_culling, "orbit_deg": list(args.orbit_deg), "transformations": {}}
    for label, T_lidar_camera in selected:
        per_bag = {bag.bag_name: _bag_views(args, proj, bag, label, T_lidar_camera, dst, log) for bag in bags}
        report["transformations"][label] = {"T_lidar_camera": [float(v) for v in T_lidar_camera.ravel()], "bags": per_bag, "nid_sum": float(sum(e["nid"] for e in per_bag.values()))}
    with open(os.path.join(dst, "viewer.json"), "w") as f:
        json.dump(report, f, indent=2, sort_keys=True)
        f.write("\n")
    log("--- summed NID ---")
    for label, _ in selected:
        log(f"{label:<12s} {report['transformations'][label]['nid_sum']:.6f}")
    log(f"saved to {dst}")
    return 0


def main(argv=None):
    return run(parse_args(argv))


if __name__ == "__main__":
    sys.exit(main())
