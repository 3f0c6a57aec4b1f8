"""``initial_guess_manual`` without a window: ``results.init_T_lidar_camera`` from a mounting picked by eye, a pose typed in, or
2D-3D pairs picked by hand in pictures this command writes.

    python -m direct_visual_lidar_calibration_amd.initial_guess_manual <data_path> ACTION [--dst_path <data_path>/manual]
        [--first_n_bags N] [--device 0]

    ACTION (exactly one):
      --candidates [--point_radius 1] [--alpha 178] [--nid_bins 16] [--disable_culling]
      --choose K
      --transform tx,ty,tz,qx,qy,qz,qw
      --sheets [--view default|candidate:K|current|panorama]... [--rotate_camera 0|90|180|270] [--point_radius 1]
      --pick BAG:u,v:VIEW:U,V | --pick BAG:u,v:point:x,y,z ...   or   --picks FILE.json
          [--rotate_camera 0] [--snap_radius 2] [--ransac_iterations 8192] [--ransac_error_thresh 10.0]
          [--robust_kernel_width 10.0] [--seed 0]

The reference's seventh executable (src/initial_guess_manual.cpp) is a window in which the user (1) turns a gizmo until the cloud
overlays the image roughly, (2) right-clicks pixel / 3D-point pairs -- the 3D side through the depth buffer of the rendered cloud --
and (3) presses "Estimate" (``PoseEstimation::estimate`` on the pairs, :55-64) and "Save" (:196-217).  Here the same three parts are
actions that write files:

* ``--candidates``  the gizmo's coarse part.  The 24 axis-aligned mountings of a camera on a LiDAR (``candidate_rotation``), translation 0;
  candidate 0 is the pose the reference's window opens with (:128-133).  Per candidate and bag ``candidate_<kk>_<bag>.png`` -- the
  overlay the viewer draws (``viewer.overlay_and_nid``) -- and, in ``candidates.json`` and a table sorted by it, the NID.  The smallest
  NID is NOT claimed to be the right mounting: the pictures are for the eye, the number sits next to them.
* ``--choose K`` / ``--transform ...``  the gizmo's "Save": candidate K, or a pose the user already has, becomes
  ``results.init_T_lidar_camera``.
* ``--sheets``  pictures to pick in.  ``<bag>_camera.png``: the camera image turned clockwise by ``--rotate_camera``.  Per ``--view``
  (``v0, v1, ...`` in command-line order) ``<bag>_v<i>.png``, the whole cloud in grey = rint(255 intensity) through the CAMERA's model
  and image size under that view's pose (``panorama``: the 1920 x 960 equirectangular camera of ``preprocess.lidar_camera``), and
  ``<bag>_v<i>_indices.png``, the row of ``<bag>.ply`` drawn at each pixel in the ``_lidar_indices.png`` layout -- both from one
  ``render.SplatRenderer.draw``.  ``sheets.json`` says what was drawn.
* ``--pick`` / ``--picks``  the estimate.  ``u,v`` is a pixel of the camera sheet as displayed (floats allowed), ``VIEW`` is ``v<i>``
  of ``sheets.json`` or ``lidar`` (the ``<bag>_lidar_indices.png`` ``preprocess`` wrote), ``U,V`` an integer pixel of it; ``point``
  gives a LiDAR-frame point directly.  The JSON file is a list of ``{"bag", "u", "v", "view", "U", "V"}`` /
  ``{"bag", "u", "v", "view": "point", "x", "y", "z"}``.  A blank LiDAR pixel snaps to the nearest covered one within
  ``--snap_radius`` (the reference's ``depth > -1 && depth < 1`` test, :141, decides the same thing: was anything drawn here).  The
  pairs of all bags, in the order given, go to ``pose.PoseEstimation.estimate`` (rotation RANSAC on the GPU, least squares on the host),
  the inverse pose to ``results.init_T_lidar_camera`` (:197-209), per-pick indices, points, inlier flags and residuals to ``report.json``.

Deliberate differences from the reference.  There is no window, no drag gizmo.  A pick is a point of the cloud, not a depth
unprojected between points.  The camera pixel is turned back with ``matching.unrotate_points``, exactly; the reference's
``transform_camera_point`` (:241-258) subtracts from the height and width instead of height - 1 and width - 1 -- one pixel off, not
reproduced (as in ``find_matches``).  The estimation options and their defaults are ``initial_guess_auto``'s, so the same pairs
give the same pose through either command; the reference's window uses the header's ``PoseEstimationParams`` (5 px threshold).
"""
import argparse
import json
import math
import os
import sys
from dataclasses import dataclass

import numpy as np

from . import dataset, matching, nid, pose, preprocess, render, se3, viewer

FACINGS = ("+x", "+y", "-x", "-y", "+z", "-z")  # where the optical axis points in the LiDAR frame, in the order of k // 4
# F_f: Rz(0), Rz(90), Rz(180), Rz(270), Ry(-90), Ry(+90) as closed forms
_FACING_ROTATIONS = (
    ((1, 0, 0), (0, 1, 0), (0, 0, 1)),
    ((0, -1, 0), (1, 0, 0), (0, 0, 1)),
    ((-1, 0, 0), (0, -1, 0), (0, 0, 1)),
    ((0, 1, 0), (-1, 0, 0), (0, 0, 1)),
    ((0, 0, -1), (0, 1, 0), (1, 0, 0)),
    ((0, 0, 1), (0, 1, 0), (-1, 0, 0)),
)
NUM_CANDIDATES = 4 * len(FACINGS)
TOO_FEW = "At least 3 correspondences are necessary!!"  # initial_guess_manual.cpp:57
PANORAMA_FOV = math.pi  # any field of view of 150 degrees or more selects preprocess.lidar_camera's equirectangular camera


class PickError(ValueError):
    """A pick that cannot be used; the message names it."""


# ------------------------------------------------------------------------------------------------ candidates
def default_rotation(camera_model):
    """initial_guess_manual.cpp:128-133: the rotation of ``T_lidar_camera`` the reference's window opens with -- AngleAxis(pi/2, Y)
    AngleAxis(-pi/2, Z), for an equirectangular camera AngleAxis(-pi/2, X) -- as ``preprocess.lidar_camera`` has them: closed forms."""
    return preprocess.lidar_camera(PANORAMA_FOV if camera_model == "equirectangular" else 0.5 * math.pi)[3][:3, :3].copy()


def candidate_rotation(k, camera_model):
    """``T_lidar_camera_k.linear() = F_f R0 Rz(90 deg r)`` for ``k = 4 f + r``: the optical axis along ``FACINGS[f]`` (for a pinhole),
    ``r`` quarter turns about it.  Every entry is 0 or +-1."""
    if not 0 <= int(k) < NUM_CANDIDATES:
        raise ValueError(f"candidate {k}: 0 .. {NUM_CANDIDATES - 1} expected")
    f, r = divmod(int(k), 4)
    return np.array(_FACING_ROTATIONS[f], dtype=np.float64) @ default_rotation(camera_model) @ np.array(_FACING_ROTATIONS[r], dtype=np.float64)


def candidate_repeats(k, camera_model):
    """The first candidate with the same rotation as ``k``, or ``None`` when there is none before it.  Under the pinhole R0 all 24 differ.
    Under the equirectangular one the camera's z lies along the LiDAR's y, Ry(-+90) turns about that axis, and 16 .. 23 repeat earlier ones."""
    R = candidate_rotation(k, camera_model)
    return next((j for j in range(int(k)) if np.array_equal(candidate_rotation(j, camera_model), R)), None)


def candidate_pose(k, camera_model):
    """4x4 ``T_lidar_camera`` of candidate ``k``: ``candidate_rotation``, translation 0."""
    T = np.eye(4)
    T[:3, :3] = candidate_rotation(k, camera_model)
    return T


def pose_to_tum(T_lidar_camera):
    """[tx ty tz qx qy qz qw] of a 4x4 ``T_lidar_camera`` (initial_guess_manual.cpp:197-201)"""
    T = np.asarray(T_lidar_camera, dtype=np.float64)
    return [float(v) for v in T[:3, 3]] + [float(v) for v in se3.rot_to_quat(T[:3, :3])]


def parse_transform(text):
    """``tx,ty,tz,qx,qy,qz,qw`` with the quaternion normalised; a zero or non-finite quaternion (or translation) is refused."""
    try:
        v = [float(s) for s in text.split(",")]
    except ValueError:
        raise ValueError(f"--transform {text}: seven comma-separated numbers expected") from None
    if len(v) != 7:
        raise ValueError(f"--transform {text}: seven comma-separated numbers expected, {len(v)} given")
    norm = math.sqrt(sum(c * c for c in v[3:]))
    if not all(math.isfinite(c) for c in v) or not math.isfinite(norm) or norm == 0.0:
        raise ValueError(f"--transform {text}: finite numbers and a non-zero quaternion expected")
    return v[:3] + [c / norm for c in v[3:]]


def _save_init_guess(data_path, config, values, log):
    """initial_guess_manual.cpp:202-214: every other key of calib.json is kept"""
    config.setdefault("results", {})["init_T_lidar_camera"] = [float(v) for v in values]
    dataset.write_calib(data_path, config)
    log("--- T_lidar_camera ---")
    log(str(viewer.tum_to_pose(values)))
    log(f"saved to {data_path}/calib.json")


def run_candidates(args, config, bags, proj, dst, log):
    model = config["camera"]["camera_model"]
    os.makedirs(dst, exist_ok=True)
    entries = []
    for k in range(NUM_CANDIDATES):
        T_lidar_camera = candidate_pose(k, model)
        T_camera_lidar = np.linalg.inv(T_lidar_camera)
        values = {}
        for bag in bags:
            overlay, _, _, values[bag.bag_name] = viewer.overlay_and_nid(args, proj, bag, T_camera_lidar)
            dataset.write_png(os.path.join(dst, f"candidate_{k:02d}_{bag.bag_name}.png"), overlay)
        entries.append({"k": k, "facing": FACINGS[k // 4], "roll": k % 4, "repeats": candidate_repeats(k, model), "T_lidar_camera": pose_to_tum(T_lidar_camera), "nid": values,
                        "nid_mean": float(np.mean(list(values.values()))) if values else float("nan")})
    report = {"data_path": args.data_path, "camera_model": model, "nid_bins": args.nid_bins, "culling": not args.disable_culling, "point_radius": args.point_radius,
              "alpha": args.alpha, "candidates": entries, "note": "the smallest NID is not claimed to be the right mounting: look at the pictures"}
    with open(os.path.join(dst, "candidates.json"), "w") as f:
        json.dump(report, f, indent=2, sort_keys=True)
        f.write("\n")
    log(" k  facing  roll  mean NID")
    for e in sorted(entries, key=lambda e: (math.isnan(e["nid_mean"]), e["nid_mean"], e["k"])):
        log(f"{e['k']:2d}  {e['facing']:>6s}  {90 * e['roll']:4d}  {e['nid_mean']:.6f}")
    log("the smallest NID is not claimed to be the right mounting: look at the pictures, then --choose K")
    log(f"saved to {dst}")
    return 0


# ------------------------------------------------------------------------------------------------ sheets
def resolve_view(spec, config, proj, image_size):
    """``(camera, (width, height), T_lidar_camera 4x4)`` of one ``--view``.  Every view but ``panorama`` looks through the camera's own
    model and image size, so that the LiDAR sheet shows what the camera sheet shows."""
    model = config["camera"]["camera_model"]
    if spec == "default":
        return proj, image_size, candidate_pose(0, model)
    if spec.startswith("candidate:"):
        try:
            return proj, image_size, candidate_pose(int(spec[len("candidate:"):]), model)
        except ValueError:
            raise ValueError(f"--view {spec}: candidate:K with K in 0 .. {NUM_CANDIDATES - 1} expected") from None
    if spec == "current":
        values, _ = dataset.init_T_lidar_camera(config)
        if values is None:
            raise ValueError("--view current: calib.json holds no initial guess")
        return proj, image_size, np.linalg.inv(se3.to_matrix(dataset.tum_to_T_camera_lidar(values)))
    if spec == "panorama":
        pano_model, pano_intrinsics, pano_size, T_lidar_camera = preprocess.lidar_camera(PANORAMA_FOV)
        return nid.create_camera(pano_model, pano_intrinsics, []), pano_size, T_lidar_camera
    raise ValueError(f"--view {spec}: default, candidate:K, current or panorama expected")


def intensity_colors(intensities):
    """RGBA8 of the LiDAR sheets: grey = rint(255 intensity) clipped (what ``_lidar_intensities.png`` stores), opaque"""
    grey = np.clip(np.rint(np.asarray(intensities, dtype=np.float64) * 255.0), 0, 255).astype(np.uint8)
    return np.stack([grey, grey, grey, np.full_like(grey, 255)], axis=1)


def run_sheets(args, config, bags, proj, dst, log):
    specs = args.view or ["default"]
    rotate = args.rotate_camera or 0
    for spec in specs:  # a misspelt view is refused before anything is written
        resolve_view(spec, config, proj, (0, 0))
    os.makedirs(dst, exist_ok=True)
    views = []
    for bag in bags:
        size = (bag.image.shape[1], bag.image.shape[0])
        dataset.write_png_gray(os.path.join(dst, f"{bag.bag_name}_camera.png"), matching.rotate_cw(bag.image, rotate))
        r = render.SplatRenderer(bag.points, device=args.device)  # one upload serves every view
        r.set_colors(intensity_colors(bag.intensities))
        for i, spec in enumerate(specs):
            view_proj, view_size, T_lidar_camera = resolve_view(spec, config, proj, size)
            T_view_lidar = np.linalg.inv(T_lidar_camera)
            rgb, index = r.draw(view_proj, view_size, T_view_lidar, radius=args.point_radius, background=None, alpha=255)
            dataset.write_png(os.path.join(dst, f"{bag.bag_name}_v{i}.png"), rgb)
            dataset.write_index_png(os.path.join(dst, f"{bag.bag_name}_v{i}_indices.png"), index)
            if i == len(views):
                views.append({"name": f"v{i}", "spec": spec, "camera_model": view_proj.model, "intrinsics": list(view_proj.intrinsics), "distortion_coeffs": list(view_proj.distortion),
                              "radius": args.point_radius, "bags": {}})
            views[i]["bags"][bag.bag_name] = {"size": [int(view_size[0]), int(view_size[1])], "T_view_lidar": [float(v) for v in T_view_lidar.ravel()],
                                              "cloud_length": int(bag.num_points), "pixels_covered": int((index >= 0).sum())}
            log(f"{bag.bag_name} v{i} [{spec}]: {view_size[0]}x{view_size[1]}, {views[i]['bags'][bag.bag_name]['pixels_covered']} pixels covered")
        r.close()
    with open(os.path.join(dst, "sheets.json"), "w") as f:
        json.dump({"data_path": args.data_path, "rotate_camera": rotate, "views": views}, f, indent=2, sort_keys=True)
        f.write("\n")
    log(f"saved to {dst}")
    return 0


# ------------------------------------------------------------------------------------------------ picks
@dataclass
class Pick:
    bag: str
    u: float  # camera sheet pixel, as displayed
    v: float
    view: str  # "v<i>", "lidar" or "point"
    U: int = None  # pixel of the LiDAR sheet
    V: int = None
    point: tuple = None  # (x, y, z) in the LiDAR frame

    def __str__(self):
        target = f"{self.point[0]!r},{self.point[1]!r},{self.point[2]!r}" if self.view == "point" else f"{self.U},{self.V}"
        return f"{self.bag}:{self.u!r},{self.v!r}:{self.view}:{target}"


def _is_view_name(view):
    return view == "lidar" or (view[:1] == "v" and view[1:].isdigit())


def _make_pick(text, bag, u, v, view, target):
    """``target``: (U, V) or (x, y, z); ``text`` names the pick in errors"""
    try:
        u, v = float(u), float(v)
    except (TypeError, ValueError):
        raise PickError(f"pick {text}: the camera pixel must be two numbers") from None
    if not bag or not isinstance(bag, str):
        raise PickError(f"pick {text}: no bag name")
    if not (math.isfinite(u) and math.isfinite(v)):
        raise PickError(f"pick {text}: the camera pixel is not finite")
    if view == "point":
        try:
            point = tuple(float(c) for c in target)
        except (TypeError, ValueError):
            raise PickError(f"pick {text}: the point must be three numbers") from None
        if len(point) != 3 or not all(math.isfinite(c) for c in point):
            raise PickError(f"pick {text}: the point must be three finite numbers")
        return Pick(bag, u, v, view, point=point)
    if not isinstance(view, str) or not _is_view_name(view):
        raise PickError(f"pick {text}: unknown view '{view}' (v<i>, lidar or point expected)")
    try:
        if len(target) != 2 or any(isinstance(c, float) and c != int(c) for c in target):
            raise ValueError
        U, V = (int(c) for c in target)
    except (TypeError, ValueError):
        raise PickError(f"pick {text}: the pixel of the LiDAR sheet must be two integers") from None
    return Pick(bag, u, v, view, U=U, V=V)


def parse_pick(text):
    """``BAG:u,v:VIEW:U,V`` or ``BAG:u,v:point:x,y,z``"""
    fields = text.rsplit(":", 3)  # (a bag name may hold a colon; the other fields cannot)
    if len(fields) != 4:
        raise PickError(f"pick {text}: BAG:u,v:VIEW:U,V or BAG:u,v:point:x,y,z expected")
    bag, camera, view, target = fields
    uv = camera.split(",")
    if len(uv) != 2:
        raise PickError(f"pick {text}: the camera pixel must be two numbers")
    return _make_pick(text, bag, uv[0], uv[1], view, target.split(","))


def picks_from_json(items):
    """The JSON form: a list of objects with the fields of the command-line form"""
    if not isinstance(items, list):
        raise PickError("picks file: a JSON list of picks expected")
    picks = []
    for i, item in enumerate(items):
        text = f"#{i} {json.dumps(item)}"
        if not isinstance(item, dict):
            raise PickError(f"pick {text}: an object expected")
        point = item.get("view") == "point"
        names = ("bag", "u", "v", "view") + (("x", "y", "z") if point else ("U", "V"))
        missing = [k for k in names if k not in item]
        unknown = [k for k in item if k not in names]
        if missing or unknown:
            raise PickError(f"pick {text}: fields {', '.join(names)} expected" + (f"; missing {', '.join(missing)}" if missing else "") + (f"; unknown {', '.join(unknown)}" if unknown else ""))
        picks.append(_make_pick(text, item["bag"], item["u"], item["v"], item["view"], [item[k] for k in names[4:]]))
    return picks


def unrotate_camera_pixel(u, v, angle, width, height):
    """A pixel (floats) of the camera sheet -- the ``width`` x ``height`` image turned clockwise by ``angle`` -- in the stored image.
    ``matching.unrotate_points`` is the map; it is affine with entries 0 and +-1, so its values at (0, 0), (1, 0) and (0, 1) carry it
    to non-integer pixels without rounding anything but the one subtraction."""
    o, ex, ey = matching.unrotate_points([[0, 0], [1, 0], [0, 1]], angle, width, height).astype(np.float64)
    x, y = o + float(u) * (ex - o) + float(v) * (ey - o)
    return float(x), float(y)


def snap_pixel(indices, U, V, radius):
    """The covered pixel (index >= 0) of ``indices`` (H, W) nearest to (U, V) within ``radius`` -- smallest dx^2 + dy^2 <= radius^2,
    then smallest dy, then smallest dx; pixels past the image edge do not count -- or ``None``.  A covered (U, V) is its own answer."""
    H, W = indices.shape
    r = int(radius)
    offsets = sorted((dx * dx + dy * dy, dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= r * r)
    for _, dy, dx in offsets:
        x, y = U + dx, V + dy
        if 0 <= x < W and 0 <= y < H and indices[y, x] >= 0:
            return x, y
    return None


def _read_sheets(dst):
    path = os.path.join(dst, "sheets.json")
    if not os.path.exists(path):
        return None
    with open(path) as f:
        return json.load(f)


def resolve_picks(picks, data_path, dst, bags, rotate_camera=0, snap_radius=2):
    """``(kpts_2d (n, 2) pixels of the stored camera images, points (n, 4), records)`` of ``picks`` in their order.  ``bags``: the
    ``dataset.VisualLiDARData`` the picks may name.  Raises ``PickError`` naming the pick: unknown bag or view, a pixel outside its
    sheet, nothing drawn within ``snap_radius``, a ``sheets.json`` made of another cloud, an index beyond the cloud."""
    by_name = {bag.bag_name: bag for bag in bags}
    sheets = None
    index_images = {}
    kpts, points, records = [], [], []
    for pick in picks:
        bag = by_name.get(pick.bag)
        if bag is None:
            raise PickError(f"pick {pick}: unknown bag '{pick.bag}' (bags: {', '.join(by_name)})")
        H, W = bag.image.shape
        Wr, Hr = (W, H) if rotate_camera in (0, 180) else (H, W)
        if not (0.0 <= pick.u <= Wr - 1 and 0.0 <= pick.v <= Hr - 1):
            raise PickError(f"pick {pick}: camera pixel outside the {Wr}x{Hr} camera sheet")
        x, y = unrotate_camera_pixel(pick.u, pick.v, rotate_camera, W, H)
        record = {"pick": str(pick), "bag": pick.bag, "camera_pixel": [pick.u, pick.v], "camera_pixel_stored": [x, y], "view": pick.view}
        if pick.view == "point":
            point = np.array([*pick.point, 1.0])
            record.update(index=None, snapped_pixel=None)
        else:
            key = (pick.bag, pick.view)
            if key not in index_images:
                if pick.view == "lidar":
                    path = os.path.join(data_path, f"{pick.bag}_lidar_indices.png")
                else:
                    sheets = sheets if sheets is not None else (_read_sheets(dst) or {})
                    entry = next((v for v in sheets.get("views", []) if v["name"] == pick.view), None)
                    if entry is None or pick.bag not in entry["bags"]:
                        raise PickError(f"pick {pick}: unknown view '{pick.view}' ({os.path.join(dst, 'sheets.json')} holds no such view of this bag)")
                    if entry["bags"][pick.bag]["cloud_length"] != bag.num_points:
                        raise PickError(f"pick {pick}: sheets.json was made of a cloud of {entry['bags'][pick.bag]['cloud_length']} points, {pick.bag}.ply holds {bag.num_points}")
                    path = os.path.join(dst, f"{pick.bag}_{pick.view}_indices.png")
                if not os.path.exists(path):
                    raise PickError(f"pick {pick}: unknown view '{pick.view}' (no {path})")
                index_images[key] = pose.read_index_image(path)
            indices = index_images[key]
            if not (0 <= pick.U < indices.shape[1] and 0 <= pick.V < indices.shape[0]):
                raise PickError(f"pick {pick}: pixel outside the {indices.shape[1]}x{indices.shape[0]} sheet '{pick.view}'")
            snapped = snap_pixel(indices, pick.U, pick.V, snap_radius)
            if snapped is None:
                raise PickError(f"pick {pick}: nothing is drawn within {snap_radius} px of ({pick.U}, {pick.V}) in sheet '{pick.view}'")
            index = int(indices[snapped[1], snapped[0]])
            if index >= bag.num_points:
                raise PickError(f"pick {pick}: point index {index} beyond the cloud ({bag.num_points} points)")
            point = np.asarray(bag.points[index], dtype=np.float64)
            record.update(index=index, snapped_pixel=[int(snapped[0]), int(snapped[1])])
        record["point"] = [float(c) for c in point[:3]]
        kpts.append((x, y))
        points.append(point)
        records.append(record)
    return np.array(kpts, dtype=np.float64).reshape(-1, 2), np.array(points, dtype=np.float64).reshape(-1, 4), records


def run_picks(args, config, bags, proj, dst, log):
    if args.picks is not None:
        with open(args.picks) as f:
            picks = picks_from_json(json.load(f))
    else:
        picks = [parse_pick(text) for text in args.pick]
    rotate = args.rotate_camera
    if rotate is None:  # the sheets the picks were presumably made in
        rotate = int((_read_sheets(dst) or {}).get("rotate_camera", 0))
    kpts, points, records = resolve_picks(picks, args.data_path, dst, bags, rotate, args.snap_radius)
    if len(records) < 3:
        print(TOO_FEW, file=sys.stderr)
        return 1

    params = pose.PoseEstimationParams(ransac_iterations=args.ransac_iterations, ransac_error_thresh=args.ransac_error_thresh, robust_kernel_width=args.robust_kernel_width)
    T_camera_lidar, inliers = pose.PoseEstimation(params).estimate(proj, kpts, points, device=args.device, seed=args.seed, log=log)
    uv = proj.project(points[:, :3] @ T_camera_lidar[:3, :3].T + T_camera_lidar[:3, 3], device=-1)
    residuals = np.linalg.norm(uv - kpts, axis=1)
    for record, inlier, residual in zip(records, inliers, residuals):
        record.update(ransac_inlier=bool(inlier), residual_px=float(residual))

    values = dataset.T_camera_lidar_to_tum(se3.from_matrix(T_camera_lidar))
    os.makedirs(dst, exist_ok=True)
    report = {"data_path": args.data_path, "rotate_camera": rotate, "snap_radius": args.snap_radius, "seed": args.seed, "ransac_iterations": args.ransac_iterations,
              "ransac_error_thresh": args.ransac_error_thresh, "robust_kernel_width": args.robust_kernel_width, "num_inliers": int(np.sum(inliers)),
              "T_camera_lidar": [float(v) for v in T_camera_lidar.ravel()], "init_T_lidar_camera": values, "picks": records}
    with open(os.path.join(dst, "report.json"), "w") as f:
        json.dump(report, f, indent=2, sort_keys=True)
        f.write("\n")
    _save_init_guess(args.data_path, config, values, log)
    log(f"{int(np.sum(inliers))} of {len(records)} picks are RANSAC inliers, worst residual {float(residuals.max()):.2f} px ({os.path.join(dst, 'report.json')})")
    log(f"for the picture: python -m direct_visual_lidar_calibration_amd.viewer {args.data_path} --transformation init_manual")
    return 0


# ------------------------------------------------------------------------------------------------ command
def build_parser():
    p = argparse.ArgumentParser(prog="initial_guess_manual", description="initial_guess_manual (headless)")
    p.add_argument("data_path", help="directory that contains preprocessed data")
    action = p.add_mutually_exclusive_group(required=True)
    action.add_argument("--candidates", action="store_true", help="draw the 24 axis-aligned mountings over the camera image, with the NID of each; the smallest NID is not claimed to be "
                        "the right mounting: the pictures are for the eye, the number sits next to them")
    action.add_argument("--choose", type=int, metavar="K", help="save candidate K as results.init_T_lidar_camera")
    action.add_argument("--transform", metavar="tx,ty,tz,qx,qy,qz,qw", help="save this T_lidar_camera as results.init_T_lidar_camera (the quaternion is normalised)")
    action.add_argument("--sheets", action="store_true", help="write the pictures to pick in: the camera image and the cloud seen through each --view, with its index image")
    action.add_argument("--pick", action="append", metavar="BAG:u,v:VIEW:U,V", help="a 2D-3D pair (repeatable): camera sheet pixel, then v<i> | lidar and a pixel of that sheet, or point and x,y,z")
    action.add_argument("--picks", metavar="FILE.json", help="the pairs as a JSON list of objects with the same fields")
    p.add_argument("--dst_path", default=None, help="where files other than calib.json go (default: <data_path>/manual)")
    p.add_argument("--first_n_bags", type=int, default=None, help="use only the first N bags")
    p.add_argument("--device", type=int, default=0, help="GPU to run on")
    p.add_argument("--view", action="append", metavar="SPEC", help="--sheets: default | candidate:K | current | panorama (repeatable; v0, v1, ... in this order; default: default)")
    p.add_argument("--rotate_camera", type=int, default=None, choices=[0, 90, 180, 270], help="the camera sheet is the camera image turned clockwise by this angle (--sheets: default 0; "
                   "picks: default what sheets.json records, else 0)")
    p.add_argument("--point_radius", type=int, default=1, help="a point covers (2 r + 1)^2 pixels")
    p.add_argument("--alpha", type=int, default=178, help="--candidates: opacity (0..255) of the points over the camera image")
    p.add_argument("--nid_bins", type=int, default=16, help="--candidates: Number of histogram bins for NID")
    p.add_argument("--disable_culling", action="store_true", help="--candidates: disable depth buffer-based hidden points removal")
    p.add_argument("--snap_radius", type=int, default=2, help="picks: a blank LiDAR pixel snaps to the nearest covered one within this many pixels (0: no snapping)")
    p.add_argument("--ransac_iterations", type=int, default=8192, help="iterations for RANSAC")
    p.add_argument("--ransac_error_thresh", type=float, default=10.0, help="reprojection error threshold [pix]")
    p.add_argument("--robust_kernel_width", type=float, default=10.0, help="Cauchy kernel width for fine estimation [pix]")
    p.add_argument("--seed", type=int, default=0, help="seed of the RANSAC hypotheses (extension)")
    return p


def parse_args(argv=None):
    """``build_parser().parse_args`` that also takes ``--transform -0.1,0,...`` as written: argparse alone reads a value that starts
    with a minus sign as an option."""
    argv = list(sys.argv[1:] if argv is None else argv)
    for i in range(len(argv) - 1):
        if argv[i] == "--transform":
            argv[i : i + 2] = ["--transform=" + argv[i + 1]]
            break
    return build_parser().parse_args(argv)


def run(args, log=print):
    config = dataset.read_calib(args.data_path)  # "error: failed to open <data_path>/calib.json" (initial_guess_manual.cpp:77-81)
    model, intrinsics, distortion = dataset.camera_from_calib(config)
    dst = args.dst_path or os.path.join(args.data_path, "manual")
    try:
        if args.choose is not None:
            _save_init_guess(args.data_path, config, pose_to_tum(candidate_pose(args.choose, model)), log)
            return 0
        if args.transform is not None:
            _save_init_guess(args.data_path, config, parse_transform(args.transform), log)
            return 0
        if not 0 <= args.alpha <= 255 or not 0 <= args.point_radius <= 8 or args.snap_radius < 0:
            raise ValueError("--alpha must lie in [0, 255], --point_radius in [0, 8] and --snap_radius must not be negative")
        proj = nid.create_camera(model, intrinsics, distortion)
        if proj is None:
            raise ValueError(f"unknown camera model / wrong number of intrinsics: {model}")
        _, bags = dataset.load_dataset(args.data_path, args.first_n_bags)
        if args.pick is not None or args.picks is not None:
            return run_picks(args, config, bags, proj, dst, log)
        if args.candidates:
            return run_candidates(args, config, bags, proj, dst, log)
        return run_sheets(args, config, bags, proj, dst, log)
    except ValueError as e:  # (PickError included) nothing has been written to calib.json
        raise SystemExit(f"error: {e}") from None


def main(argv=None):
    return run(parse_args(argv))


if __name__ == "__main__":
    sys.exit(main())
