"""``initial_guess_auto`` on the MI355X engine: reads a preprocessed directory and its ``<bag>_matches.json`` files (2D-3D
keypoint matches between the camera image and the rendered LiDAR intensity image), estimates ``T_lidar_camera`` -- rotation
RANSAC on the GPU, reprojection least squares on the host -- and writes ``results.init_T_lidar_camera_auto`` into
``calib.json``, the key ``calibrate`` starts from.

Mirrors the reference executable (src/initial_guess_auto.cpp:26-185):

    python -m direct_visual_lidar_calibration_amd.initial_guess_auto <data_path> [--ransac_iterations 8192]
        [--ransac_error_thresh 10.0] [--robust_kernel_width 10.0] [--seed 0] [--picture]

Same option names, defaults (:161-165) and ``calib.json`` key; ``--seed`` is an extension (the reference's sampling depends on
its thread count).  ``--picture`` (extension) stands in for the window the reference opens on its result: one
``<bag>_init_auto.png`` per bag, the camera image with every correspondence's keypoint, its 3-D point's projection under the estimated
pose and the line between them, green where the reprojection error is below ``--ransac_error_thresh`` and red elsewhere
(draw.residual_primitives); ``calib.json`` does not depend on it.  The matches come from ``find_matches`` (find_matches.py: a FAST / BRIEF stand-in for the reference's SuperGlue script,
find_matches_superglue.py, whose file this reads just as well).
"""
import argparse
import os
import sys

import numpy as np

from . import dataset, draw, nid, pose, se3


def build_parser():
    p = argparse.ArgumentParser(prog="initial_guess_auto", description="initial_guess_auto")
    p.add_argument("data_path", help="directory that contains preprocessed data")
    p.add_argument("--ransac_iterations", type=int, default=8192, help="iterations for RANSAC")
    p.add_argument("--ransac_error_thresh", type=float, default=10.0, help="reprojection error threshold [pix]")
    p.add_argument("--robust_kernel_width", type=float, default=10.0, help="Cauchy kernel width for fine estimation [pix]")
    p.add_argument("--seed", type=int, default=0, help="seed of the RANSAC hypotheses (extension)")
    p.add_argument("--device", type=int, default=0, help="GPU the RANSAC runs on (extension)")
    p.add_argument("--picture", action="store_true", help="write <bag>_init_auto.png: the correspondences' residuals under the estimated pose (extension)")
    return p


def write_pictures(data_path, proj, bags, T_camera_lidar, error_thresh, device=0, log=print):
    """One ``<bag>_init_auto.png`` per ``(bag_name, image, kpts_2d, points)``: draw.residual_primitives over the camera image"""
    written = []
    for bag_name, image, kp, pts in bags:
        prims, green, red = draw.residual_primitives(proj, kp, pts, T_camera_lidar, error_thresh)
        path = os.path.join(data_path, bag_name + "_init_auto.png")
        dataset.write_png(path, draw.draw(image, None, prims, device=device))
        log(f"{bag_name}: {green} correspondences within {error_thresh} px (green), {red} beyond (red) -> {path}")
        written.append(path)
    return written


def run(args, log=print):
    config = dataset.read_calib(args.data_path)  # "error: failed to open <data_path>/calib.json" (initial_guess_auto.cpp:29-33)
    model, intrinsics, distortion = dataset.camera_from_calib(config)
    proj = nid.create_camera(model, intrinsics, distortion)
    if proj is None:
        raise SystemExit(f"error: unknown camera model / wrong number of intrinsics: {model}")
    kpts, points, bags = [], [], []
    for bag_name in config["meta"]["bag_names"]:  # :53-58
        bag = dataset.VisualLiDARData(args.data_path, bag_name)
        kp, pts = pose.read_correspondences(args.data_path, bag_name, bag.points, log=log)
        kpts.append(kp)
        points.append(pts)
        bags.append((bag_name, bag.image, kp, pts))
    kpts = np.concatenate(kpts) if kpts else np.zeros((0, 2))
    points = np.concatenate(points) if points else np.zeros((0, 4))
    if kpts.shape[0] < 2:
        raise SystemExit(f"error: {kpts.shape[0]} usable correspondences; the rotation needs at least two")

    params = pose.PoseEstimationParams(ransac_iterations=args.ransac_iterations, ransac_error_thresh=args.ransac_error_thresh, robust_kernel_width=args.robust_kernel_width)
    T_camera_lidar, inliers = pose.PoseEstimation(params).estimate(proj, kpts, points, device=args.device, seed=args.seed, log=log)

    # :124-129: the INVERSE pose, TUM order, quaternion normalised
    values = dataset.T_camera_lidar_to_tum(se3.from_matrix(T_camera_lidar))
    config.setdefault("results", {})["init_T_lidar_camera_auto"] = values
    dataset.write_calib(args.data_path, config)
    log(f"saved to {args.data_path}/calib.json")
    if args.picture:
        write_pictures(args.data_path, proj, bags, T_camera_lidar, args.ransac_error_thresh, device=args.device, log=log)
    return config, T_camera_lidar, inliers


def main(argv=None):
    args = build_parser().parse_args(argv)
    run(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
