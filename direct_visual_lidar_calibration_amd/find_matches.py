"""``find_matches`` on the MI355X engine: for every bag of a preprocessed directory, keypoints of the camera image and of the LiDAR
intensity image and the matches between them, written to ``<bag>_matches.json`` -- the file ``initial_guess_auto`` reads.

    python -m direct_visual_lidar_calibration_amd.find_matches <data_path> [--max_keypoints 2048] [--nms_radius 4]
        [--fast_threshold T] [--max_distance D] [--ratio R] [--levels 8] [--rotate_camera 0] [--rotate_lidar 0] [--device 0]
        [--picture | --picture_only] [--mask PATH|auto]

This takes the place of the reference's ``scripts/find_matches_superglue.py`` and is NOT a port of it: SuperGlue needs pretrained
weights under a non-commercial licence, and OpenCV.  What runs here is a classical stand-in (matching.py: FAST-9 over a 6/5 pyramid,
upright BRIEF-256, mutual-best Hamming matching with a ratio test; integer arithmetic, deterministic).  Of the reference script it
keeps the command line's shape (``data_path``, ``--max_keypoints``, ``--nms_radius``, ``--rotate_camera``, ``--rotate_lidar``) and the
four JSON keys.  Its quality on real camera / LiDAR pairs is unmeasured.  Two deliberate differences: ``--max_keypoints`` defaults to
2048 (the reference: -1), and a rotation is undone exactly -- for 90 degrees clockwise the original pixel is (y_r, H - 1 - x_r), where
the reference script computes H - x_r, one pixel off.

``--picture`` also writes the match visualisation image, the reference script's ``<bag>_superglue.png``, as ``<bag>_matches.png``: both
images side by side, every keypoint circled, every match a line coloured by its confidence (draw.py says how it differs from the
script's: unrotated images, RGB colours, an integer resize).  ``--picture_only`` draws it from the ``<bag>_matches.json`` files already
in the directory and runs no detection or matching; it draws a file the reference's SuperGlue script wrote just as well (float
keypoints are truncated; a keypoint outside its image is refused).  ``--show_keypoints``, which opens a window, is not built.

``--mask PATH|auto`` (extension; the files ``calibrate --mask`` reads, ``dataset.load_mask``) reports camera keypoints only on the
mask's non-zero pixels: the mask is used as given, with no margin.
"""
import argparse
import json
import os
import sys

import numpy as np

from . import dataset, draw, matching, pose


def build_parser():
    p = argparse.ArgumentParser(prog="find_matches", description="find_matches: 2D-2D matches between camera and LiDAR intensity images (FAST/BRIEF stand-in for SuperGlue)")
    p.add_argument("data_path", help="directory that contains preprocessed data")
    p.add_argument("--max_keypoints", type=int, default=matching.MAX_KEYPOINTS, help="keypoints kept per image, strongest first (-1 keeps all, capped at %d)" % matching.CAPACITY)
    p.add_argument("--nms_radius", type=int, default=matching.NMS_RADIUS, help="non-maximum suppression radius [pix of the pyramid level]")
    p.add_argument("--fast_threshold", type=int, default=matching.FAST_THRESHOLD, help="FAST-9 threshold [grey levels]")
    p.add_argument("--max_distance", type=int, default=matching.MAX_DISTANCE, help="largest accepted Hamming distance of 256 bits")
    p.add_argument("--ratio", type=float, default=matching.RATIO, help="accepted when best < ratio * second best (three decimals are kept)")
    p.add_argument("--levels", type=int, default=matching.LEVELS, help="pyramid levels at ratio 6/5")
    p.add_argument("--fill_passes", type=int, default=matching.FILL_PASSES, help="hole-filling passes over the LiDAR image's blank pixels")
    p.add_argument("--rotate_camera", type=int, default=0, choices=(0, 90, 180, 270), help="rotate camera image before matching (CW)")
    p.add_argument("--rotate_lidar", type=int, default=0, choices=(0, 90, 180, 270), help="rotate LiDAR image before matching (CW)")
    p.add_argument("--device", type=int, default=0, help="GPU")
    p.add_argument("--mask", default=None, metavar="PATH|auto", help="camera keypoints only where this 8-bit PNG is non-zero: one file for all bags, or 'auto' = <bag>_mask.png, else mask.png")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--picture", action="store_true", help="also write <bag>_matches.png: both images, keypoints and matches")
    g.add_argument("--picture_only", action="store_true", help="draw <bag>_matches.png from the <bag>_matches.json already there; no detection or matching")
    return p


def write_picture(data_path, bag_name, camera, lidar, result, device=0):
    """``<bag>_matches.png`` of one bag (draw.match_picture); returns its path"""
    path = os.path.join(data_path, bag_name + "_matches.png")
    dataset.write_png(path, draw.match_picture(camera, lidar, result, device=device))
    return path


def run(args, log=print):
    """Returns the ``<bag>_matches.json`` paths written (none with ``--picture_only``); the pictures are named in the log only."""
    config = dataset.read_calib(args.data_path)
    written = []
    for bag_name in config["meta"]["bag_names"]:
        camera = dataset.read_png_gray(os.path.join(args.data_path, bag_name + ".png"))
        lidar = dataset.read_png_gray(os.path.join(args.data_path, bag_name + "_lidar_intensities.png"))
        if args.picture_only:
            path = os.path.join(args.data_path, bag_name + "_matches.json")
            if not os.path.exists(path):
                raise FileNotFoundError(f"error: failed to open {path}")
            with open(path) as f:
                result = json.load(f)
            try:
                picture = write_picture(args.data_path, bag_name, camera, lidar, result, device=args.device)
            except ValueError as e:
                raise ValueError(f"{path}: {e}") from None
            log(f"{bag_name}: {sum(1 for m in result['matches'] if m >= 0)} matches of {path} -> {picture}")
            continue
        indices = pose.read_index_image(os.path.join(args.data_path, bag_name + "_lidar_indices.png"))
        if indices.shape != lidar.shape:
            raise ValueError(f"{bag_name}: the LiDAR index image is {indices.shape[1]}x{indices.shape[0]}, the intensity image {lidar.shape[1]}x{lidar.shape[0]}")
        extra = {}
        if args.mask is not None:
            cam_mask = dataset.load_mask(args.data_path, bag_name, args.mask, camera.shape, log=log)
            if cam_mask is not None:
                extra["camera_valid_mask"] = cam_mask
        result = matching.find_matches(np.ascontiguousarray(camera, dtype=np.uint8), np.ascontiguousarray(lidar, dtype=np.uint8), indices >= 0, max_keypoints=args.max_keypoints,
                                       nms_radius=args.nms_radius, fast_threshold=args.fast_threshold, max_distance=args.max_distance, ratio=args.ratio, levels=args.levels,
                                       fill_passes=args.fill_passes, rotate_camera=args.rotate_camera, rotate_lidar=args.rotate_lidar, device=args.device, **extra)
        path = os.path.join(args.data_path, bag_name + "_matches.json")
        with open(path, "w") as f:
            json.dump(result, f)
        n = sum(1 for m in result["matches"] if m >= 0)
        picture = ", " + write_picture(args.data_path, bag_name, camera, lidar, result, device=args.device) if args.picture else ""
        log(f"{bag_name}: {len(result['kpts0']) // 2} camera keypoints, {len(result['kpts1']) // 2} LiDAR keypoints, {n} matches -> {path}{picture}")
        written.append(path)
    return written


def main(argv=None):
    args = build_parser().parse_args(argv)
    run(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
