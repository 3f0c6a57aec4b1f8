"""``preprocess_map`` on the MI355X engine: a point-cloud map and one photograph in, a preprocessed directory out -- ``calib.json``,
``000000.png``, ``000000.ply``, ``000000_lidar_intensities.png`` and ``000000_lidar_indices.png`` --, the directory
``initial_guess_auto`` and ``calibrate`` read.  From raw inputs:

    python -m direct_visual_lidar_calibration_amd.preprocess_map --map_path map.ply --image_path image.png --dst_path data
        --camera_model plumb_bob --camera_intrinsics 1100,1100,960,540 --camera_distortion_coeffs -0.04,0.08,0,0,0
    (2D-3D matches between data/000000.png and data/000000_lidar_intensities.png -> data/000000_matches.json)
    python -m direct_visual_lidar_calibration_amd.initial_guess_auto data
    python -m direct_visual_lidar_calibration_amd.calibrate data

Mirrors the reference executable (src/preprocess_map.cpp:34-223), same option names and defaults (:41-49), same steps in the same
order: equalise the image (``cv::equalizeHist``), voxel-filter the map, rank-equalise the intensities (:158-168), write the PLY
(:173-180), estimate the LiDAR's field of view and render the LiDAR intensity / index images through the virtual camera it selects
(:183-211), write ``calib.json`` (:97-109).  Differences from the reference:

* the voxel filter is the voxel integrator (``preprocess.StaticPointCloudIntegrator``: the LAST point of every occupied voxel, in
  input order of the winners) in place of ``pcl::ApproximateVoxelGrid`` (:139-143) -- PCL's order-dependent approximate centroid
  filter, which is not in the reference tree and cannot be restated;
* ``--min_distance`` is accepted and NOT applied: the reference passes it to ``load_lidar_points`` (:93), which never uses it.  The
  integrator runs with a minimum distance of 0;
* images are PNGs (whatever ``dataset.read_png_gray`` reads) or baseline JPEGs, read as ``cv::imread(path, 0)`` reads them (:69):
  the Y plane of the stream, turned as its EXIF orientation says (``dataset.read_image_gray``; the inverse DCT runs on the GPU).
  Progressive, arithmetic-coded, 12-bit and CMYK JPEGs are refused with the reason; the values are pinned against libjpeg-turbo,
  not against OpenCV itself;
* an empty ``--camera_distortion_coeffs`` string means no coefficients (the reference's ``std::stod("")`` throws);
* ``--visualize`` is not offered; ``--device`` is an extension.
"""
import argparse
import sys

import numpy as np

from . import dataset, preprocess

BAG_NAME = "000000"
_REQUIRED = ("map_path", "image_path", "dst_path", "camera_model", "camera_intrinsics", "camera_distortion_coeffs")


def build_parser():
    p = argparse.ArgumentParser(prog="preprocess_map", description="preprocess_map")
    p.add_argument("--map_path", help="path to input point cloud map (PCD or PLY)")
    p.add_argument("--image_path", help="path to input image: PNG, or baseline JPEG read as cv::imread(path, 0) reads it (the Y plane, EXIF orientation applied)")
    p.add_argument("--dst_path", help="directory to save preprocessed data")
    p.add_argument("--camera_model", help="atan, plumb_bob, fisheye, omnidir, or equirectangular")
    p.add_argument("--camera_intrinsics", help="camera intrinsic parameters [fx,fy,cx,cy(,xi)] (don't put spaces between values!!)")
    p.add_argument("--camera_distortion_coeffs", help="camera distortion parameters [k1,k2,p1,p2,k3] (don't put spaces between values!!); an empty string = none")
    p.add_argument("--voxel_resolution", type=float, default=0.002, help="voxel grid resolution")
    p.add_argument("--min_distance", type=float, default=1.0, help="minimum point distance. Accepted and NOT applied, as in the reference (its load_lidar_points never uses it)")
    p.add_argument("--device", type=int, default=0, help="GPU the voxel filter, the equalisation and the rendering run on (extension)")
    return p


def parse_values(text):
    """``boost::split(tokens, text, is_any_of(","))`` + ``std::stod`` per token (:84-91); an empty string gives no values."""
    return [float(tok) for tok in text.split(",")] if text.strip() else []


def read_map(path):
    """The map's points and intensities as stored: float32 ``(xyz (n, 3), intensities (n,))`` for PCD files and float32 PLY
    files, else float64 ``(points (n, 4), intensities (n,))`` (``dataset.read_ply``)."""
    if path.lower().endswith(".pcd"):
        return dataset.read_pcd(path)
    f32 = dataset.read_ply_float32(path)
    if f32 is not None:
        return f32
    points, intensities = dataset.read_ply(path)
    return points, (np.zeros(points.shape[0]) if intensities is None else intensities)


def load_lidar_points(path, voxel_resolution, device=0, log=print):
    """``load_lidar_points`` (:127-171): ``(points (m, 4) float64, intensities (m,) float64 rank-equalised)`` of the filtered map;
    the points are float32 values (``getVector4fMap().cast<double>()``, :150)."""
    xyz, inten = read_map(path)
    if xyz.shape[0] == 0:
        raise ValueError(f"error: no map points in {path}")
    integ = preprocess.StaticPointCloudIntegrator(voxel_resolution=voxel_resolution, min_distance=0.0, device=device)
    try:
        integ.insert_points(xyz, inten)
        rec = integ.get_records()
    finally:
        integ.close()
    log(f"map_points={xyz.shape[0]} filtered={rec.shape[0]}")
    return preprocess.equalized_cloud(rec, device=device)  # :158-168


def run(args, log=print):
    image = preprocess.equalize_hist(dataset.read_image_gray(args.image_path, device=args.device))  # :69-75 (written with the rest of the directory below)
    intrinsics = parse_values(args.camera_intrinsics)
    distortion = parse_values(args.camera_distortion_coeffs)

    points, intensities = load_lidar_points(args.map_path, args.voxel_resolution, device=args.device, log=log)

    # save_lidar_data (:173-215)
    meta = {"data_path": args.map_path, "camera_info_topic": "N/A", "image_topic": "N/A", "points_topic": "N/A", "intensity_channel": "N/A"}  # :97-106
    config, lidar_fov = preprocess.save_preprocessed(args.dst_path, (args.camera_model, intrinsics, distortion), [(BAG_NAME, image, points, intensities)], meta, device=args.device, log=log)
    return config, points, intensities, lidar_fov


def _attach_values(argv):
    """``--camera_distortion_coeffs -0.04,0.08`` as boost::program_options takes it: argparse would read a value that starts with
    a minus sign and is not a plain number as another option, so the two list options get their value attached with ``=``."""
    out, it = [], iter(argv)
    for a in it:
        if a in ("--camera_intrinsics", "--camera_distortion_coeffs"):
            v = next(it, None)
            out.append(a if v is None else f"{a}={v}")
        else:
            out.append(a)
    return out


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(_attach_values(sys.argv[1:] if argv is None else list(argv)))
    if any(getattr(args, k) is None for k in _REQUIRED):  # :56-61: the usage, and 0
        parser.print_help()
        return 0
    try:
        run(args)
    except (OSError, ValueError) as e:  # (the reference prints "error: failed to load ..." and returns 1, :70-73 / :130-138)
        msg = str(e)
        print(msg if msg.startswith("error:") else f"error: {msg}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
