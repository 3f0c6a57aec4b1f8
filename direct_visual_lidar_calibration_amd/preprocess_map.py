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
* ``--visualize`` is not offered; ``--device`` is an extension;
* survey maps (extensions; the reference reads PCD and PLY through PCL): ``--map_path map.las`` reads ASPRS LAS 1.0 - 1.4, point formats
  0 - 10, streamed in chunks and decoded on the GPU as ``(int32 * scale + offset) - origin`` in fp64 straight into the voxel filter, and
  a PCD map may be ``DATA binary_compressed``.  ``--map_origin auto|x,y,z`` is where the virtual camera of the LiDAR intensity image
  stands, in map coordinates -- about where the photograph was taken; for a georeferenced map the file's origin is a datum kilometres
  away.  It is recorded as ``meta.map_origin`` and ``T_lidar_camera`` is expressed in the map frame shifted by it.
  ``--map_intensity``, ``--las_exclude_classes`` and ``--las_keep_withheld`` are LAS options.  Unpinned against laspy / PDAL / PCL /
  liblzf and real files.
"""
import argparse
import math
import sys

import numpy as np

from . import dataset, preprocess

BAG_NAME = "000000"
_REQUIRED = ("map_path", "image_path", "dst_path", "camera_model", "camera_intrinsics", "camera_distortion_coeffs")


def build_parser():
    p = argparse.ArgumentParser(prog="preprocess_map", description="preprocess_map")
    p.add_argument("--map_path", help="path to input point cloud map (PCD, PLY or LAS)")
    p.add_argument("--image_path", help="path to input image: PNG, or baseline JPEG read as cv::imread(path, 0) reads it (the Y plane, EXIF orientation applied)")
    p.add_argument("--dst_path", help="directory to save preprocessed data")
    p.add_argument("--camera_model", help="atan, plumb_bob, fisheye, omnidir, or equirectangular")
    p.add_argument("--camera_intrinsics", help="camera intrinsic parameters [fx,fy,cx,cy(,xi)] (don't put spaces between values!!)")
    p.add_argument("--camera_distortion_coeffs", help="camera distortion parameters [k1,k2,p1,p2,k3] (don't put spaces between values!!); an empty string = none")
    p.add_argument("--voxel_resolution", type=float, default=0.002, help="voxel grid resolution")
    p.add_argument("--min_distance", type=float, default=1.0, help="minimum point distance. Accepted and NOT applied, as in the reference (its load_lidar_points never uses it)")
    p.add_argument("--map_origin", default="auto", help="where the virtual LiDAR camera stands, in map coordinates -- about where the photograph was taken: auto, or x,y,z. auto is 0,0,0, "
                   "except for a LAS map whose header bounds leave +-1024 m: floor of the middle of the bounds (extension)")
    p.add_argument("--map_intensity", choices=("intensity", "rgb"), default=None, help="LAS maps: the 16-bit intensity (default) or the luma 77R+150G+29B of the colour channels (extension)")
    p.add_argument("--las_exclude_classes", default=None, help="LAS maps: classes to drop, e.g. 7,18 (default: none) (extension)")
    p.add_argument("--las_keep_withheld", action="store_true", help="LAS maps: keep points flagged withheld (default: dropped, as the flag means) (extension)")
    p.add_argument("--device", type=int, default=0, help="GPU the voxel filter, the equalisation and the rendering run on (extension)")
    return p


def parse_values(text):
    """``boost::split(tokens, text, is_any_of(","))`` + ``std::stod`` per token (:84-91); an empty string gives no values."""
    return [float(tok) for tok in text.split(",")] if text.strip() else []


def read_map(path):
    """The map's points and intensities as stored: float32 ``(xyz (n, 3), intensities (n,))`` for PCD files and float32 PLY
    files, else float64 ``(points (n, 4), intensities (n,))`` (``dataset.read_ply``).  (A ``.las`` map is not read whole: its
    header is returned, ``dataset.read_las_header``, and ``load_lidar_points`` streams the records.)"""
    if is_las(path):
        return dataset.read_las_header(path)
    if path.lower().endswith(".pcd"):
        return dataset.read_pcd(path)
    f32 = dataset.read_ply_float32(path)
    if f32 is not None:
        return f32
    points, intensities = dataset.read_ply(path)
    return points, (np.zeros(points.shape[0]) if intensities is None else intensities)


def is_las(path):
    return path.lower().endswith(".las")


LAS_AUTO_ORIGIN_LIMIT = 1024.0  # [m]: float32 spacing is 2^-13 m = 0.12 mm from here on, and the default key limit is 2097 m


def parse_map_origin(text):
    """``--map_origin``: ``None`` for ``auto``, else the three finite numbers of ``x,y,z``"""
    if text is None or text.strip().lower() == "auto":
        return None
    try:
        values = [float(tok) for tok in text.split(",")]
    except ValueError:
        values = []
    if len(values) != 3 or not all(math.isfinite(v) for v in values):
        raise ValueError(f"--map_origin must be 'auto' or three finite numbers x,y,z, got '{text}'")
    return tuple(values)


def parse_classes(text):
    """``--las_exclude_classes 7,18``: the class numbers, each in 0..255"""
    if text is None or not text.strip():
        return ()
    try:
        values = [int(tok) for tok in text.split(",")]
    except ValueError:
        values = [-1]
    if any(not 0 <= v <= 255 for v in values):
        raise ValueError(f"--las_exclude_classes must be class numbers in 0..255 separated by commas, got '{text}'")
    return tuple(values)


def las_auto_origin(header):
    """``--map_origin auto`` for a LAS map: ``0,0,0`` when all six header bounds lie within +-1024 m -- the map starts at the
    scanner, as the reference's do --, else ``floor((min + max) / 2)`` per axis: a whole number of metres, so the shift is
    easy to carry and exact in fp64."""
    bounds = tuple(header["min"]) + tuple(header["max"])
    if not all(math.isfinite(v) for v in bounds):
        raise ValueError(f"LAS header bounds {bounds} are not finite: give --map_origin x,y,z")
    if all(abs(v) <= LAS_AUTO_ORIGIN_LIMIT for v in bounds):
        return (0.0, 0.0, 0.0)
    return tuple(float(math.floor((lo + hi) / 2.0)) for lo, hi in zip(header["min"], header["max"]))


def resolve_map_origin(path, map_origin=None):
    """The origin ``load_lidar_points`` will use: ``map_origin`` if given, else ``auto`` -- ``las_auto_origin`` for a LAS map,
    ``0,0,0`` for PLY and PCD (the unchanged route)."""
    if map_origin is not None:
        return tuple(float(v) for v in map_origin)
    return las_auto_origin(dataset.read_las_header(path)) if is_las(path) else (0.0, 0.0, 0.0)


def integrate_las(integ, path, header, origin, map_intensity="intensity", exclude_classes=(), keep_withheld=False, chunk_points=1 << 23):
    """Streams the records of a LAS file into the integrator, ``chunk_points`` records at a time (host memory: one chunk); returns
    the number of points the class and withheld filters dropped."""
    skipped = 0
    for raw in dataset.read_las_chunks(path, header, chunk_points):
        skipped += integ.insert_las(raw, header["record_length"], header["point_format"], header["scale"], header["offset"], origin, map_intensity, exclude_classes, keep_withheld)
    return skipped


def load_lidar_points(path, voxel_resolution, device=0, log=print, map_origin=None, map_intensity=None, las_exclude_classes=None, las_keep_withheld=False, chunk_points=1 << 23):
    """``load_lidar_points`` (:127-171): ``(points (m, 4) float64, intensities (m,) float64 rank-equalised)`` of the filtered map;
    the points are float32 values (``getVector4fMap().cast<double>()``, :150), in the frame whose origin is
    ``resolve_map_origin(path, map_origin)``.  ``map_intensity`` (``intensity`` | ``rgb``), ``las_exclude_classes`` and
    ``las_keep_withheld`` are LAS options: given (not ``None`` / falsy) with another map format they are refused by name."""
    las = is_las(path)
    if not las:
        for name, given in (("--map_intensity", map_intensity is not None), ("--las_exclude_classes", bool(las_exclude_classes)), ("--las_keep_withheld", bool(las_keep_withheld))):
            if given:
                raise ValueError(f"{name} is an option for LAS maps; {path} is not a .las file")
    origin = resolve_map_origin(path, map_origin)
    origin_line = f"map_origin={origin[0]:.17g},{origin[1]:.17g},{origin[2]:.17g}"
    if las:
        header = read_map(path)
        source = map_intensity or "intensity"
        if source not in ("intensity", "rgb"):
            raise ValueError(f"--map_intensity must be intensity or rgb, got '{source}'")
        if source == "rgb" and header["point_format"] not in dataset.LAS_RGB_OFFSET:
            raise ValueError(f"--map_intensity rgb: {path} has point format {header['point_format']}, which carries no colour")
        if header["num_points"] == 0:
            raise ValueError(f"error: no map points in {path}")
    else:
        xyz, inten = read_map(path)
        if xyz.shape[0] == 0:
            raise ValueError(f"error: no map points in {path}")
    integ = preprocess.StaticPointCloudIntegrator(voxel_resolution=voxel_resolution, min_distance=0.0, device=device)
    try:
        if las:
            log(origin_line)
            skipped = integrate_las(integ, path, header, origin, source, tuple(las_exclude_classes or ()), bool(las_keep_withheld), chunk_points)
            rec = integ.get_records()
            log(f"map_points={header['num_points']} skipped={skipped} filtered={rec.shape[0]}")
            if rec.shape[0] == 0:
                raise ValueError(f"error: no map points in {path} after the class and withheld filters")
            if source == "intensity" and bool((rec[:, 3] == rec[0, 3]).all()):
                log(f"every kept intensity is {float(rec[0, 3]):g}: the LiDAR image will show no texture; if the file carries colour, try --map_intensity rgb")
        else:
            if any(v != 0.0 for v in origin):
                log(origin_line)
                xyz = np.asarray(xyz[:, :3], dtype=np.float64) - np.asarray(origin, dtype=np.float64)  # widened on the host, then the float64 route
                inten = np.asarray(inten, dtype=np.float64)
            integ.insert_points(xyz, inten)
            rec = integ.get_records()
            log(f"map_points={xyz.shape[0]} filtered={rec.shape[0]}")
    finally:
        integ.close()
    return preprocess.equalized_cloud(rec, device=device)  # :158-168


def run(args, log=print):
    image = preprocess.equalize_hist(dataset.read_image_gray(args.image_path, device=args.device))  # :69-75 (written with the rest of the directory below)
    intrinsics = parse_values(args.camera_intrinsics)
    distortion = parse_values(args.camera_distortion_coeffs)

    origin = resolve_map_origin(args.map_path, parse_map_origin(getattr(args, "map_origin", None)))
    points, intensities = load_lidar_points(args.map_path, args.voxel_resolution, device=args.device, log=log, map_origin=origin, map_intensity=getattr(args, "map_intensity", None),
                                            las_exclude_classes=parse_classes(getattr(args, "las_exclude_classes", None)), las_keep_withheld=getattr(args, "las_keep_withheld", False))

    # save_lidar_data (:173-215)
    meta = {"data_path": args.map_path, "camera_info_topic": "N/A", "image_topic": "N/A", "points_topic": "N/A", "intensity_channel": "N/A"}  # :97-106
    if is_las(args.map_path) or any(v != 0.0 for v in origin):
        meta["map_origin"] = [float(v) for v in origin]  # T_lidar_camera is expressed in the map frame shifted by this
    config, lidar_fov = preprocess.save_preprocessed(args.dst_path, (args.camera_model, intrinsics, distortion), [(BAG_NAME, image, points, intensities)], meta, device=args.device, log=log)
    return config, points, intensities, lidar_fov


def _attach_values(argv):
    """``--camera_distortion_coeffs -0.04,0.08`` as boost::program_options takes it: argparse would read a value that starts with
    a minus sign and is not a plain number as another option, so the two list options and ``--map_origin`` get their value attached with ``=``."""
    out, it = [], iter(argv)
    for a in it:
        if a in ("--camera_intrinsics", "--camera_distortion_coeffs", "--map_origin"):
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
