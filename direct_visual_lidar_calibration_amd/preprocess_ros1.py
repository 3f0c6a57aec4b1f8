"""``preprocess`` on the MI355X engine, from ROS1 bags: a directory of bags in, a preprocessed directory out -- ``calib.json`` and,
per bag, ``<bag>.png``, ``<bag>.ply``, ``<bag>_lidar_intensities.png`` and ``<bag>_lidar_indices.png`` --, the directory
``initial_guess_auto`` and ``calibrate`` read.

    python -m direct_visual_lidar_calibration_amd.preprocess_ros1 bags/ data/ -a
    python -m direct_visual_lidar_calibration_amd.preprocess_ros1 bags/ data/ --image_topic /image --points_topic /points
        --camera_model plumb_bob --camera_intrinsics 1100,1100,960,540 --camera_distortion_coeffs -0.04,0.08,0,0,0

Mirrors ``vlcal::Preprocess::run`` (src/vlcal/preprocess/preprocess.cpp:37-264) with its ROS1 back end (src/preprocess_ros1.cpp),
same option names and defaults (:43-61), same steps in the same order: the bags of ``data_path`` sorted (:84-120), topics (:266-317),
intensity channel (:319-347) and camera parameters (:349-404) from the FIRST bag; per bag the first image equalised
(``cv::equalizeHist``, :414-419), every PointCloud2 frame of the points topic through ``TimeKeeper::process`` and, unless its stamp
rewinds, into the static integrator (:442-460), the intensities rank-equalised (:464-473), ``<bag>.png`` and ``<bag>.ply`` (:160-169);
then the LiDAR's field of view from the first bag, both LiDAR images of every bag (:177-212) and ``calib.json`` (:220-232).
The bag reader is ``rosbag1`` (pure Python, no ROS); a frame's records are uploaded as they lie in the message and decoded on the
GPU (``StaticPointCloudIntegrator.insert_cloud2``).  Differences from the reference:

* a points topic of ``velodyne_msgs/VelodyneScan`` (the raw packets of a VLP-16 / HDL-32E, decoded on the GPU: ``--lidar_model``,
  ``--velodyne_calibration``) or ``livox_ros_driver(2)/CustomMsg`` is read in a PointCloud2 topic's place (``lidar_messages``, unpinned
  against the vendor drivers); with ``-a`` only in a bag that has no PointCloud2 topic.  The reference needs the driver's cloud;
* a points topic of ``ouster_ros/PacketMsg`` (one UDP packet of an Ouster sensor a message; with ``-a`` a topic whose name ends in
  ``lidar_packets``) is batched into scans and decoded on the GPU likewise: ``--ouster_metadata auto|FILE.json`` gives the sensor's
  geometry, ``--ouster_frame sensor|lidar`` the frame of the points.  The records come in packet order, not the driver's H x W image;

* ``-d / --dynamic_lidar_integration`` is refused here with status 1 and a message: the dynamic LiDAR integration (CT-GICP) is a
  command of its own, ``preprocess_dynamic``, which runs this module's ``run`` with ``odometry.DynamicPointCloudIntegrator``;
* ROS2 bags (sqlite3 / mcap) are not read here: a file that does not start with ``#ROSBAG V2.0`` is not a bag (``valid_bag``).  They are
  ``preprocess_ros2``'s, which runs this module's ``run`` with ``rosbag2`` as the reader;
* images: ``sensor_msgs/Image`` in mono8 / bgr8 / rgb8 / bgra8 / rgba8 and, converted on the GPU (``rosbag1.image_to_mono8``; the rules are unpinned
  against OpenCV and cv_bridge), the Bayer mosaics, yuv422 / yuv422_yuy2, mono16 and 16-bit colour; every other encoding (8UC1, 16UC1, 32FC1, nv21 ...) and a
  mosaic below 3 x 3 are refused by name; ``sensor_msgs/CompressedImage`` with a PNG or a baseline JPEG payload.  A JPEG
  is decoded as ``cv_bridge::toCvCopy(msg, "mono8")`` decodes it -- to BGR, then OpenCV's luma; NOT the Y plane ``preprocess_map`` takes
  from a JPEG file -- with the inverse DCT and the colour conversion on the GPU; streams outside the decoder's scope are refused;
* where the reference dereferences a null message -- a cloud without x / y / z or without the intensity channel, a bag without the
  image, points or camera_info topic it needs --, where ``extract_raw_points`` gives up (big-endian data, an unsupported datatype)
  and where it aborts (an invalid ``--camera_model``): a ``ValueError`` that names the topic and the bag, status 1;
* the voxel table's packed key (``preprocess.StaticPointCloudIntegrator``): a frame with a finite point whose voxel index leaves
  [-2^20, 2^20) is refused; the output order of the points is ascending sequence number of the winners;
* an empty ``--camera_distortion_coeffs`` string means no coefficients (the reference's ``std::stod("")`` throws);
* ``--visualize`` is not offered; ``--device`` is an extension; ``--k_neighbors`` and ``--verbose`` are accepted and unused (they
  configure the dynamic integrator: ``preprocess_dynamic``).
"""
import argparse
import os
import sys

import numpy as np

from . import lidar_messages, preprocess, rosbag1
from .preprocess_map import _attach_values, parse_values

VALID_CAMERA_MODELS = ("plumb_bob", "fisheye", "equidistant", "omnidir", "equirectangular")  # preprocess.cpp:362
TIME_FIELDS = ("t", "time", "time_stamp", "timestamp")  # ros_cloud_converter.hpp:81-84


def _warn(msg):
    print(msg, file=sys.stderr)


def build_parser():
    p = argparse.ArgumentParser(prog="preprocess_ros1", description="preprocess")
    p.add_argument("data_path", nargs="?", help="directory that contains rosbags for calibration")
    p.add_argument("dst_path", nargs="?", help="directory to save preprocessed data")
    p.add_argument("--bag_id", type=int, help="specify the bag to use (just for evaluation)")
    p.add_argument("--first_n_bags", type=int, help="use only the first N bags (just for evaluation)")
    p.add_argument("-a", "--auto_topic", action="store_true", help="automatically select topics")
    p.add_argument("-d", "--dynamic_lidar_integration", action="store_true", help="create target point cloud from dynamic LiDAR data (refused here: use preprocess_dynamic)")
    p.add_argument("-i", "--intensity_channel", default="auto", help="auto or channel name")
    p.add_argument("--camera_info_topic")
    p.add_argument("--image_topic", help="sensor_msgs/Image, or CompressedImage with a PNG or baseline JPEG payload; a JPEG is decoded as cv_bridge::toCvCopy(msg, mono8) decodes "
                                         "it (to BGR, then luma), which is not the Y plane cv::imread(path, 0) returns")
    p.add_argument("--points_topic", help="sensor_msgs/PointCloud2, velodyne_msgs/VelodyneScan (the raw packets, decoded on the GPU), livox_ros_driver(2)/CustomMsg or ouster_ros/PacketMsg "
                                          "(the lidar packets, decoded on the GPU: --ouster_metadata)")
    p.add_argument("--lidar_model", default="auto", choices=("auto",) + lidar_messages.LIDAR_MODELS,
                   help="packet layout and laser angles of a VelodyneScan topic: auto reads the product id of the first packet (extension)")
    p.add_argument("--velodyne_calibration", help="the vendor driver's calibration YAML (16 or 32 lasers) in place of the built-in angles of a VelodyneScan topic (extension)")
    p.add_argument("--ouster_metadata", default="auto", help="the sensor's metadata JSON for a points topic of Ouster packets (ouster_ros/PacketMsg): auto takes the first message of a "
                                                              "std_msgs/String topic of the bag whose name ends in 'metadata', else a FILE.json (extension)")
    p.add_argument("--ouster_frame", default="sensor", choices=lidar_messages.OUSTER_FRAMES,
                   help="frame of the points decoded from Ouster packets, and so the frame T_lidar_camera is expressed in: sensor applies the metadata's lidar_to_sensor_transform, "
                        "lidar the identity (extension)")
    p.add_argument("--camera_model", default="auto", help="auto, atan, plumb_bob, fisheye(=equidistant), omnidir, or equirectangular")
    p.add_argument("--camera_intrinsics", help="camera intrinsic parameters [fx,fy,cx,cy(,xi)] (don't put spaces between values!!)")
    p.add_argument("--camera_distortion_coeffs", help="camera distortion parameters [k1,k2,p1,p2,k3] (don't put spaces between values!!)")
    p.add_argument("--k_neighbors", type=int, default=20, help="num of neighbor points used for point covariance estimation of CT-ICP (accepted, unused)")
    p.add_argument("--voxel_resolution", type=float, default=0.002, help="voxel grid resolution")
    p.add_argument("--min_distance", type=float, default=1.0, help="minimum point distance. Points closer than this value will be discarded")
    p.add_argument("--verbose", action="store_true", help="accepted, unused (the dynamic integrator's optimisation status)")
    p.add_argument("--device", type=int, default=0, help="GPU the integrator, the equalisation and the rendering run on (extension)")
    return p


def find_bags(data_path, reader=rosbag1):
    """:84-103: the entries of ``data_path`` that open as a bag of ``reader`` (``rosbag1``: files; ``rosbag2``: files and directories), sorted"""
    names = [os.path.join(data_path, n) for n in os.listdir(data_path)]
    return sorted(p for p in names if (os.path.isfile(p) or os.path.isdir(p)) and reader.valid_bag(p))


def get_topics(args, bag, log=print, warn=_warn):
    """:266-317: ``(camera_info_topic, image_topic, points_topic)``; with ``-a`` by substring of the connection's type -- the LAST
    match wins, with a warning --, then the named options for what is still empty.  A ``VelodyneScan`` or ``CustomMsg`` topic
    (``lidar_messages``) is chosen only in a bag without any ``PointCloud2`` topic."""
    camera_info_topic = image_topic = points_topic = packets_topic = ""
    if args.auto_topic:
        log(f"topics in {bag.path}:")
        for topic, type_ in bag.topics_and_types():
            log(f"- {topic} : {type_}")
            if "CameraInfo" in type_:
                if camera_info_topic:
                    warn("warning: bag constains multiple camera_info topics!!")
                camera_info_topic = topic
            elif "Image" in type_:
                if image_topic:
                    warn("warning: bag constains multiple image topics!!")
                image_topic = topic
            elif "PointCloud2" in type_:
                if points_topic:
                    warn("warning: bag constains multiple points topics!!")
                points_topic = topic
            # read in a PointCloud2 topic's place, never beside one; the Ouster IMU packets have the lidar packets' type, so the name decides
            elif "VelodyneScan" in type_ or "CustomMsg" in type_ or (lidar_messages.points_kind(type_) == "PacketMsg" and topic.endswith("lidar_packets")):
                if packets_topic:
                    warn("warning: bag constains multiple points topics!!")
                packets_topic = topic
    points_topic = points_topic or packets_topic
    camera_info_topic = camera_info_topic or args.camera_info_topic or ""
    image_topic = image_topic or args.image_topic or ""
    points_topic = points_topic or args.points_topic or ""
    for name, topic in (("camera_info", camera_info_topic), ("image", image_topic), ("points", points_topic)):
        if not topic:
            warn(f"warning: failed to get {name} topic!!")
    return camera_info_topic, image_topic, points_topic


def _first(bag, topic, type_name, decode):
    m = bag.first_message(topic, type_name)
    return None if m is None else decode(m.data)


def _first_points(bag, points_topic):
    """The topic's first PointCloud2 message; without any, its first message of another kind ``lidar_messages`` reads"""
    m = bag.first_message(points_topic, "PointCloud2")
    if m is None:
        m = next((m for m in bag.messages(points_topic) if lidar_messages.points_kind(m.type) is not None), None)
    return m


def get_intensity_channel(args, bag, points_topic, reader=rosbag1):
    """:319-347: the named channel, or with ``auto`` the field of the first cloud with the highest priority: ``reflectivity`` (2)
    beats ``intensity`` (1)"""
    channel = args.intensity_channel
    if channel != "auto":
        return channel
    priorities = {"auto": -1, "intensity": 1, "reflectivity": 2}
    m = _first_points(bag, points_topic)
    if m is None:
        raise ValueError(f"error: no sensor_msgs/PointCloud2, velodyne_msgs/VelodyneScan or livox_ros_driver(2)/CustomMsg message on points topic '{points_topic}' in {bag.path}")
    cloud = reader.decode_points(m.type, m.data, header_only=True)  # (of a VelodyneScan only the fields: nothing is decoded for them)
    for f in cloud.fields:
        if f.name in priorities and priorities[channel] < priorities[f.name]:
            channel = f.name
    if channel == "auto":
        raise ValueError(f"error: failed to determine point intensity channel automatically (points topic '{points_topic}' in {bag.path} has fields "
                         f"{', '.join(f.name for f in cloud.fields)}): you must specify the intensity channel to be used manually")
    return channel


def get_image(bag, image_topic, device=0, reader=rosbag1):
    """src/preprocess_ros1.cpp:126-139: the first ``sensor_msgs/Image`` of the topic as mono8 (``rosbag1.image_to_mono8``: Bayer, packed
    YUV 4:2:2 and 16-bit images are converted on GPU ``device``), else the first ``sensor_msgs/CompressedImage``"""
    image = _first(bag, image_topic, "Image", reader.decode_image)
    if image is not None:
        return rosbag1.image_to_mono8(image, device=device, where=f"image topic '{image_topic}' in {bag.path}")
    compressed = _first(bag, image_topic, "CompressedImage", reader.decode_compressed_image)
    if compressed is not None:
        return rosbag1.compressed_to_mono8(compressed, f"of image topic '{image_topic}' in {bag.path}", device=device)
    raise ValueError(f"error: failed to obtain an image (image_topic='{image_topic}') from {bag.path}: the bag holds no sensor_msgs/Image or CompressedImage message on it")


def get_camera_params(args, bag, camera_info_topic, image_topic, log=print, reader=rosbag1):
    """:349-404: ``(camera_model, (width, height), intrinsics, distortion_coeffs)``"""
    image = get_image(bag, image_topic, device=args.device, reader=reader)
    size = (int(image.shape[1]), int(image.shape[0]))
    model = args.camera_model
    if model != "auto":
        if model not in VALID_CAMERA_MODELS:
            raise ValueError(f"error: invalid camera model {model}: supported camera models are {' '.join(VALID_CAMERA_MODELS)}")
        if model == "equirectangular":
            return model, size, [float(size[0]), float(size[1])], []
        if args.camera_intrinsics is None:
            raise ValueError("error: camera_intrinsics has not been set!!")
        if args.camera_distortion_coeffs is None:
            raise ValueError("error: camera_distortion_coeffs has not been set!!")
        return model, size, parse_values(args.camera_intrinsics), parse_values(args.camera_distortion_coeffs)
    log("try to get the camera model automatically")
    info = _first(bag, camera_info_topic, "CameraInfo", reader.decode_camera_info)
    if info is None:
        raise ValueError(f"error: no sensor_msgs/CameraInfo message on camera_info topic '{camera_info_topic}' in {bag.path} (name --camera_model and the intrinsics instead)")
    model, intrinsics, distortion = rosbag1.camera_from_info(info)
    return model, size, intrinsics, distortion


def time_field(cloud):
    """The cloud's per-point time field (ros_cloud_converter.hpp:81-84: the last one listed of ``TIME_FIELDS``), or ``None``"""
    field = None
    for f in cloud.fields:
        if f.name in TIME_FIELDS:
            field = f
    return field


def frame_times(cloud, where):
    """What ``TimeKeeper.process`` needs of a frame (extract_raw_points, ros_cloud_converter.hpp:121-142): ``(stamp, first, last,
    min)`` with ``first`` = ``None`` when the cloud has no time field or no points; ``min`` is a callable (one pass over the column,
    run only if a time is negative).  uint32 times are nanoseconds (``/ 1e9``)."""
    stamp = rosbag1.stamp_to_sec(cloud.stamp)
    field = time_field(cloud)
    n = rosbag1.num_points(cloud)
    if field is None or n == 0:
        return stamp, None, None, None
    if field.datatype not in (rosbag1.UINT32, rosbag1.FLOAT32, rosbag1.FLOAT64):
        raise ValueError(f"error: unsupported time type {field.datatype} of field '{field.name}' {where}")
    if field.offset + np.dtype(rosbag1.DATATYPE_DTYPES[field.datatype]).itemsize > cloud.point_step:
        raise ValueError(f"error: time field '{field.name}' lies outside the {cloud.point_step}-byte record {where}")
    scale = 1e9 if field.datatype == rosbag1.UINT32 else 1.0
    first, last = (float(v) / scale for v in rosbag1.read_field(cloud, field, [0, n - 1]))
    return stamp, first, last, lambda: float(rosbag1.read_field_all(cloud, field).min()) / scale


def integrate_bag(args, bag, points_topic, intensity_channel, integrator, warn=_warn, reader=rosbag1, lidar=None):
    """:442-460: every PointCloud2 message of the topic -- or the cloud ``reader.decode_points`` makes of a VelodyneScan or CustomMsg
    message; ``lidar``: the run's ``lidar_messages.LidarOptions`` --, in the view's order, through the time keeper and into the integrator.
    Returns ``(frames inserted, frames skipped for a rewinding stamp, points skipped for a non-finite coordinate)``.  An integrator
    with ``insert_cloud2_timed`` (the dynamic one) also gets the frame's per-point times, as the time field and the affine map of
    ``TimeKeeper.process_times``."""
    keeper = preprocess.TimeKeeper(log=warn)
    timed = getattr(integrator, "insert_cloud2_timed", None)
    inserted = rewound = nonfinite = 0
    # (Ouster packets arrive here as one message per scan: ``batch_points`` groups them; every other message passes through it untouched)
    scans = reader.batch_points(bag.messages(points_topic), lidar=lidar, warn=warn, where=f"(points topic '{points_topic}' in {bag.path})")
    for k, m in enumerate(scans):
        where = f"(message {k} of points topic '{points_topic}' in {bag.path})"
        if lidar_messages.points_kind(m.type) is None:
            break  # read_next returns nullptr at the first message that does not instantiate (src/preprocess_ros1.cpp:33-36)
        cloud = reader.decode_points(m.type, m.data, lidar=lidar, device=getattr(args, "device", 0), where=where)
        names = [f.name for f in cloud.fields]
        if any(c not in names for c in ("x", "y", "z")):
            raise ValueError(f"error: missing point coordinate fields {where}: the cloud has {', '.join(names)}")
        if intensity_channel not in names:
            raise ValueError(f"error: no intensity channel '{intensity_channel}' {where}: the cloud has {', '.join(names)}")
        if cloud.is_bigendian:
            raise ValueError(f"error: big-endian point data is not read {where}")
        if cloud.data.size < rosbag1.num_points(cloud) * cloud.point_step:
            raise ValueError(f"error: {cloud.data.size} data bytes for {cloud.width} x {cloud.height} points of {cloud.point_step} bytes {where}")
        times = frame_times(cloud, where)
        if timed is None:
            keep = keeper.process(*times)
        else:
            field = time_field(cloud) if times[1] is not None else None
            keep, scale, shift = keeper.process_times(*times, raw_scale=1e-9 if field is not None and field.datatype == rosbag1.UINT32 else 1.0)
        if not keep:
            warn("warning: skip frame with an invalid timestamp!!")
            rewound += 1
            continue
        try:
            if timed is None:
                nonfinite += integrator.insert_cloud2(cloud, intensity_channel)
            else:
                nonfinite += timed(cloud, intensity_channel, None if field is None else (field.offset, field.datatype), scale, shift)
        except ValueError as e:
            raise ValueError(f"error: {e} {where}") from None
        inserted += 1
    return inserted, rewound, nonfinite


def ouster_metadata(args, bag, points_topic, reader=rosbag1):
    """``--ouster_metadata`` and ``--ouster_frame`` as ``lidar_messages.OusterInfo``: the JSON of the named file, or with ``auto`` the first
    message of a ``std_msgs/String`` topic of the bag whose name ends in ``metadata``"""
    source, frame = getattr(args, "ouster_metadata", "auto") or "auto", getattr(args, "ouster_frame", "sensor")
    if source != "auto":
        with open(source) as f:
            return lidar_messages.ouster_info(f.read(), frame, where=source)
    for topic, type_ in bag.topics_and_types():
        if topic.endswith("metadata") and (type_.endswith("/String") or type_ == "String"):
            m = bag.first_message(topic, "String")
            if m is not None:
                where = f"the first message of topic '{topic}' in {bag.path}"
                return lidar_messages.ouster_info(reader.decode_string(m.data), frame, where=where)
    raise ValueError(f"error: points topic '{points_topic}' in {bag.path} holds Ouster packets, and the bag has no std_msgs/String topic whose name ends in 'metadata': "
                     "name the sensor's metadata JSON with --ouster_metadata FILE.json")


def lidar_options(args, bag, points_topic, log=print, reader=rosbag1):
    """``--lidar_model`` and ``--velodyne_calibration`` as ``lidar_messages.LidarOptions`` when the points topic is a VelodyneScan one;
    for any other topic they are ignored, with one logged line if either was given, and the result is ``None``.  ``--ouster_metadata``
    and ``--ouster_frame`` likewise: options with the sensor's ``OusterInfo`` when the points topic is a PacketMsg one, else one logged
    line if either was given."""
    lidar_model, calibration = getattr(args, "lidar_model", "auto"), getattr(args, "velodyne_calibration", None)
    kinds = [lidar_messages.points_kind(type_) for topic, type_ in bag.topics_and_types() if topic == points_topic]
    if "PacketMsg" not in kinds and (getattr(args, "ouster_metadata", "auto") not in (None, "auto") or getattr(args, "ouster_frame", "sensor") != "sensor"):
        log(f"--ouster_metadata and --ouster_frame are ignored: points topic '{points_topic}' is not an ouster_ros/PacketMsg topic")
    if "VelodyneScan" in kinds:
        return lidar_messages.LidarOptions(lidar_model, calibration)
    if lidar_model != "auto" or calibration:
        log(f"--lidar_model and --velodyne_calibration are ignored: points topic '{points_topic}' is not a velodyne_msgs/VelodyneScan topic")
    if "PacketMsg" in kinds:
        return lidar_messages.LidarOptions(ouster=ouster_metadata(args, bag, points_topic, reader=reader))
    return None


def run(args, log=print, warn=_warn, integrator_factory=preprocess.StaticPointCloudIntegrator, reader=rosbag1):
    """The steps of the module docstring; ``reader`` is the module that opens and decodes the bags: ``rosbag1``, or ``rosbag2`` for
    ``preprocess_ros2``, which has the same surface"""
    log(f"data_path: {args.data_path}")
    log(f"dst_path : {args.dst_path}")
    bag_filenames = find_bags(args.data_path, reader)
    log("input_bags:")
    for f in bag_filenames:
        log(f"- {f}")
    if not bag_filenames:
        raise ValueError("error: no input bags!!")
    if args.bag_id is not None:
        if not 0 <= args.bag_id < len(bag_filenames):
            raise ValueError(f"error: --bag_id {args.bag_id} with {len(bag_filenames)} bag(s)")
        warn(f"use only {bag_filenames[args.bag_id]}")
        bag_filenames = [bag_filenames[args.bag_id]]
    if args.first_n_bags is not None:
        bag_filenames = bag_filenames[: max(0, args.first_n_bags)]
        warn("use only the following rosbags:")
        for f in bag_filenames:
            warn(f"- {f}")
        if not bag_filenames:
            raise ValueError("error: no input bags!!")

    first = reader.Bag(bag_filenames[0])
    camera_info_topic, image_topic, points_topic = get_topics(args, first, log=log, warn=warn)
    log("selected topics:")
    log(f"- camera_info: {camera_info_topic}")
    log(f"- image      : {image_topic}")
    log(f"- points     : {points_topic}")
    lidar = lidar_options(args, first, points_topic, log=log, reader=reader)
    intensity_channel = get_intensity_channel(args, first, points_topic, reader=reader)
    log(f"intensity_channel: {intensity_channel}")
    camera_model, image_size, intrinsics, distortion = get_camera_params(args, first, camera_info_topic, image_topic, log=log, reader=reader)
    log(f"camera_model: {camera_model}")
    log(f"image_size  : {image_size[0]} {image_size[1]}")
    log(f"intrinsics  : {' '.join(f'{v:g}' for v in intrinsics)}")
    log(f"dist_coeffs : {' '.join(f'{v:g}' for v in distortion)}")

    bags = []
    for i, filename in enumerate(bag_filenames):
        log(f"start processing {filename}")
        bag = first if i == 0 else reader.Bag(filename)
        image = preprocess.equalize_hist(get_image(bag, image_topic, device=args.device, reader=reader))  # :414-419
        integ = integrator_factory(voxel_resolution=args.voxel_resolution, min_distance=args.min_distance, device=args.device)
        try:
            inserted, rewound, nonfinite = integrate_bag(args, bag, points_topic, intensity_channel, integ, warn=warn, reader=reader, lidar=lidar)
            records = integ.get_records()
        finally:
            integ.close()
        if records.shape[0] == 0:
            raise ValueError(f"error: no points left of points topic '{points_topic}' in {filename} ({inserted} frame(s) inserted, {rewound} skipped)")
        log(f"frames={inserted} skipped_frames={rewound} skipped_points={nonfinite} voxels={records.shape[0]}")
        points, intensities = preprocess.equalized_cloud(records, device=args.device)  # :464-473
        bags.append((os.path.basename(filename), image, points, intensities))
        log(f"processed {filename}")

    meta = {"data_path": args.data_path, "camera_info_topic": camera_info_topic, "image_topic": image_topic, "points_topic": points_topic,
            "intensity_channel": intensity_channel}  # :220-226
    log("save LiDAR images")
    config, lidar_fov = preprocess.save_preprocessed(args.dst_path, (camera_model, intrinsics, distortion), bags, meta, device=args.device, log=log)
    log("save meta data")
    return config, lidar_fov


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(_attach_values(sys.argv[1:] if argv is None else list(argv)))
    if args.data_path is None or args.dst_path is None:  # :73-76: the usage
        parser.print_help()
        return 0
    if args.dynamic_lidar_integration:
        print("error: dynamic LiDAR integration (-d, CT-GICP) is a command of its own: python -m direct_visual_lidar_calibration_amd.preprocess_dynamic <bags> <dst> "
              "takes the same options. This command runs the static integration path only; run it without -d.", file=sys.stderr)
        return 1
    try:
        run(args)
    except (OSError, ValueError) as e:
        msg = str(e)
        print(msg if msg.startswith("error:") else f"error: {msg}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
