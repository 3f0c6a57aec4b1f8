"""``preprocess`` on the MI355X engine, from ROS2 bags (sqlite3 or MCAP storage): a directory of bags in, the preprocessed directory
``preprocess_ros1`` writes out.

    python -m direct_visual_lidar_calibration_amd.preprocess_ros2 bags/ data/ -a
    python -m direct_visual_lidar_calibration_amd.preprocess_ros2 bags/ data/ -a -d --target_num_points 10000

Mirrors ``vlcal::Preprocess::run`` with its ROS2 back end (src/preprocess_ros2.cpp).  The steps are ``preprocess_ros1.run``'s -- that
module's docstring lists them and its differences from the reference, which all hold here, refusals and their wording included -- with
``rosbag2`` in the place of ``rosbag1`` as the reader.  No kernel is new: the ``data`` sequence of a CDR-serialised
``sensor_msgs/msg/PointCloud2`` holds the same records as the ROS1 message, and a zero-copy view of them goes to the same GPU decode
(``StaticPointCloudIntegrator.insert_cloud2``; with ``-d``, ``odometry.DynamicPointCloudIntegrator``).  What differs from ``preprocess_ros1``
and from the reference:

* ``-d / --dynamic_lidar_integration`` is honoured, as the reference's ROS2 ``preprocess -d`` is: it runs the dynamic integrator of
  ``preprocess_dynamic`` and takes that command's ``--target_num_points``, ``--seed`` and ``--lru_thresh`` with its defaults and checks
  (without ``-d`` the three are accepted and unused);
* an entry of ``data_path`` is a bag by ``rosbag2.valid_bag``: a directory with ``metadata.yaml``, a bare ``.db3`` or a bare ``.mcap``;
  ROS1 ``.bag`` files are ignored.  The bag's name in the output is the entry's file or directory name;
* ``sensor_msgs/msg/Image`` or ``CompressedImage`` is chosen by the topic's RECORDED TYPE, as ``preprocess_ros1`` does.  The reference looks
  for ``"compressed"`` in the topic NAME (src/preprocess_ros2.cpp:114,136) and deserialises the wrong type for a compressed topic named
  otherwise, or a raw one whose name contains the word;
* ``rosbag2`` lists what it does not read: big-endian CDR, a compression whose module does not import.  The reader is unpinned against
  ``rosbag2_cpp``, Fast-CDR and libmcap.
"""
import sys

from . import odometry, preprocess_dynamic, preprocess_ros1, rosbag2
from .preprocess_map import _attach_values


def build_parser():
    p = preprocess_ros1.build_parser()
    p.prog = "preprocess_ros2"
    for action in p._actions:
        if action.dest == "dynamic_lidar_integration":
            action.help = "create target point cloud from dynamic LiDAR data (CT-GICP odometry and deskewed integration)"
        elif action.dest == "k_neighbors":
            action.help = "num of neighbor points used for point covariance estimation of CT-ICP (with -d)"
    return preprocess_dynamic.add_dynamic_options(p)


def run(args, **kw):
    if args.dynamic_lidar_integration:
        kw.setdefault("integrator_factory", preprocess_dynamic.integrator_factory(args))
    return preprocess_ros1.run(args, reader=rosbag2, **kw)


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(_attach_values(sys.argv[1:] if argv is None else list(argv)))
    if args.data_path is None or args.dst_path is None:  # preprocess.cpp:73-76: the usage
        parser.print_help()
        return 0
    try:
        run(args)
    except (OSError, ValueError, odometry.ModelFullError) as e:
        msg = str(e)
        print(msg if msg.startswith("error:") else f"error: {msg}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
