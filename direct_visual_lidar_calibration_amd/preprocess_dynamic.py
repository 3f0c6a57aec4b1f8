"""``preprocess -d`` on the MI355X engine, from ROS1 bags: the LiDAR is carried through the scene, every scan is registered against a
running model with continuous-time GICP and deskewed, and all raw points go into the voxel grid (``odometry``).

    python -m direct_visual_lidar_calibration_amd.preprocess_dynamic bags/ data/ -a
    python -m direct_visual_lidar_calibration_amd.preprocess_dynamic bags/ data/ -a --target_num_points 10000 --k_neighbors 20 --seed 0

``preprocess_ros1.run`` with ``odometry.DynamicPointCloudIntegrator`` in the place of the static integrator: the same options, topics,
camera parameters, per-bag outputs and ``calib.json`` (``preprocess_ros1`` lists the differences from the reference; ``odometry`` those of
the integrator).  ``--k_neighbors`` is used here; ``--target_num_points`` and ``--seed`` (the scan sampler's) are extensions: the reference
fixes 10000 and seeds ``std::mt19937`` by default; ``--lru_thresh`` (the model forgets a voxel unused for that many scans; 0: never) is
an extension too: the reference fixes 100.  ``-d`` is accepted and implied.  ``--min_distance`` is honoured, in the odometry frame.
"""
import functools
import sys

from . import odometry, preprocess_ros1
from .preprocess_map import _attach_values


def add_dynamic_options(p):
    """The options of the dynamic integrator that ``preprocess_ros1``'s parser does not have (``preprocess_ros2 -d`` takes them too)"""
    p.add_argument("--target_num_points", type=int, default=10000, help="points a scan is sampled down to for the registration")
    p.add_argument("--seed", type=int, default=0, help="seed of the scan sampler")
    p.add_argument("--lru_thresh", type=int, default=100, help="extension: scans after which the registration model drops a voxel it neither inserted into nor searched "
                   "(the reference fixes 100); 0 keeps every voxel")
    return p


def build_parser():
    p = preprocess_ros1.build_parser()
    p.prog = "preprocess_dynamic"
    p.description = "preprocess with dynamic LiDAR integration"
    return add_dynamic_options(p)


def integrator_factory(args):
    """The checks of the dynamic options, then the factory ``preprocess_ros1.run`` builds one integrator per bag with"""
    if args.k_neighbors < 2 or args.k_neighbors > 32:
        raise ValueError(f"error: --k_neighbors {args.k_neighbors}: 2..32 neighbours are supported")
    if args.target_num_points < args.k_neighbors:
        raise ValueError(f"error: --target_num_points {args.target_num_points} is below --k_neighbors {args.k_neighbors}")
    if args.lru_thresh < 0:
        raise ValueError(f"error: --lru_thresh {args.lru_thresh}: must be >= 0 (0 disables the eviction)")
    return functools.partial(odometry.DynamicPointCloudIntegrator, k_neighbors=args.k_neighbors, target_num_points=args.target_num_points, seed=args.seed, lru_thresh=args.lru_thresh)


def run(args, **kw):
    return preprocess_ros1.run(args, integrator_factory=integrator_factory(args), **kw)


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(_attach_values(sys.argv[1:] if argv is None else list(argv)))
    if args.data_path is None or args.dst_path is None:
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
