"""GPU parity tests proper: the HIP path (through the C ABI) against the CPU oracle on the same
seeded inputs.  Run with ``pytest -m gpu`` on an MI355X.

Tolerances (ours; the reference defines none -- SURVEY.md section 7):
  * NEAREST (CostCalculatorNID): integer joint histogram BIT-EXACT; NID abs <= 1e-12.
  * SPLINE  (NIDCost), fp64: the bars of tests/parity.py, set from the margins the suite observes (raw joint histogram abs
    <= 1e-9 per bin -- fixed point 2^-39..2^-40 per tap --, NID abs <= 1e-11, 7-gradient rel <= 5e-10 + abs 1e-11).
"""
import numpy as np
import pytest

import oracle_lib
import parity
from direct_visual_lidar_calibration_amd import _lib, nid, se3, synth

pytestmark = pytest.mark.gpu

CAMERAS = {
    "plumb_bob": ("plumb_bob", [210.0, 205.0, 160.0, 120.0], [-0.04, 0.08, 1e-4, -3e-4, -0.04], 320, 240),
    "fisheye": ("fisheye", [140.0, 140.0, 160.0, 120.0], [-0.01, 0.002, -1e-4, 1e-5], 320, 240),
    "omnidir": ("omnidir", [110.0, 110.0, 160.0, 160.0, 1.0], [-0.02, 0.003, 1e-4, -2e-4], 320, 320),
    "equirectangular": ("equirectangular", [384.0, 256.0], [], 384, 256),
    "atan": ("atan", [210.0, 205.0, 160.0, 120.0], [0.6], 320, 240),
    "rational_polynomial": ("rational_polynomial", [210.0, 205.0, 160.0, 120.0], [0.05, -0.02, 1e-4, -2e-4, 0.01, 0.03, -0.01, 0.002], 320, 240),
}

_scene_cache = {}


def scene_for(name, n=30000, seed=11):
    key = (name, n, seed)
    if key not in _scene_cache:
        _scene_cache[key] = synth.make_scene(CAMERAS[name], num_points=n, seed=seed)
    return _scene_cache[key]


def oracle_nid(s, bins, x, **kw):
    return oracle_lib.nid_cost(s.model, s.intrinsics, s.distortion, s.image_f64, s.points, s.intensities, bins, x, **kw)


@pytest.mark.parametrize("model", list(CAMERAS))
def test_project_matches_oracle(model):
    s = scene_for(model, n=2000)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    T = se3.to_matrix(s.T_camera_lidar_true)
    pc = s.points[:, :3] @ T[:3, :3].T + T[:3, 3]
    uv, jac = proj.project(pc, jacobian=True)
    ruv, rjac = oracle_lib.project_jacobian(s.model, s.intrinsics, s.distortion, pc)
    assert np.allclose(uv, ruv, rtol=1e-12, atol=1e-9)
    assert np.allclose(jac, rjac, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("model", list(CAMERAS))
@pytest.mark.parametrize("bins", [16, 256])
def test_spline_value_gradient_histogram(model, bins):
    s = scene_for(model)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    cost = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, bins)
    assert cost.info()["float32_records"] == 1  # synthetic clouds are PLY-float32 representable
    for x in (s.T_camera_lidar_init, s.T_camera_lidar_true):
        ref = oracle_nid(s, bins, x, want_hist=True)
        ok, c, g = cost(x)
        assert ok and ref["ok"]
        parity.check_cost(c, ref["cost"])
        parity.check_grad(g, ref["grad"])
        joint, hi, hp = cost.histograms()
        parity.check_hist(joint, ref["hist"])
        parity.check_hist(hi, ref["hist_image"], kind="hist_image")
        assert np.array_equal(hp, ref["hist_points"])  # integer inlier counts per column
        # cost-only instantiation (T = double) gives the same value
        ok2, c2, g2 = cost(x, want_grad=False)
        assert ok2 and g2 is None and c2 == c
    cost.close()


def test_spline_is_deterministic_and_tiling_independent():
    """Fixed-point accumulation: the histogram (hence the cost) is bit-identical across repeated
    runs, workgroup counts and column-group widths."""
    s = scene_for("plumb_bob")
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    x = s.T_camera_lidar_init
    ref = None
    for gw, tb in [(16, 0), (16, 37), (1, 64), (4, 500), (64, 8), (256, 16)]:
        cost = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 256, columns_per_group=gw, target_blocks=tb)
        for _ in range(2):
            ok, c, g = cost(x)
            fx, inl, frac = cost.histogram_fixed()
            if ref is None:
                ref = (fx.copy(), inl, c)
            assert np.array_equal(fx, ref[0]) and inl == ref[1]
            assert c == ref[2]
        cost.close()


def test_single_column_specialisations_match_generic_kernels():
    """B = 256 with default tuning runs the WIDE histogram kernel (512 threads, 32 copies, v_perm
    addressing) and the GW1 gradient kernel; an explicit lds_copies / columns_per_group selects the
    generic kernels.  Same fixed-point histogram bit for bit, same cost, gradient equal to rounding --
    for float records and double records."""
    s = scene_for("fisheye", n=40000)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    x = s.T_camera_lidar_init
    pts64 = s.points.copy()
    pts64[:, :3] += 1e-9 * np.random.default_rng(0).normal(size=(pts64.shape[0], 3))  # not float-representable -> Rec64
    for pts, prec in ((s.points, "fp64"), (pts64, "fp64")):
        wide = nid.NIDCost(proj, s.image_f64, pts, s.intensities, 256, precision=prec)
        assert wide.info()["lds_copies"] == 32
        generic = nid.NIDCost(proj, s.image_f64, pts, s.intensities, 256, precision=prec, lds_copies=16)
        multi = nid.NIDCost(proj, s.image_f64, pts, s.intensities, 256, precision=prec, columns_per_group=4)
        assert generic.info()["lds_copies"] == 16
        ok0, c0, g0 = wide(x)
        h0 = wide.histogram_fixed()
        for other in (generic, multi):
            ok1, c1, g1 = other(x)
            h1 = other.histogram_fixed()
            assert ok0 and ok1 and c0 == c1
            assert np.array_equal(h0[0], h1[0]) and h0[1] == h1[1]
            assert np.allclose(g0, g1, rtol=1e-11, atol=1e-14)
        if prec == "fp64":
            ref = oracle_lib.nid_cost(s.model, s.intrinsics, s.distortion, s.image_f64, pts, s.intensities, 256, x)
            parity.check_cost(c0, ref["cost"])
            parity.check_grad(g0, ref["grad"])
        for c in (wide, generic, multi):
            c.close()


def test_spline_double_records_when_not_float_representable():
    s = scene_for("plumb_bob", n=8000)
    pts = s.points.copy()
    pts[:, :3] += 1e-9 * np.arange(pts.shape[0])[:, None]  # no longer float32-exact
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    cost = nid.NIDCost(proj, s.image_f64, pts, s.intensities, 16)
    assert cost.info()["float32_records"] == 0 and cost.info()["record_bytes"] == 32
    x = s.T_camera_lidar_init
    ref = oracle_lib.nid_cost(s.model, s.intrinsics, s.distortion, s.image_f64, pts, s.intensities, 16, x)
    ok, c, g = cost(x)
    assert ok
    parity.check_cost(c, ref["cost"])
    parity.check_grad(g, ref["grad"])
    cost.close()


def test_float_geometry_mode_is_gone():
    """NIDREG_PREC_FP32 (float transform / projection, rounds 1-4) bought 8 % on the headline for |dNID| <= 2e-5 and was removed in
    round 5 rather than kept half-built: the flag is refused with a message, never silently computed in double."""
    s = scene_for("plumb_bob", n=2000)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    with pytest.raises(ValueError, match="removed"):
        nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 16, precision="fp32")
    with pytest.raises(RuntimeError, match="NIDREG_PREC_FP32 was removed"):
        nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 16, precision=1)


def test_spline_edge_cases():
    s = scene_for("plumb_bob", n=5000)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    # (a) every point behind / outside: sum == 0 -> NaN -> functor returns false (nid_cost.hpp:98-102)
    far = se3.compose(s.T_camera_lidar_true, np.array([0, 0, 0, 1, 0, 0, 500.0]))
    x_out = se3.compose(np.array([0, 1.0, 0, 0, 0, 0, 0]), far)  # 180 deg about y then pushed away
    cost = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 16)
    ref = oracle_nid(s, 16, x_out)
    ok, c, g = cost(x_out)
    assert ok == ref["ok"]
    # (b) empty cloud
    empty = nid.NIDCost(proj, s.image_f64, np.zeros((0, 4)), np.zeros(0), 16)
    ok, c, g = empty(s.T_camera_lidar_true)
    assert not ok
    empty.close()
    # (c) points exactly at the camera centre (division by zero in the projection) and NaNs
    pts = s.points.copy()
    Tinv = np.linalg.inv(se3.to_matrix(s.T_camera_lidar_true))
    pts[0, :3] = Tinv[:3, 3]
    pts[1, :3] = np.nan
    ints = s.intensities.copy()
    ints[2] = 1.5  # clamps to the last bin
    ints[3] = -0.2  # clamps to bin 0
    c2 = nid.NIDCost(proj, s.image_f64, pts, ints, 16)
    ref = oracle_lib.nid_cost(s.model, s.intrinsics, s.distortion, s.image_f64, pts, ints, 16, s.T_camera_lidar_true, want_hist=True)
    ok, c, g = c2(s.T_camera_lidar_true)
    assert ok == ref["ok"]
    parity.check_cost(c, ref["cost"])
    joint, hi, hp = c2.histograms()
    assert np.array_equal(hp, ref["hist_points"])
    c2.close()
    # (d) unnormalised quaternion: the reference differentiates the un-normalised formula
    xq = s.T_camera_lidar_init.copy()
    xq[:4] *= 1.01
    ref = oracle_nid(s, 16, xq)
    ok, c, g = cost(xq)
    assert ok == ref["ok"]
    parity.check_cost(c, ref["cost"])
    parity.check_grad(g, ref["grad"])
    cost.close()


@pytest.mark.parametrize("bins", [16, 256])
def test_ragged_cloud_sizes_around_the_batch_and_wave_boundaries(bins):
    """Clouds of 1 ... 4097 points around every boundary of the point loops: one wave (64), one batch slot (256 / 512 threads), one
    full batch (1024 records for the 256-thread kernels, 2048 for the WIDE histogram kernel), and one record more or less.  The
    full batches run straight-line, the last batch of a segment is guarded and skips the slots that lie past the end for a whole
    wave (nid_kernels.hpp spline_hist_body): every size must give the oracle's histogram, cost and gradient."""
    s = scene_for("plumb_bob", n=4097)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    x = s.T_camera_lidar_init
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097):
        pts, ints = s.points[:n], s.intensities[:n]
        ref = oracle_lib.nid_cost(s.model, s.intrinsics, s.distortion, s.image_f64, pts, ints, bins, x, want_hist=True)
        for tuning in ({}, {"target_blocks": 1}):  # the library's chunk rule, and everything in ONE workgroup (several batches + a ragged tail)
            cost = nid.NIDCost(proj, s.image_f64, pts, ints, bins, **tuning)
            ok, c, g = cost(x)
            assert ok == ref["ok"], (n, tuning)
            joint, hi, hp = cost.histograms()
            assert np.array_equal(hp, ref["hist_points"]), (n, tuning)
            parity.check_hist(joint, ref["hist"])
            if ok:
                parity.check_cost(c, ref["cost"])
                parity.check_grad(g, ref["grad"])
            cost.close()
    # the NEAREST twin (one guarded loop, four records per thread): integer histogram bit for bit at the same sizes
    max_fov = oracle_lib.estimate_camera_fov(s.model, s.intrinsics, s.distortion, s.width, s.height)
    T = se3.to_matrix(x)
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 4097):
        pts, ints = s.points[:n], s.intensities[:n]
        ref_cost, ref_hist = oracle_lib.cost_calculator_nid(s.model, s.intrinsics, s.distortion, s.image_u8, pts, ints, bins, max_fov, T, want_hist=True)
        calc = nid.CostCalculatorNID(proj, s.image_u8, pts, ints, nid.NIDCostParams(bins), max_fov=max_fov)
        calc.calculate(T)
        fx, inl, frac = calc.histogram_fixed()
        assert frac == 0 and np.array_equal(fx, ref_hist) and inl == ref_hist.sum(), n
        calc.close()


def test_border_points_contribute_clamped_taps():
    """Knots on the image border keep their 16 taps with clamped pixel coordinates
    (nid_cost.hpp:70-73): a cloud projected onto the first/last rows and columns."""
    model, intr, dist, W, H = CAMERAS["plumb_bob"]
    s = scene_for("plumb_bob", n=4000)
    rng = np.random.default_rng(3)
    uv = np.stack([rng.uniform(0, W, 4000), rng.uniform(0, H, 4000)], -1)
    uv[:1000, 0] = rng.uniform(0, 1, 1000)
    uv[1000:2000, 0] = rng.uniform(W - 1, W, 1000)
    uv[2000:3000, 1] = rng.uniform(0, 1, 1000)
    uv[3000:, 1] = rng.uniform(H - 1, H, 1000)
    import torch

    from direct_visual_lidar_calibration_amd import camera_models

    bear = camera_models.unproject(model, intr, dist, torch.tensor(uv)).numpy()
    T = se3.to_matrix(s.T_camera_lidar_true)
    pc = bear * rng.uniform(2.0, 9.0, (4000, 1))
    pl = (pc - T[:3, 3]) @ T[:3, :3]
    pts = np.concatenate([pl.astype(np.float32).astype(np.float64), np.ones((4000, 1))], -1)
    ints = rng.integers(0, 256, 4000) / 256.0
    proj = nid.create_camera(model, intr, dist)
    cost = nid.NIDCost(proj, s.image_f64, pts, ints, 64)
    ref = oracle_lib.nid_cost(model, intr, dist, s.image_f64, pts, ints, 64, s.T_camera_lidar_true, want_hist=True)
    ok, c, g = cost(s.T_camera_lidar_true)
    assert ok
    parity.check_cost(c, ref["cost"])
    joint, _, hp = cost.histograms()
    parity.check_hist(joint, ref["hist"])
    assert np.array_equal(hp, ref["hist_points"])
    parity.check_grad(g, ref["grad"])
    cost.close()


@pytest.mark.parametrize("model", list(CAMERAS))
@pytest.mark.parametrize("bins", [16, 256])
def test_nearest_integer_histogram_bit_exact(model, bins):
    s = scene_for(model)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    max_fov = oracle_lib.estimate_camera_fov(s.model, s.intrinsics, s.distortion, s.width, s.height)
    calc = nid.CostCalculatorNID(proj, s.image_u8, s.points, s.intensities, nid.NIDCostParams(bins), max_fov=max_fov)
    rng = np.random.default_rng(5)
    for k in range(3):
        x = synth.random_pose_near(s.T_camera_lidar_true, rng) if k else s.T_camera_lidar_true
        T = se3.to_matrix(x)
        ref_cost, ref_hist = oracle_lib.cost_calculator_nid(s.model, s.intrinsics, s.distortion, s.image_u8, s.points, s.intensities, bins, max_fov, T, want_hist=True)
        c = calc.calculate(T)
        fx, inl, frac = calc.histogram_fixed()
        assert frac == 0
        assert np.array_equal(fx, ref_hist)
        assert inl == ref_hist.sum()
        assert abs(c - ref_cost) <= 1e-12
    calc.close()


def test_estimate_camera_fov_matches_oracle():
    for model in ("plumb_bob", "fisheye", "omnidir"):
        s = scene_for(model, n=2000)
        proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
        a = nid.estimate_camera_fov(proj, (s.width, s.height))
        b = oracle_lib.estimate_camera_fov(s.model, s.intrinsics, s.distortion, s.width, s.height)
        assert abs(a - b) < 1e-6


def test_multi_nid_cost_sum_and_trust_gate():
    s1 = scene_for("plumb_bob", n=12000, seed=21)
    s2 = scene_for("plumb_bob", n=9000, seed=22)
    proj = nid.create_camera(s1.model, s1.intrinsics, s1.distortion)
    init = s1.T_camera_lidar_true
    multi = nid.MultiNIDCost(init)
    for s in (s1, s2):
        multi.add(nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 16))
    pairs = [(s.image_f64, s.points, s.intensities) for s in (s1, s2)]
    x = se3.plus(init, np.array([0.01, -0.02, 0.015, 0.004, -0.003, 0.002]))
    ok, c, g = multi(x)
    rok, rc, rg = oracle_lib.multi_nid_cost(s1.model, s1.intrinsics, s1.distortion, pairs, 16, init, x)
    assert ok and rok
    parity.check_cost(c, rc, atol=4 * parity.COST_ATOL)  # a sum over the set's pairs
    parity.check_grad(g, rg)
    # outside the 0.2 m / 2 deg gate -> false without evaluating
    for delta in ([0.25, 0, 0, 0, 0, 0], [0, 0, 0, 0, np.radians(2.5), 0]):
        xg = se3.plus(init, np.array(delta, dtype=float))
        ok, _, _ = multi(xg)
        rok, _, _ = oracle_lib.multi_nid_cost(s1.model, s1.intrinsics, s1.distortion, pairs, 16, init, xg)
        assert not ok and not rok
    for c_ in multi.costs:
        c_.close()


def test_create_camera_error_behaviour():
    assert nid.create_camera("no_such_model", [1, 2, 3, 4], []) is None
    assert nid.create_camera("plumb_bob", [1, 2, 3], []) is None  # intrinsic count mismatch
    cam = nid.create_camera("plumb_bob", [1, 2, 3, 4], [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7])  # truncated to 5
    assert cam is not None and cam.distortion == [0.1, 0.2, 0.3, 0.4, 0.5]
    assert nid.create_camera("equidistant", [1, 2, 3, 4], []).model_id == nid.create_camera("fisheye", [1, 2, 3, 4], [0]).model_id
    with pytest.raises(RuntimeError):
        s = scene_for("plumb_bob", n=2000)
        proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
        nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 5000)  # bins > 4096 unsupported (257 ... 4096: the occupied bins)


def test_full_size_properties_cfg2_like():
    """Size-independent properties at (a slice of) BASELINE config 2's shape: 1080p pinhole, 256
    bins, 2M points: partition of unity (sum of the joint histogram == number of inliers, row sums ==
    hist_image, column sums == hist_points), shard additivity of the fixed-point histogram, and a
    central finite-difference check of the tangent gradient."""
    s = synth.make_scene("pinhole_1080p", num_points=2_000_000, seed=20250525, device="cuda:0")
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    x = s.T_camera_lidar_init
    full = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 256)
    ok, c, g = full(x)
    assert ok
    fx, inl, frac = full.histogram_fixed()
    joint, hi, hp = full.histograms()
    unit = 2.0**frac
    assert abs(fx.sum() / unit - inl) < 1e-3
    assert np.allclose(fx.sum(1) / unit, hi, atol=1e-6)
    assert np.array_equal(np.rint(fx.sum(0) / unit), hp) and hp.sum() == inl
    # shards: histograms of disjoint point slices add up exactly (what the RCCL all-reduce relies on)
    n = s.points.shape[0]
    acc = np.zeros_like(fx)
    acc_inl = 0
    for a, b in ((0, n // 3), (n // 3, n)):
        part = nid.NIDCost(proj, s.image_f64, s.points[a:b], s.intensities[a:b], 256)
        part(x, want_grad=False)
        pfx, pinl, pfrac = part.histogram_fixed()
        assert pfrac == frac
        acc += pfx
        acc_inl += pinl
        part.close()
    assert acc_inl == inl
    assert np.array_equal(acc, fx)  # integer fixed point: exactly additive
    # finite differences on the 6-D tangent, at a pose where every point is >= 1 px inside the
    # image (the inlier test makes NID discontinuous where points cross the border, which central
    # differences see and the Jet / analytic gradient by construction does not)
    xs = se3.plus(s.T_camera_lidar_true, np.array([4e-4, -3e-4, 5e-4, 2e-4, -1.5e-4, 1e-4]))
    ok, c, g = full(xs)
    assert ok and full.histogram_fixed()[1] == n
    gt = se3.plus_jacobian(xs).T @ g
    h = 1e-6
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        _, cp, _ = full(se3.plus(xs, e), want_grad=False)
        _, cm, _ = full(se3.plus(xs, -e), want_grad=False)
        fd = (cp - cm) / (2 * h)
        assert abs(fd - gt[k]) <= 1e-4 * max(1.0, abs(gt[k])), (k, fd, gt[k])
    full.close()


@pytest.mark.parametrize("model", list(CAMERAS))
def test_view_culling_indices_identical(model):
    """ViewCulling::cull on the GPU returns exactly the reference's surviving index list: FoV gate on
    the normalised 4-vector, in-image test, float depth buffer with the +0.1 m threshold."""
    s = scene_for(model, n=20000)
    T = se3.to_matrix(s.T_camera_lidar_init)
    Tinv = np.linalg.inv(T)
    pc = s.points[:5000, :3] @ T[:3, :3].T + T[:3, 3]
    far = pc * (1.0 + 1.0 / np.linalg.norm(pc, axis=1, keepdims=True))  # occluded copies 1 m behind
    near = pc * (1.0 + 0.05 / np.linalg.norm(pc, axis=1, keepdims=True))  # within the 0.1 m threshold
    behind = -pc
    extra = np.concatenate([far, near, behind]) @ Tinv[:3, :3].T + Tinv[:3, 3]
    pts = np.concatenate([s.points, np.concatenate([extra, np.ones((extra.shape[0], 1))], -1)])
    pts[7, :3] = np.nan
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    min_z = np.cos(oracle_lib.estimate_camera_fov(s.model, s.intrinsics, s.distortion, s.width, s.height))
    for depth in (True, False):
        vc = nid.ViewCulling(proj, (s.width, s.height), nid.ViewCullingParams(depth), min_z=min_z)
        got = vc.cull(pts, T)
        ref = oracle_lib.view_culling(s.model, s.intrinsics, s.distortion, s.width, s.height, pts, T, depth)
        assert np.array_equal(got, ref)
        assert 0 < got.shape[0] < pts.shape[0]
    # and with min_z estimated on the device-projection path (estimate_camera_fov restated on the host)
    vc = nid.ViewCulling(proj, (s.width, s.height))
    assert abs(vc.min_z - min_z) < 1e-6
    assert vc.cull(np.zeros((0, 4)), T).shape == (0,)


def test_sharded_cost_single_process_matches_plain():
    """ShardedNIDCost's device plumbing (torch-owned histogram / result buffers, torch's current
    stream, split-phase calls) on one GPU: two shards evaluated back to back into the SAME histogram
    buffer reproduce the unsharded result bit for bit (what the RCCL all-reduce does across ranks)."""
    import torch

    from direct_visual_lidar_calibration_amd import _lib, parallel

    s = scene_for("plumb_bob", n=30000)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    x = s.T_camera_lidar_init
    plain = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 64)
    ok, c, g = plain(x)
    fx, inl, frac = plain.histogram_fixed()
    # world-size-1 path of the product class
    sh = parallel.ShardedNIDCost(proj, s.image_f64, s.points, s.intensities, 64, device=0)
    ok1, c1, g1 = sh(x)
    assert ok1 and c1 == c and np.array_equal(g1, g)
    ok2, c2, g2 = sh(x, want_grad=False)
    assert ok2 and c2 == c and g2 is None
    sh.close()
    # two shards, manual "all-reduce" = sum of the two fixed-point buffers on the device
    n = s.points.shape[0]
    lo, hi = parallel.shard_slice(n, 0, 2), parallel.shard_slice(n, 1, 2)
    backs = [parallel._GpuShardBackend(proj, s.image_f64, s.points[a:b], s.intensities[a:b], 64, n, 0, "fp64") for a, b in (lo, hi)]
    for b in backs:
        b.shard_hist(x)
    # no host sync: the kernels run on torch's current stream, so torch ops are ordered behind them
    total = backs[0].hist_tensor + backs[1].hist_tensor
    B = 64
    assert int(total[B * B].item()) == inl
    assert np.array_equal(total[: B * B].cpu().numpy().reshape(B, B).T, fx)  # device layout [bin_points][bin_image]
    grads = []
    for b in backs:
        b.hist_tensor.copy_(total)
        b.shard_entropy()
        b.shard_grad()
    gsum = (backs[0].grad_tensor + backs[1].grad_tensor).cpu().numpy()
    oks = [b.shard_finish(True) for b in backs]
    assert all(o[0] for o in oks) and oks[0][1] == c and oks[1][1] == c
    assert np.allclose(gsum, g, rtol=1e-12, atol=1e-15)
    for b in backs:
        b.cost.close()
    plain.close()


@pytest.mark.parametrize("bins", [2, 7, 100, 255])
def test_spline_and_nearest_odd_bin_counts(bins):
    """nid_bins is a free integer in the reference (calibrate.cpp:176); non-power-of-two counts change
    the LDS tiling (columns per workgroup, ragged last group)."""
    s = scene_for("plumb_bob", n=15000)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    x = s.T_camera_lidar_init
    cost = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, bins)
    ref = oracle_nid(s, bins, x, want_hist=True)
    ok, c, g = cost(x)
    assert ok == ref["ok"]
    parity.check_cost(c, ref["cost"])
    parity.check_grad(g, ref["grad"])
    joint, hi, hp = cost.histograms()
    assert np.array_equal(hp, ref["hist_points"])
    parity.check_hist(joint, ref["hist"])
    cost.close()
    max_fov = oracle_lib.estimate_camera_fov(s.model, s.intrinsics, s.distortion, s.width, s.height)
    calc = nid.CostCalculatorNID(proj, s.image_u8, s.points, s.intensities, nid.NIDCostParams(bins), max_fov=max_fov)
    T = se3.to_matrix(x)
    rc, rh = oracle_lib.cost_calculator_nid(s.model, s.intrinsics, s.distortion, s.image_u8, s.points, s.intensities, bins, max_fov, T, want_hist=True)
    c = calc.calculate(T)
    assert np.array_equal(calc.histogram_fixed()[0], rh) and abs(c - rc) <= 1e-12
    calc.close()


@pytest.mark.parametrize("camera,n", [("pinhole_1080p", 300000), ("pinhole_4k", 300000), ("equirect_2k", 300000), ("fisheye_1080p", 300000), ("omnidir_2k", 300000)])
def test_baseline_config_cameras_at_scale(camera, n):
    """The camera models of BASELINE configs 2-5 at their full image sizes -- including the shape the
    bench line is quoted on (configs[1], 1920x1080 plumb_bob) and configs[4]'s 3840x2160 image, which
    no longer fits one XCD's L2 -- with the cloud reduced so the oracle finishes in seconds: value,
    gradient, histogram; and the NEAREST twin's integer histogram bit for bit."""
    s = synth.make_scene(camera, num_points=n, seed=20250530, device="cuda:0")
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    x = s.T_camera_lidar_init
    cost = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 256)
    ref = oracle_nid(s, 256, x, want_hist=True)
    ok, c, g = cost(x)
    assert ok and ref["ok"]
    parity.check_cost(c, ref["cost"])
    parity.check_grad(g, ref["grad"])
    joint, hi, hp = cost.histograms()
    assert np.array_equal(hp, ref["hist_points"])
    parity.check_hist(joint, ref["hist"])
    cost.close()
    max_fov = oracle_lib.estimate_camera_fov(s.model, s.intrinsics, s.distortion, s.width, s.height)
    calc = nid.CostCalculatorNID(proj, s.image_u8, s.points, s.intensities, nid.NIDCostParams(256), max_fov=max_fov)
    T = se3.to_matrix(x)
    rc, rh = oracle_lib.cost_calculator_nid(s.model, s.intrinsics, s.distortion, s.image_u8, s.points, s.intensities, 256, max_fov, T, want_hist=True)
    cn = calc.calculate(T)
    assert np.array_equal(calc.histogram_fixed()[0], rh) and abs(cn - rc) <= 1e-12
    calc.close()


def test_headline_workload_10m_points_matches_oracle():
    """BASELINE configs[1] exactly as bench.py runs it (10M-point cloud, 1920x1080 plumb_bob, 256 bins,
    same seed) against the oracle with its OpenMP split over points on every host core (~1 s of CPU):
    the 32-bit chunk arithmetic, the one-round chunk tables and the fraction-bit choice at full N
    (frac = 38) are oracle-checked, not only property-checked."""
    import torch

    s = synth.make_scene("pinhole_1080p", num_points=10_000_000, seed=20250523 + 2, device="cuda:0" if torch.cuda.is_available() else "cpu")
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    cost = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 256)
    info = cost.info()
    assert info["num_points"] == 10_000_000 and info["lds_copies"] == 32 and info["frac_bits"] == 38
    rng = np.random.default_rng(1234)
    x = synth.random_pose_near(s.T_camera_lidar_true, rng)
    ref = oracle_nid(s, 256, x, want_hist=True, threads=oracle_lib.num_threads())
    ok, c, g = cost(x)
    assert ok and ref["ok"]
    parity.check_cost(c, ref["cost"])
    parity.check_grad(g, ref["grad"])
    joint, hi, hp = cost.histograms()
    # 2^-38 per tap, <= ~2500 taps in the fullest bin; the oracle's own double sums round at ~1e-12 there
    assert np.array_equal(hp, ref["hist_points"])
    parity.check_hist(joint, ref["hist"], atol=parity.hist_atol_for(ref["hist"], info["frac_bits"]), what="10M points")
    assert hp.sum() == ref["hist_points"].sum()
    cost.close()


@pytest.mark.parametrize("camera,n,seed", [("equirect_2k", 10_000_000, 20250523 + 3), ("omnidir_2k", 10_000_000, 20250523 + 3), ("fisheye_1080p", 5_000_000, 20250523 + 4)])
def test_config_cameras_full_size_match_oracle(camera, n, seed):
    """BASELINE configs[2] (10M points, 2048 x 2048 equirectangular, and its omnidir variant) and one pair of configs[3] (5M points,
    1920 x 1080 fisheye) at their FULL point counts, 256 bins, exactly as bench.py's `configs` leg builds them: value, gradient,
    marginals and joint histogram against the oracle with its OpenMP split over points (1-2 s of CPU each), and the NEAREST twin's
    integer histogram bit for bit.  What only shows at this size: the 32-bit chunk arithmetic, frac = 38 / 39, the table `atan2`
    at 10^7 evaluations per pass, the Morton order of a 360-degree cloud, 2048^2 / 4 MB bin images against one XCD's L2."""
    import torch

    s = synth.make_scene(camera, num_points=n, seed=seed, device="cuda:0" if torch.cuda.is_available() else "cpu")
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    cost = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 256)
    info = cost.info()
    assert info["num_points"] == n and info["frac_bits"] == (38 if n > 2**23 else 39)
    rng = np.random.default_rng(99)
    x = synth.random_pose_near(s.T_camera_lidar_true, rng)
    ref = oracle_nid(s, 256, x, want_hist=True, threads=oracle_lib.num_threads())
    ok, c, g = cost(x)
    assert ok and ref["ok"]
    parity.check_cost(c, ref["cost"], what=f"{camera} {n}")
    parity.check_grad(g, ref["grad"], what=f"{camera} {n}")
    joint, hi, hp = cost.histograms()
    assert np.array_equal(hp, ref["hist_points"]) and hp.sum() == ref["hist_points"].sum()
    parity.check_hist(joint, ref["hist"], atol=parity.hist_atol_for(ref["hist"], info["frac_bits"]), what=f"{camera} {n} points")
    ok2, c2, _ = cost(x, want_grad=False)
    assert ok2 and c2 == c
    cost.close()
    max_fov = oracle_lib.estimate_camera_fov(s.model, s.intrinsics, s.distortion, s.width, s.height)
    calc = nid.CostCalculatorNID(proj, s.image_u8, s.points, s.intensities, nid.NIDCostParams(256), max_fov=max_fov)
    T = se3.to_matrix(x)
    rc, rh = oracle_lib.cost_calculator_nid(s.model, s.intrinsics, s.distortion, s.image_u8, s.points, s.intensities, 256, max_fov, T, want_hist=True)
    cn = calc.calculate(T)
    fx, inl, frac = calc.histogram_fixed()
    assert frac == 0 and np.array_equal(fx, rh) and int(fx.sum()) == inl and abs(cn - rc) <= 1e-12
    calc.close()


@pytest.mark.parametrize("shards", [2, 3])
def test_equirect_pair_sharded_at_a_million_points(shards):
    """configs[2]'s shape -- one equirectangular pair cut over several GPUs -- with the shards co-located on the one GPU of the
    test box, at 1.5M points (every shard holds whole column groups of a 360-degree cloud): the set's cost is the plain handle's
    bit for bit, cost / gradient / histogram meet the oracle's bars."""
    import torch

    s = synth.make_scene("equirect_2k", num_points=1_500_000, seed=20250523 + 3, device="cuda:0" if torch.cuda.is_available() else "cpu")
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    rng = np.random.default_rng(5)
    poses = [synth.random_pose_near(s.T_camera_lidar_true, rng) for _ in range(3)]
    plain = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 256)
    sharded = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 256, devices=[0] * shards)
    assert sharded.info()["num_points"] == 1_500_000
    ref = oracle_nid(s, 256, poses[0], want_hist=True, threads=oracle_lib.num_threads())
    for k, x in enumerate(poses):
        okp, cp, gp = plain(x)
        oks, cs, gs = sharded(x)
        assert okp and oks and cs == cp, (k, cs, cp)
        assert np.allclose(gs, gp, rtol=1e-11, atol=1e-14)
        assert np.array_equal(sharded.histogram_fixed()[0], plain.histogram_fixed()[0])
        if k == 0:
            parity.check_cost(cs, ref["cost"], what=f"equirect {shards} shards")
            parity.check_grad(gs, ref["grad"], what=f"equirect {shards} shards")
            parity.check_hist(sharded.histograms()[0], ref["hist"], atol=parity.hist_atol_for(ref["hist"], sharded.info()["frac_bits"]), what=f"equirect {shards} shards")
        okc, cc, _ = sharded(x, want_grad=False)
        assert okc and cc == cp
    sharded.close()
    plain.close()


def test_eight_fisheye_pairs_as_one_grid_match_the_summed_oracle():
    """configs[3]'s shape on ONE GPU: eight fisheye pairs (8 x 600k points, 1920 x 1080, 256 bins) through MultiNIDCost -- a single
    grid per pass over all pairs -- against the sum of the oracle's eight costs / gradients (visual_camera_calibration.cpp:166-170),
    and every pair's own cost against its oracle."""
    import torch

    dev = "cuda:0" if torch.cuda.is_available() else "cpu"
    scenes = [synth.make_scene("fisheye_1080p", num_points=600_000, seed=20250523 + 40 + k, device=dev) for k in range(8)]
    proj = nid.create_camera(scenes[0].model, scenes[0].intrinsics, scenes[0].distortion)
    x = synth.random_pose_near(scenes[0].T_camera_lidar_true, np.random.default_rng(3), dt=0.02, drot_deg=0.2)
    handles = [nid.NIDCost(proj, sc.image_f64, sc.points, sc.intensities, 256) for sc in scenes]
    multi = nid.MultiNIDCost(None)
    for h in handles:
        multi.add(h)
    refs = [oracle_nid(sc, 256, x, threads=oracle_lib.num_threads()) for sc in scenes]
    ok, c, g = multi(x)
    assert ok and all(r["ok"] for r in refs)
    parity.check_cost(c, sum(r["cost"] for r in refs), atol=8 * parity.COST_ATOL, what="8 fisheye pairs, one grid")
    parity.check_grad(g, sum(r["grad"] for r in refs), atol=8 * parity.GRAD_ATOL, what="8 fisheye pairs, one grid")
    for h, r in zip(handles, refs):
        okh, ch, gh = h(x)
        assert okh
        parity.check_cost(ch, r["cost"], what="fisheye pair of the 8")
        parity.check_grad(gh, r["grad"], what="fisheye pair of the 8")
    for h in handles:
        h.close()


@pytest.mark.parametrize("bins", [300, 512, 4096])
def test_bins_above_256_run_on_the_occupied_bins(bins):
    """The reference takes any --nid_bins (src/calibrate.cpp:175); its 8-bit images and 256-level intensities occupy at most
    256 bins per axis however many there are.  A handle with bins > 256 runs on the occupied bins, relabelled 0, 1, 2, ... --
    the NID depends on the multiset of cells and the marginals only -- and must give the oracle's value and gradient AT THAT
    BIN COUNT, the bits of the same data at 256 bins, and histograms in the caller's own B x B layout.  SPLINE and NEAREST,
    plain / device-resident cloud / sharded."""
    s = scene_for("plumb_bob", n=30011)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    rng = np.random.default_rng(12)
    poses = [s.T_camera_lidar_init, synth.random_pose_near(s.T_camera_lidar_true, rng)]
    wide = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, bins)
    b256 = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 256)
    cl = nid.Cloud(s.points, s.intensities)
    from_cloud = nid.NIDCost.from_cloud(proj, s.image_f64, cl, bins)
    sharded = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, bins, devices=[0, 0, 0])
    for k, x in enumerate(poses):
        ok, c, g = wide(x)
        ok2, c2, g2 = b256(x)
        assert ok and ok2 and c == c2 and np.array_equal(g, g2)  # a monotone relabelling of the same 256 x 256 cells
        ok3, c3, g3 = from_cloud(x)
        assert ok3 and c3 == c and np.allclose(g3, g, rtol=1e-11, atol=1e-14)
        ok4, c4, g4 = sharded(x)
        assert ok4 and c4 == c and np.allclose(g4, g, rtol=1e-11, atol=1e-14)
        if k == 0 and bins <= 512:  # (the oracle's Jet histogram at 4096 bins is 1 GB: the 256-bin identity above covers it)
            ref = oracle_nid(s, bins, x, want_hist=True)
            parity.check_cost(c, ref["cost"], what=f"bins {bins}")
            parity.check_grad(g, ref["grad"], what=f"bins {bins}")
            joint, hi, hp = wide.histograms()
            assert joint.shape == (bins, bins)
            parity.check_hist(joint, ref["hist"], atol=parity.hist_atol_for(ref["hist"], wide.info()["frac_bits"]), what=f"bins {bins}")
            assert np.array_equal(hp, ref["hist_points"])
            assert np.allclose(hi, ref["hist_image"], rtol=0, atol=1e-8)
            js, _, _ = sharded.histograms()
            assert np.array_equal(js, joint)
    for h in (wide, b256, from_cloud, sharded):
        h.close()
    cl.close()
    # the derivative-free twin: integer histogram in the caller's layout, bit for bit
    if bins <= 512:
        max_fov = oracle_lib.estimate_camera_fov(s.model, s.intrinsics, s.distortion, s.width, s.height)
        calc = nid.CostCalculatorNID(proj, s.image_u8, s.points, s.intensities, nid.NIDCostParams(bins), max_fov=max_fov)
        T = se3.to_matrix(poses[1])
        rc, rh = oracle_lib.cost_calculator_nid(s.model, s.intrinsics, s.distortion, s.image_u8, s.points, s.intensities, bins, max_fov, T, want_hist=True)
        cn = calc.calculate(T)
        fx, inl, frac = calc.histogram_fixed()
        assert frac == 0 and fx.shape == (bins, bins) and np.array_equal(fx, rh) and int(fx.sum()) == inl and abs(cn - rc) <= 1e-12
        calc.close()


def test_nearest_twin_10m_points_bit_exact():
    """CostCalculatorNID::calculate (cost_calculator_nid.cpp:21-67) on the headline cloud: the integer joint histogram of
    10M points bit for bit against the oracle's serial loop (~1 s of CPU), NID to 1e-12."""
    import torch

    s = synth.make_scene("pinhole_1080p", num_points=10_000_000, seed=20250523 + 2, device="cuda:0" if torch.cuda.is_available() else "cpu")
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    max_fov = oracle_lib.estimate_camera_fov(s.model, s.intrinsics, s.distortion, s.width, s.height)
    calc = nid.CostCalculatorNID(proj, s.image_u8, s.points, s.intensities, nid.NIDCostParams(256), max_fov=max_fov)
    rng = np.random.default_rng(77)
    T = se3.to_matrix(synth.random_pose_near(s.T_camera_lidar_true, rng))
    rc, rh = oracle_lib.cost_calculator_nid(s.model, s.intrinsics, s.distortion, s.image_u8, s.points, s.intensities, 256, max_fov, T, want_hist=True)
    c = calc.calculate(T)
    fx, inl, frac = calc.histogram_fixed()
    assert frac == 0 and np.array_equal(fx, rh) and int(fx.sum()) == inl
    assert abs(c - rc) <= 1e-12
    calc.close()


def test_dense_map_50m_points_4k_image_matches_oracle():
    """BASELINE configs[4] at its full size: 50M-point map, 3840x2160 plumb_bob, 256 bins.  At this N the fixed-point
    fraction drops to 36 bits (62 - bits(N)), the 32-bit chunk arithmetic sees offsets up to 8e8 bytes and the 8 MB bin image
    no longer fits one XCD's L2; the oracle runs with its OpenMP split over points on every host core."""
    import torch

    s = synth.make_scene("pinhole_4k", num_points=50_000_000, seed=20250523 + 5, device="cuda:0" if torch.cuda.is_available() else "cpu")
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    cost = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 256)
    info = cost.info()
    assert info["num_points"] == 50_000_000 and info["frac_bits"] == 36
    rng = np.random.default_rng(4321)
    x = synth.random_pose_near(s.T_camera_lidar_true, rng)
    ref = oracle_nid(s, 256, x, want_hist=True, threads=oracle_lib.num_threads())
    ok, c, g = cost(x)
    assert ok and ref["ok"]
    parity.check_cost(c, ref["cost"])
    parity.check_grad(g, ref["grad"])
    joint, hi, hp = cost.histograms()
    # 2^-36 per tap, <= ~12 000 taps in the fullest bin
    assert np.array_equal(hp, ref["hist_points"])
    parity.check_hist(joint, ref["hist"], atol=parity.hist_atol_for(ref["hist"], info["frac_bits"]), what="50M points")
    assert hp.sum() == ref["hist_points"].sum()
    ok2, c2, g2 = cost(x, want_grad=False)
    assert ok2 and c2 == c
    cost.close()


@pytest.mark.parametrize("model", ["plumb_bob", "fisheye", "equirectangular"])
def test_device_resident_cull_and_build_matches_host_path(model):
    """nidreg_create_from_cloud: ViewCulling + bucketing + sort + gather on the GPU gives the same handle
    contents as the host path fed with the CPU-culled cloud: identical fixed-point histogram, cost and
    gradient (the record order may differ; the sums do not)."""
    s = scene_for(model, n=30000)
    T = se3.to_matrix(s.T_camera_lidar_init)
    Tinv = np.linalg.inv(T)
    pc = s.points[:6000, :3] @ T[:3, :3].T + T[:3, 3]
    extra = np.concatenate([pc * (1.0 + 1.0 / np.linalg.norm(pc, axis=1, keepdims=True)), -pc]) @ Tinv[:3, :3].T + Tinv[:3, 3]
    pts = np.concatenate([s.points, np.concatenate([extra, np.ones((extra.shape[0], 1))], -1)])
    ints = np.concatenate([s.intensities, s.intensities[:6000], s.intensities[:6000]])
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    min_z = np.cos(oracle_lib.estimate_camera_fov(s.model, s.intrinsics, s.distortion, s.width, s.height))
    idx = oracle_lib.view_culling(s.model, s.intrinsics, s.distortion, s.width, s.height, pts, T, True)
    cloud = nid.Cloud(pts, ints)
    x = s.T_camera_lidar_init
    for bins in (16, 256):
        host = nid.NIDCost(proj, s.image_f64, pts[idx], ints[idx], bins)
        dev = nid.NIDCost.from_cloud(proj, s.image_f64, cloud, bins, cull=(T, min_z, True))
        assert dev.num_points == idx.shape[0] == host.num_points
        ok_h, c_h, g_h = host(x)
        ok_d, c_d, g_d = dev(x)
        assert ok_h and ok_d and c_d == c_h
        assert np.array_equal(dev.histogram_fixed()[0], host.histogram_fixed()[0])
        assert np.allclose(g_d, g_h, rtol=1e-12, atol=1e-15)  # partial sums are grouped differently
        host.close()
        dev.close()
    # no culling: every point, and the NEAREST twin
    dev = nid.NIDCost.from_cloud(proj, s.image_f64, cloud, 64)
    host = nid.NIDCost(proj, s.image_f64, pts, ints, 64)
    assert dev(x, want_grad=False)[1] == host(x, want_grad=False)[1]
    dev.close()
    host.close()
    max_fov = float(np.arccos(min_z))
    cd = nid.CostCalculatorNID.from_cloud(proj, s.image_u8, cloud, nid.NIDCostParams(16), max_fov=max_fov, cull=(T, min_z, True))
    ch = nid.CostCalculatorNID(proj, s.image_u8, pts[idx], ints[idx], nid.NIDCostParams(16), max_fov=max_fov)
    assert cd.calculate(T) == ch.calculate(T) and np.array_equal(cd.histogram_fixed()[0], ch.histogram_fixed()[0])
    cd.close()
    ch.close()
    # a cloud that is not float32-representable keeps double records
    c2 = nid.Cloud(pts + np.array([1e-9, 0, 0, 0]), ints)
    d2 = nid.NIDCost.from_cloud(proj, s.image_f64, c2, 16)
    assert d2.info()["record_bytes"] == 32
    d2.close()
    c2.close()
    cloud.close()


def test_concurrent_handles_from_host_threads_and_no_leaks():
    """The reference evaluates one NIDCost per OpenMP thread (visual_camera_calibration.cpp:161):
    concurrent nidreg_eval on DIFFERENT handles from different host threads must be safe and give
    the single-threaded bits.  Also: create/destroy in a loop does not leak device memory."""
    import threading

    import torch

    scenes = [scene_for("plumb_bob", n=20000, seed=60 + k) for k in range(4)]
    proj = nid.create_camera(scenes[0].model, scenes[0].intrinsics, scenes[0].distortion)
    costs = [nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 64) for s in scenes]
    rng = np.random.default_rng(9)
    poses = [synth.random_pose_near(scenes[0].T_camera_lidar_true, rng) for _ in range(25)]
    serial = [[c(x) for x in poses] for c in costs]
    results = [None] * len(costs)

    def work(k):
        results[k] = [costs[k](x) for x in poses]

    threads = [threading.Thread(target=work, args=(k,)) for k in range(len(costs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for k in range(len(costs)):
        for (ok_a, c_a, g_a), (ok_b, c_b, g_b) in zip(serial[k], results[k]):
            assert ok_a == ok_b and c_a == c_b and np.array_equal(g_a, g_b)
    for c in costs:
        c.close()
    s = scenes[0]
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(60):
        c = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 256)
        c(poses[0])
        c.close()
        cl = nid.Cloud(s.points, s.intensities)
        d = nid.NIDCost.from_cloud(proj, s.image_f64, cl, 16)
        d.close()
        cl.close()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 64 * 1024 * 1024


@pytest.mark.parametrize("nshards", [2, 3, 5])
def test_in_library_sharding_matches_plain_handle(nshards):
    """desc.num_devices > 1 (here: the same GPU listed several times -- all a 1-GPU box offers; the peer-mapped
    fine-grained flag blocks and histogram replicas, k_entropy_repl's push / wait are the ones a multi-GPU node runs): the
    points are cut along the histogram column, every shard owns a range of column groups and stores its columns into every
    shard's replica of the integer histogram -- one exchange per evaluation.  Histogram and cost are
    bit-identical to the unsharded handle, the gradient equal up to summation order -- SPLINE and NEAREST, 16 and 256 bins,
    a cloud size that does not divide evenly."""
    s = scene_for("plumb_bob", n=30011)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    rng = np.random.default_rng(5)
    poses = [s.T_camera_lidar_init] + [synth.random_pose_near(s.T_camera_lidar_true, rng) for _ in range(6)]
    for bins in (16, 100, 256):
        plain = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, bins)
        sh = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, bins, devices=[0] * nshards)
        assert sh.num_shards() == nshards and sh.shard_devices() == [0] * nshards and plain.num_shards() == 1
        assert sh.info()["num_points"] == s.points.shape[0]
        for x in poses:  # back to back: both histogram buffers, flag sequence numbers
            ok, c, g = plain(x)
            ok1, c1, g1 = sh(x)
            assert ok and ok1 and c1 == c
            assert np.allclose(g1, g, rtol=1e-12, atol=1e-15)
            assert np.array_equal(sh.histogram_fixed()[0], plain.histogram_fixed()[0]) and sh.histogram_fixed()[1] == plain.histogram_fixed()[1]
            jp, hip_, hpp = plain.histograms()
            js, his, hps = sh.histograms()
            assert np.array_equal(js, jp) and np.array_equal(his, hip_) and np.array_equal(hps, hpp)
            ok2, c2, g2 = sh(x, want_grad=False)
            assert ok2 and c2 == c and g2 is None
        ref = oracle_nid(s, bins, poses[1])
        ok1, c1, g1 = sh(poses[1])
        parity.check_cost(c1, ref["cost"])
        parity.check_grad(g1, ref["grad"])
        # nothing projects: every shard reports zero inliers, the functor returns false like the reference's 0 / 0
        far = np.array(poses[1], dtype=np.float64).copy()
        far[4:7] += 1.0e4
        okf, cf, gf = sh(far)
        assert not okf and not np.isfinite(cf)
        okb, cb, gb = sh(poses[2])
        assert okb and cb == plain(poses[2])[1]
        plain.close()
        sh.close()
    max_fov = oracle_lib.estimate_camera_fov(s.model, s.intrinsics, s.distortion, s.width, s.height)
    T = se3.to_matrix(poses[2])
    near = nid.CostCalculatorNID(proj, s.image_u8, s.points, s.intensities, nid.NIDCostParams(64), max_fov=max_fov)
    near_sh = nid.CostCalculatorNID(proj, s.image_u8, s.points, s.intensities, nid.NIDCostParams(64), max_fov=max_fov, devices=[0] * nshards)
    assert near_sh.calculate(T) == near.calculate(T)
    assert np.array_equal(near_sh.histogram_fixed()[0], near.histogram_fixed()[0])
    near.close()
    near_sh.close()


def test_sharding_a_device_resident_cloud_with_culling():
    """nidreg_create_from_cloud honours desc.device_ids: ViewCulling + bucketing + sort on the cloud's GPU, then every shard
    takes the records of its column groups device to device -- same bits as the unsharded device-resident handle (BASELINE
    configs[4]: a map culled on the GPU every outer iteration, visual_camera_calibration.cpp:199-208, on several GPUs)."""
    s = scene_for("plumb_bob", n=40000)
    T = se3.to_matrix(s.T_camera_lidar_init)
    Tinv = np.linalg.inv(T)
    pc = s.points[:8000, :3] @ T[:3, :3].T + T[:3, 3]
    extra = np.concatenate([pc * (1.0 + 1.0 / np.linalg.norm(pc, axis=1, keepdims=True)), -pc]) @ Tinv[:3, :3].T + Tinv[:3, 3]
    pts = np.concatenate([s.points, np.concatenate([extra, np.ones((extra.shape[0], 1))], -1)])
    ints = np.concatenate([s.intensities, s.intensities[:8000], s.intensities[:8000]])
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    min_z = np.cos(oracle_lib.estimate_camera_fov(s.model, s.intrinsics, s.distortion, s.width, s.height))
    cloud = nid.Cloud(pts, ints)
    rng = np.random.default_rng(8)
    poses = [s.T_camera_lidar_init] + [synth.random_pose_near(s.T_camera_lidar_true, rng) for _ in range(3)]
    for bins in (16, 256):
        one = nid.NIDCost.from_cloud(proj, s.image_f64, cloud, bins, cull=(T, min_z, True))
        many = nid.NIDCost.from_cloud(proj, s.image_f64, cloud, bins, cull=(T, min_z, True), devices=[0, 0, 0, 0])
        assert many.num_shards() == 4 and many.num_points == one.num_points and many.info()["frac_bits"] == one.info()["frac_bits"]
        for x in poses:
            ok1, c1, g1 = one(x)
            okm, cm, gm = many(x)
            assert ok1 and okm and cm == c1 and np.allclose(gm, g1, rtol=1e-12, atol=1e-15)
            assert np.array_equal(many.histogram_fixed()[0], one.histogram_fixed()[0])
        one.close()
        many.close()
    cloud.close()


def test_nidreg_devices_environment_shards_an_unchanged_caller(monkeypatch):
    """NIDREG_DEVICES: the caller passes nothing about GPUs (the reference's `new NIDCost(proj, image, points, bins)`,
    visual_camera_calibration.cpp:206) and the handle is sharded all the same; MultiNIDCost over a sharded and a plain
    pair sums like the reference's."""
    s = scene_for("fisheye", n=20000)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    x = s.T_camera_lidar_init
    plain = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 16)
    monkeypatch.setenv("NIDREG_DEVICES", "0,0")
    sh = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 16)
    monkeypatch.delenv("NIDREG_DEVICES")
    assert sh.num_shards() == 2 and plain.num_shards() == 1
    ok, c, g = plain(x)
    ok1, c1, g1 = sh(x)
    assert ok and ok1 and c1 == c and np.allclose(g1, g, rtol=1e-12, atol=1e-15)
    multi = nid.MultiNIDCost(x)
    multi.add(sh)
    multi.add(plain)
    okm, cm, gm = multi(x)
    assert okm and cm == c + c and np.allclose(gm, g1 + g, rtol=1e-13, atol=1e-16)
    plain.close()
    sh.close()


def test_points_on_knot_and_border_boundaries():
    """The SPLINE kernels divide by v_rcp_f64 + ONE Newton step (csrc/nid_device.hpp fast_rcp: <= 2^-46 relative, i.e.
    3e-11 px on a 2000-px coordinate) where the reference divides exactly.  Knot decisions near integer pixel coordinates
    cannot matter -- the cubic B-spline weights are continuous across knots (at s -> 1 the weights of knot k equal those of
    knot k + 1 at s = 0) -- and the in-image decision can only differ inside that band around the image border.  Points
    placed +-1e-12 .. 1e-9 px around knots, and >= 1e-9 px inside / outside the borders: same inlier count, histogram, cost
    and gradient as the oracle."""
    s = scene_for("plumb_bob", n=2000)
    W, H = s.width, s.height
    fx, fy, cx, cy = s.intrinsics[:4]
    dist = [0.0] * 5  # invertible in closed form
    rng = np.random.default_rng(12)
    n = 6000
    ku = rng.integers(2, W - 2, n).astype(np.float64)
    kv = rng.integers(2, H - 2, n).astype(np.float64)
    deltas = np.array([0.0, 1e-12, -1e-12, 1e-10, -1e-10, 1e-9, -1e-9])
    u = ku + deltas[rng.integers(0, len(deltas), n)]
    v = kv + deltas[rng.integers(0, len(deltas), n)]
    # borders: well-resolved distances only (>= 1e-9 px from the edge, on both sides)
    nb = 400
    edge = np.array([1e-9, -1e-9, 1e-6, -1e-6])
    ub = np.where(rng.random(nb) < 0.5, 0.0, float(W)) + edge[rng.integers(0, 4, nb)]
    vb = rng.uniform(5, H - 5, nb)
    u = np.concatenate([u, ub, rng.uniform(5, W - 5, nb)])
    v = np.concatenate([v, vb, np.where(rng.random(nb) < 0.5, 0.0, float(H)) + edge[rng.integers(0, 4, nb)]])
    z = rng.uniform(2.0, 30.0, u.shape[0])
    pts = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z, np.ones_like(z)], -1)
    ints = (np.floor(rng.random(u.shape[0]) * 256) / 256).astype(np.float64)
    x = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])  # p_cam = p: the placement survives the transform
    proj = nid.create_camera("plumb_bob", list(s.intrinsics[:4]), dist)
    for bins in (16, 256):
        cost = nid.NIDCost(proj, s.image_f64, pts, ints, bins)
        assert cost.info()["float32_records"] == 0  # these coordinates do not round-trip through float: double records
        ref = oracle_lib.nid_cost("plumb_bob", list(s.intrinsics[:4]), dist, s.image_f64, pts, ints, bins, x, want_hist=True)
        ok, c, g = cost(x)
        joint, hi, hp = cost.histograms()
        assert ok and ref["ok"] and np.array_equal(hp, ref["hist_points"])  # same inlier decisions
        parity.check_hist(joint, ref["hist"])
        parity.check_cost(c, ref["cost"])
        parity.check_grad(g, ref["grad"])
        cost.close()


def test_input_order_flag_and_strided_points():
    """NIDREG_FLAG_INPUT_ORDER (stable sort on the column-group bits only) and a point stride > 32 bytes: same bits."""
    from direct_visual_lidar_calibration_amd import _lib

    s = scene_for("plumb_bob", n=12000)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    x = s.T_camera_lidar_init
    a = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 64)
    b = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 64, flags=_lib.FLAG_INPUT_ORDER)
    ra, rb = a(x), b(x)
    assert ra[1] == rb[1]
    assert np.array_equal(a.histogram_fixed()[0], b.histogram_fixed()[0])
    assert np.allclose(ra[2], rb[2], rtol=1e-12, atol=1e-15)
    for h in (a, b):
        h.close()


@pytest.mark.parametrize("bins", [16, 256])
def test_outliers_and_padding_do_not_change_the_bits(bins):
    """The histogram kernels pick, per wave and per four points, between tap code with uniform constants (every lane an
    inlier) and with per-lane constants zeroed for outliers / padding slots.  Both must give a point the same bits:
    interleaving outliers (outside the image, behind the camera, NaN) with the cloud -- in the caller's order, so that
    they share waves with inliers -- changes neither the fixed-point histogram nor the cost, and only adds zeros to the
    gradient sums."""
    from direct_visual_lidar_calibration_amd import _lib

    s = scene_for("plumb_bob", n=24000)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    x = s.T_camera_lidar_true
    base = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, bins, flags=_lib.FLAG_INPUT_ORDER)
    ok, c, g = base(x)
    fx, inl, frac = base.histogram_fixed()
    assert ok and inl > 0.9 * s.points.shape[0]
    T = se3.to_matrix(x)
    Tinv = np.linalg.inv(T)
    rng = np.random.default_rng(12)
    n_out = 5000
    cam = np.stack([rng.uniform(-1, 1, n_out) * 50.0, rng.uniform(-1, 1, n_out) * 50.0, rng.uniform(0.2, 1.0, n_out)], -1)  # far outside the image
    cam[::3, 2] *= -1.0  # behind the camera (mirrored projection: still outside or inside? keep only those that fall outside below)
    outl = np.concatenate([cam @ Tinv[:3, :3].T + Tinv[:3, 3], np.ones((n_out, 1))], -1)
    outl[:, :3] = outl[:, :3].astype(np.float32).astype(np.float64)  # PLY-representable like the cloud: float32 records either way
    outl[::7, :3] = np.nan
    uv = oracle_lib.project(s.model, s.intrinsics, s.distortion, outl[:, :3] @ T[:3, :3].T + T[:3, 3])
    outside = ~((uv[:, 0] >= 0) & (uv[:, 0] < s.width) & (uv[:, 1] >= 0) & (uv[:, 1] < s.height))  # NaN compares false -> outside
    outl = outl[outside]
    assert outl.shape[0] > 2000
    # interleave: every 5th record of the mixed cloud is an outlier, intensities drawn from the cloud's own levels
    n = s.points.shape[0]
    k = min(outl.shape[0], n // 4)
    pts = np.empty((n + k, 4))
    ints = np.empty(n + k)
    mask = np.zeros(n + k, dtype=bool)
    mask[np.arange(k) * 5 + 2] = True
    pts[mask], pts[~mask] = outl[:k], s.points
    ints[mask], ints[~mask] = s.intensities[rng.integers(0, n, k)], s.intensities
    for flags in (_lib.FLAG_INPUT_ORDER, 0):
        mixed = nid.NIDCost(proj, s.image_f64, pts, ints, bins, flags=flags)
        ok2, c2, g2 = mixed(x)
        fx2, inl2, frac2 = mixed.histogram_fixed()
        assert ok2 and inl2 == inl and frac2 == frac
        assert np.array_equal(fx2, fx) and c2 == c
        assert np.allclose(g2, g, rtol=1e-12, atol=1e-15)
        mixed.close()
    base.close()


@pytest.mark.parametrize("bins", [16, 256])
def test_multi_pair_single_grid_matches_individual_evaluations(bins, monkeypatch):
    """nidreg_eval_multi over several compatible pairs on one GPU runs ONE grid per pass over all pairs' chunks (three
    launches in all).  Every pair keeps its own histogram, unit and scratch, so the result must be exactly the sum of
    the individual evaluations -- cost bit for bit, member histograms bit for bit -- for pairs of very different sizes,
    over repeated calls (both histogram buffers), cost-only calls, and with the single-grid path switched off."""
    sizes = [26000, 9000, 700, 15000]
    scenes = [scene_for("plumb_bob", n=n, seed=70 + k) for k, n in enumerate(sizes)]
    proj = nid.create_camera(scenes[0].model, scenes[0].intrinsics, scenes[0].distortion)
    costs = [nid.NIDCost(proj, s.image_f64, s.points, s.intensities, bins) for s in scenes]
    solo = [nid.NIDCost(proj, s.image_f64, s.points, s.intensities, bins) for s in scenes]
    rng = np.random.default_rng(21)
    poses = [scenes[0].T_camera_lidar_init] + [synth.random_pose_near(scenes[0].T_camera_lidar_true, rng) for _ in range(4)]
    multi = nid.MultiNIDCost(None)
    for c in costs:
        multi.add(c)
    for x in poses:
        ok, c, g = multi(x)
        parts = [s_(x) for s_ in solo]
        assert ok and all(p[0] for p in parts)
        csum = 0.0
        for p in parts:
            csum += p[1]
        assert c == csum
        assert np.allclose(g, sum(p[2] for p in parts), rtol=1e-12, atol=1e-15)
        for a, b in zip(costs, solo):
            assert np.array_equal(a.histogram_fixed()[0], b.histogram_fixed()[0]) and a.histogram_fixed()[1] == b.histogram_fixed()[1]
        ok2, c2, g2 = multi(x, want_grad=False)
        assert ok2 and c2 == csum and g2 is None
    # a member evaluated on its own afterwards (its own stream, its own chunk table) still agrees
    x = poses[2]
    assert costs[1](x)[1] == solo[1](x)[1]
    # the same through the per-pair launches
    monkeypatch.setenv("NIDREG_NO_MULTI_GRID", "1")
    ok3, c3, g3 = multi(poses[1])
    monkeypatch.delenv("NIDREG_NO_MULTI_GRID")
    ok4, c4, g4 = multi(poses[1])
    assert ok3 and ok4 and c3 == c4 and np.allclose(g3, g4, rtol=1e-12, atol=1e-15)
    # the trust gate still applies (visual_camera_calibration.cpp:152-156)
    gated = nid.MultiNIDCost(poses[0])
    for c in costs:
        gated.add(c)
    far = se3.plus(poses[0], np.array([0.3, 0.0, 0.0, 0.0, 0.0, 0.0]))
    assert gated(far)[0] is False
    # the Nelder-Mead objective's sum over pairs (nidreg_eval_iso_multi) through the same single-grid path
    max_fov = oracle_lib.estimate_camera_fov(scenes[0].model, scenes[0].intrinsics, scenes[0].distortion, scenes[0].width, scenes[0].height)
    calcs = [nid.CostCalculatorNID(proj, s.image_u8, s.points, s.intensities, nid.NIDCostParams(bins), max_fov=max_fov) for s in scenes]
    solo_calcs = [nid.CostCalculatorNID(proj, s.image_u8, s.points, s.intensities, nid.NIDCostParams(bins), max_fov=max_fov) for s in scenes]
    for x in poses[:3]:
        T = se3.to_matrix(x)
        tot = 0.0
        for cc in solo_calcs:
            tot += cc.calculate(T)
        assert nid.sum_costs(calcs, T) == tot
        for a, b in zip(calcs, solo_calcs):
            assert np.array_equal(a.histogram_fixed()[0], b.histogram_fixed()[0])
    for cc in calcs + solo_calcs:
        cc.close()
    # a group dies with any of its members; the rest keep working
    costs[2].close()
    rest = nid.MultiNIDCost(None)
    for k in (0, 1, 3):
        rest.add(costs[k])
    okr, cr, gr = rest(poses[3])
    assert okr and cr == solo[0](poses[3])[1] + solo[1](poses[3])[1] + solo[3](poses[3])[1]
    for c in costs + solo:
        c.close()


@pytest.mark.parametrize("model", ["plumb_bob", "equirectangular"])
def test_chunks_across_column_groups_match_one_group_per_chunk(model, monkeypatch):
    """Round 4: on a cloud whose histogram columns are unequally full (every view-culled cloud) a chunk is a contiguous range of
    records that may run across column groups; the workgroup flushes / re-zeroes its histogram tile, or switches to the next
    staged G column, at each boundary (csrc/nid_kernels.hpp Segments, the looped kernel instantiations).  Against tables of
    one group per chunk (NIDREG_MAX_SEGS=1, the rule of rounds 1-3): fixed-point histogram and cost bit for bit, gradient to
    rounding; against the oracle: the usual bars.  SPLINE (WIDE and generic histogram kernels, gradient) and NEAREST."""
    s = scene_for(model, n=120000, seed=31)
    rng = np.random.default_rng(2)
    col = np.minimum((s.intensities * 256).astype(int), 255)
    keep_p = rng.uniform(0.05, 1.0, 256)
    keep_p[rng.integers(0, 256, 40)] = 0.0  # empty columns too
    keep = rng.uniform(size=col.shape[0]) < keep_p[col]
    pts, ints = np.ascontiguousarray(s.points[keep]), np.ascontiguousarray(s.intensities[keep])
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    x = s.T_camera_lidar_init
    ref = oracle_lib.nid_cost(s.model, s.intrinsics, s.distortion, s.image_f64, pts, ints, 256, x, want_hist=True)
    # (tuning, NIDREG_SEG_OVERHEAD): the default cost model keeps a cloud this small on one group per chunk; a small per-segment
    # cost, or few workgroups, makes the chunks run across groups -- in the gradient table and in the WIDE histogram table
    for tuning, overhead, expect in (({}, None, None), ({}, "16", (None, 1)), ({"lds_copies": 16}, "16", None), ({"target_blocks": 40}, "384", (1, 1)), ({"target_blocks": 3000}, "0", None)):
        if overhead is not None:
            monkeypatch.setenv("NIDREG_SEG_OVERHEAD", overhead)
            monkeypatch.setenv("NIDREG_SEG_MIN_GAIN", "0")  # (by default a segmented table must win by 10 % in the cost model to be used)
        seg = nid.NIDCost(proj, s.image_f64, pts, ints, 256, **tuning)
        monkeypatch.setenv("NIDREG_MAX_SEGS", "1")
        one = nid.NIDCost(proj, s.image_f64, pts, ints, 256, **tuning)
        monkeypatch.delenv("NIDREG_MAX_SEGS")
        monkeypatch.delenv("NIDREG_SEG_OVERHEAD", raising=False)
        monkeypatch.delenv("NIDREG_SEG_MIN_GAIN", raising=False)
        assert (one.info()["segmented"], one.info()["segmented_hist"]) == (0, 0)
        if expect is not None:
            got = (seg.info()["segmented"], seg.info()["segmented_hist"])
            assert all(e is None or e == g_ for e, g_ in zip(expect, got)), (tuning, overhead, seg.info())
        for _ in range(2):  # both histogram buffers
            ok0, c0, g0 = seg(x)
            ok1, c1, g1 = one(x)
            assert ok0 and ok1 and c0 == c1
            h0, h1 = seg.histogram_fixed(), one.histogram_fixed()
            assert np.array_equal(h0[0], h1[0]) and h0[1] == h1[1]
            assert np.allclose(g0, g1, rtol=1e-11, atol=1e-14)
        parity.check_cost(c0, ref["cost"])
        parity.check_grad(g0, ref["grad"])
        joint, hi, hp = seg.histograms()
        parity.check_hist(joint, ref["hist"])
        assert np.array_equal(hp, ref["hist_points"])
        okc, cc, _ = seg(x, want_grad=False)
        assert okc and cc == c0
        seg.close()
        one.close()
    # NEAREST twin: integer histogram bit for bit against the oracle, with chunks across groups
    max_fov = oracle_lib.estimate_camera_fov(s.model, s.intrinsics, s.distortion, s.width, s.height)
    T = se3.to_matrix(x)
    ref_cost, ref_hist = oracle_lib.cost_calculator_nid(s.model, s.intrinsics, s.distortion, s.image_u8, pts, ints, 256, max_fov, T, want_hist=True)
    for bins, tb in ((256, 0), (256, 48), (16, 0)):
        if bins != 256:
            ref_cost, ref_hist = oracle_lib.cost_calculator_nid(s.model, s.intrinsics, s.distortion, s.image_u8, pts, ints, bins, max_fov, T, want_hist=True)
        monkeypatch.setenv("NIDREG_SEG_MIN_GAIN", "0")
        calc = nid.CostCalculatorNID(proj, s.image_u8, pts, ints, nid.NIDCostParams(bins), max_fov=max_fov, target_blocks=tb)
        monkeypatch.delenv("NIDREG_SEG_MIN_GAIN")
        if tb:
            assert calc.info()["segmented"] == 1
        for _ in range(2):
            c = calc.calculate(T)
            fx, inl, frac = calc.histogram_fixed()
            assert np.array_equal(fx, ref_hist) and inl == ref_hist.sum() and abs(c - ref_cost) <= 1e-12
        calc.close()


def test_destroyed_handles_leave_their_stream_and_result_blocks_to_the_next():
    """The reference builds a new NIDCost per pair in every outer iteration (visual_camera_calibration.cpp:199-208): a destroyed
    handle's stream and host-mapped result blocks are kept for the next handle on the device (nidreg_core.hip ResourcePool; creating
    them anew cost 0.9 of the 1.0 ms a small handle took).  A recycled block must not leak its previous owner's results or
    completion tags: handles of different clouds and bin counts created, evaluated (synchronously, through submit / wait and as
    a multi-pair grid) and destroyed in an interleaved order give what fresh handles gave; nidreg_trim() empties the lists."""
    from direct_visual_lidar_calibration_amd import _lib

    lib = _lib.load()
    scenes = [scene_for("plumb_bob", n=n, seed=300 + k) for k, n in enumerate((20_000, 33_000, 26_000))]
    proj = nid.create_camera(scenes[0].model, scenes[0].intrinsics, scenes[0].distortion)
    rng = np.random.default_rng(21)
    poses = [synth.random_pose_near(scenes[0].T_camera_lidar_true, rng) for _ in range(6)]

    def make(k, bins):
        sc = scenes[k]
        return nid.NIDCost(proj, sc.image_f64, sc.points, sc.intensities, bins)

    lib.nidreg_trim()
    ref = {}
    for k in range(3):
        for bins in (16, 256):
            c = make(k, bins)
            ref[k, bins] = [c(x) for x in poses]
            c.close()
            lib.nidreg_trim()  # every reference handle gets a new stream and new blocks
    live = []
    for rnd in range(4):
        for k in range(3):
            for bins in (16, 256):
                c = make(k, bins)  # (from the second handle on: a recycled stream, recycled blocks)
                j = (rnd + k) % len(poses)
                if rnd % 2:
                    t = [c.submit(poses[(j + i) % len(poses)]) for i in range(3)]
                    got = [c.wait(tk) for tk in t]
                    want = [ref[k, bins][(j + i) % len(poses)] for i in range(3)]
                else:
                    got, want = [c(poses[j])], [ref[k, bins][j]]
                for a, b in zip(got, want):
                    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]), (rnd, k, bins)
                live.append((k, bins, c))
                if len(live) > 2:  # destroyed out of creation order, two handles always alive
                    kk, bb, old = live.pop(0)
                    ok, cc, gg = old(poses[0])
                    assert cc == ref[kk, bb][0][1]
                    old.close()
        multi = nid.MultiNIDCost(None)
        group = [make(k, 256) for k in range(3)]
        for c in group:
            multi.add(c)
        ok, cm, gm = multi(poses[rnd])
        tot = 0.0
        for k in range(3):
            tot += ref[k, 256][rnd][1]
        assert ok and cm == tot
        for c in group:
            c.close()
    for _, _, c in live:
        c.close()
    lib.nidreg_trim()
    c = make(0, 16)
    assert c(poses[1])[1] == ref[0, 16][1][1]
    c.close()


def test_small_tables_need_no_entropy_kernel(monkeypatch):
    """bins <= 32 (the reference's default is 16): a cost+Jacobian evaluation launches two kernels -- every gradient workgroup
    sums the B x B table itself and clears the next evaluation's buffer (nid_kernels.hpp kSelfEntropyCells).  The sums are
    integers, so cost, marginals and gradient are the SAME BITS as with k_entropy (NIDREG_NO_SELF_ENTROPY=1), also when
    cost-only and cost+Jacobian evaluations alternate on the double-buffered histogram, for tables of several column groups,
    and through submit / wait."""
    s = scene_for("plumb_bob", n=60_000, seed=77)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    rng = np.random.default_rng(8)
    poses = [s.T_camera_lidar_init] + [synth.random_pose_near(s.T_camera_lidar_true, rng) for _ in range(5)]
    for bins, tuning in ((16, {}), (2, {}), (7, {}), (32, {}), (16, {"columns_per_group": 4}), (16, {"target_blocks": 3}), (33, {})):
        monkeypatch.setenv("NIDREG_NO_SELF_ENTROPY", "1")
        old = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, bins, **tuning)
        ref = [old(x) for x in poses]
        ref_marg = old.histograms()
        assert old.info()["grad_sums_table"] == 0
        monkeypatch.delenv("NIDREG_NO_SELF_ENTROPY")
        new = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, bins, **tuning)
        assert new.info()["grad_sums_table"] == (1 if bins <= 32 else 0)
        for j, x in enumerate(poses):
            if j % 2:
                okc, cc, _ = new(x, want_grad=False)  # k_entropy with its tail, between two evaluations that launch none
                assert okc and cc == ref[j][1]
            ok, c, g = new(x)
            assert ok == ref[j][0] and c == ref[j][1] and np.array_equal(g, ref[j][2]), (bins, tuning, j)
        for a, b in zip(new.histograms(), ref_marg):
            assert np.array_equal(a, b)
        oks, cs, gs = new.eval_batch(np.ascontiguousarray(poses), pipelined=True)
        assert oks and [float(v) for v in cs] == [r[1] for r in ref] and np.array_equal(gs, np.array([r[2] for r in ref]))
        o = oracle_nid(s, bins, poses[1], want_hist=False)
        parity.check_cost(ref[1][1], o["cost"])
        parity.check_grad(ref[1][2], o["grad"])
        old.close()
        new.close()
    # several pairs as ONE grid (nidreg_eval_multi): the same two launches, every pair's first workgroup publishes its own cost
    scenes = [scene_for("plumb_bob", n=n, seed=90 + k) for k, n in enumerate((50_000, 20_000, 35_000))]
    for bins in (16, 33):
        singles = [nid.NIDCost(proj, sc.image_f64, sc.points, sc.intensities, bins) for sc in scenes]
        multi = nid.MultiNIDCost(None)
        for c in singles:
            multi.add(c)
        for x in poses[:3]:
            parts = [c(x) for c in singles]
            ok, c, g = multi(x)
            tot = 0.0
            for p in parts:
                tot += p[1]
            assert ok and c == tot and np.allclose(g, np.sum([p[2] for p in parts], axis=0), rtol=1e-11, atol=1e-14), (bins, c, tot)
            okc, cc, _ = multi(x, want_grad=False)
            assert okc and cc == tot
        for c in singles:
            c.close()


def test_submit_wait_matches_synchronous_evaluation():
    """nidreg_submit / nidreg_wait (round 4): up to eight evaluations of a handle in flight, each into its own result block;
    collected in any order they equal the synchronous calls bit for bit (cost AND gradient: same kernels, same chunk table,
    same order of partial sums).  Also the pipelined batch, cost-only submissions, the NEAREST twin, and the error paths."""
    s = scene_for("plumb_bob", n=50000, seed=3)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    rng = np.random.default_rng(12)
    poses = np.ascontiguousarray([synth.random_pose_near(s.T_camera_lidar_true, rng) for _ in range(19)])
    for bins in (16, 256):
        cost = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, bins)
        ok_s, c_s, g_s = cost.eval_batch(poses)
        tickets = [cost.submit(x) for x in poses[:8]]
        with pytest.raises(RuntimeError):
            cost.submit(poses[8])  # a ninth evaluation in flight
        for k in reversed(range(8)):  # any order
            ok, c, g = cost.wait(tickets[k])
            assert ok and c == c_s[k] and np.array_equal(g, g_s[k])
        with pytest.raises(RuntimeError):
            cost.wait(tickets[3])  # collected already
        # synchronous and asynchronous calls interleaved; cost-only submissions
        t0 = cost.submit(poses[9], want_grad=False)
        okm, cm, gm = cost(poses[10])
        t1 = cost.submit(poses[11])
        assert okm and cm == c_s[10] and np.array_equal(gm, g_s[10])
        ok1, c1, g1 = cost.wait(t1)
        ok0, c0, g0 = cost.wait(t0)
        assert ok0 and c0 == c_s[9] and g0 is None and ok1 and c1 == c_s[11] and np.array_equal(g1, g_s[11])
        ok_p, c_p, g_p = cost.eval_batch(poses, pipelined=True)
        assert ok_p == ok_s and np.array_equal(c_p, c_s) and np.array_equal(g_p, g_s)
        ok_q, c_q, g_q = cost.eval_batch(poses, want_grad=False, pipelined=True)
        assert ok_q and np.array_equal(c_q, c_s) and g_q is None
        # the histograms afterwards are those of the last evaluation queued
        fx = cost.histogram_fixed()
        cost(poses[-1])
        assert np.array_equal(fx[0], cost.histogram_fixed()[0])
        cost.close()
    max_fov = oracle_lib.estimate_camera_fov(s.model, s.intrinsics, s.distortion, s.width, s.height)
    calc = nid.CostCalculatorNID(proj, s.image_u8, s.points, s.intensities, nid.NIDCostParams(256), max_fov=max_fov)
    mats = [se3.to_matrix(x) for x in poses[:7]]  # Nelder-Mead's initial simplex: 7 vertices (nelder_mead.hpp:32-57)
    sync = [calc.calculate(T) for T in mats]
    tickets = [calc.submit(T) for T in mats]
    assert [calc.wait(t) for t in tickets] == sync
    calc.close()
    # a handle spread over several (here: co-located) shards evaluates inside submit; the ticket carries the results
    sharded = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 256, devices=[0, 0])
    plain = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 256)
    t = sharded.submit(poses[0])
    oks, cs, gs = sharded.wait(t)
    okp, cp, gp = plain(poses[0])
    assert oks and okp and cs == cp and np.allclose(gs, gp, rtol=1e-11, atol=1e-14)
    # eight tickets outstanding and the pipelined batch on handles whose submit evaluates synchronously (a sharded handle bumps
    # its leader's sequence number itself, a timing handle is evaluated in place): tickets come from a counter of their own, so
    # the ring of eight holds eight (they ran 1, 3, 5, ... and collided at the fifth)
    ok_s, c_s, g_s = plain.eval_batch(poses)
    timed = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 256)
    timed.set_timing(True)
    for hnd, exact in ((sharded, False), (timed, True)):
        tickets = [hnd.submit(x) for x in poses[:8]]
        with pytest.raises(RuntimeError):
            hnd.submit(poses[8])
        for k in reversed(range(8)):
            ok, c, g = hnd.wait(tickets[k])
            assert ok and c == c_s[k]
            assert np.array_equal(g, g_s[k]) if exact else np.allclose(g, g_s[k], rtol=1e-11, atol=1e-14)
        ok_p, c_p, g_p = hnd.eval_batch(poses, pipelined=True)
        assert ok_p == ok_s and np.array_equal(c_p, c_s)
        assert np.array_equal(g_p, g_s) if exact else np.allclose(g_p, g_s, rtol=1e-11, atol=1e-14)
    timed.close()
    sharded.close()
    plain.close()


@pytest.mark.parametrize("pose", ["identity", "init"])
def test_nearest_fast_tier_decides_like_the_reference_around_every_boundary(pose):
    """k_nearest_hist's fast decision tier (round 4; plumb_bob, fp64): zn, u, v by fused multiply-adds and one-Newton-step
    reciprocals, kept only where every decision -- inside the FoV cone, inside the image, which pixel -- lies outside a proven
    error band; lanes inside the band repeat the point in the reference's exact expression order.  Points placed 0 ... 1e-8 px
    around pixel boundaries and the image border, and 0 ... 1e-8 rad around the FoV cone (a cone that cuts through the image),
    with lens distortion and a general pose: the integer histogram must equal the oracle's bit for bit, as must the histogram
    of a handle with the tier switched off."""
    s = scene_for("plumb_bob", n=2000)
    W, H = s.width, s.height
    intr, dist = list(s.intrinsics), list(s.distortion)
    fx, fy, cx, cy = intr[:4]
    x = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]) if pose == "identity" else s.T_camera_lidar_init
    T = se3.to_matrix(x)
    R, t = T[:3, :3], T[:3, 3]
    rng = np.random.default_rng(99)
    deltas = np.array([0.0, 1e-13, -1e-13, 1e-12, -1e-12, 1e-11, -1e-11, 1e-10, -1e-10, 1e-9, -1e-9, 1e-8, -1e-8])
    n = 12000
    u = rng.integers(0, W, n).astype(np.float64) + deltas[rng.integers(0, len(deltas), n)]
    v = rng.integers(0, H, n).astype(np.float64) + deltas[rng.integers(0, len(deltas), n)]
    half = rng.random(n) < 0.5  # half of them near a boundary in one coordinate only
    u = np.where(half & (rng.random(n) < 0.5), rng.uniform(0, W, n), u)
    v = np.where(half & (rng.random(n) < 0.5), rng.uniform(0, H, n), v)
    nb = 1500  # the image border: trunc(u) in [0, W)  <=>  -1 < u < W
    ub = np.where(rng.random(nb) < 0.5, -1.0, float(W)) + deltas[rng.integers(0, len(deltas), nb)]
    vb = np.where(rng.random(nb) < 0.5, -1.0, float(H)) + deltas[rng.integers(0, len(deltas), nb)]
    u = np.concatenate([u, ub, rng.uniform(0, W, nb)])
    v = np.concatenate([v, rng.uniform(0, H, nb), vb])
    z = rng.uniform(1.5, 25.0, u.shape[0])
    pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)
    for _ in range(8):  # Newton on (x, y) at fixed depth, with the oracle's own projection and Jacobian
        uv, J = oracle_lib.project_jacobian("plumb_bob", intr, dist, pc)
        r = np.stack([u, v], -1) - uv
        J2 = J.reshape(-1, 2, 3)[:, :, :2]
        pc[:, :2] += np.linalg.solve(J2, r[:, :, None])[:, :, 0]
    max_fov = 0.55  # radians: a cone through the image (the corners of this camera sit at ~0.74)
    nf = 3000
    dth = np.array([0.0, 1e-15, -1e-15, 1e-14, -1e-14, 1e-13, -1e-13, 1e-12, -1e-12, 1e-10, -1e-10, 1e-8, -1e-8])
    th = max_fov + dth[rng.integers(0, len(dth), nf)]
    ph = rng.uniform(0, 2 * np.pi, nf)
    rr = rng.uniform(1.5, 25.0, nf)
    cone = np.stack([rr * np.sin(th) * np.cos(ph), rr * np.sin(th) * np.sin(ph), rr * np.cos(th)], -1)
    pc = np.concatenate([pc, cone, np.zeros((3, 3))])  # and points at the camera centre (|p_cam| = 0)
    pl = (pc - t) @ R  # R^T (p_cam - t)
    pts = np.concatenate([pl, np.ones((pl.shape[0], 1))], -1)
    ints = (np.floor(rng.random(pts.shape[0]) * 256) / 256).astype(np.float64)
    proj = nid.create_camera("plumb_bob", intr, dist)
    for bins in (256, 16):
        ref_cost, ref_hist = oracle_lib.cost_calculator_nid("plumb_bob", intr, dist, s.image_u8, pts, ints, bins, max_fov, T, want_hist=True)
        calc = nid.CostCalculatorNID(proj, s.image_u8, pts, ints, nid.NIDCostParams(bins), max_fov=max_fov)
        assert calc.info()["nearest_fast"] == 1 and calc.info()["float32_records"] == 0
        c = calc.calculate(T)
        fx_, inl, frac = calc.histogram_fixed()
        assert np.array_equal(fx_, ref_hist) and inl == ref_hist.sum()
        assert abs(c - ref_cost) <= 1e-12
        assert 0.2 * pts.shape[0] < inl < 0.95 * pts.shape[0]  # the cone and the border really cut the set
        calc.close()
    # float records (what PLY data gives): the placement is lost to the float rounding, the decisions must still agree
    pts32 = pts.astype(np.float32).astype(np.float64)
    ref_cost, ref_hist = oracle_lib.cost_calculator_nid("plumb_bob", intr, dist, s.image_u8, pts32, ints, 256, max_fov, T, want_hist=True)
    calc = nid.CostCalculatorNID(proj, s.image_u8, pts32, ints, nid.NIDCostParams(256), max_fov=max_fov)
    assert calc.info()["float32_records"] == 1
    calc.calculate(T)
    assert np.array_equal(calc.histogram_fixed()[0], ref_hist)
    calc.close()
    # a cone close to 90 degrees (tan(max_fov) unbounded), a model without a band (atan): no fast tier
    wide = nid.CostCalculatorNID(proj, s.image_u8, pts32, ints, nid.NIDCostParams(256), max_fov=1.5)
    assert wide.info()["nearest_fast"] == 0
    wide.close()
    sa = scene_for("atan", n=2000)
    other = nid.CostCalculatorNID(nid.create_camera(sa.model, sa.intrinsics, sa.distortion), sa.image_u8, sa.points, sa.intensities, nid.NIDCostParams(256), max_fov=0.7)
    assert other.info()["nearest_fast"] == 0
    other.close()


def _wide_angle_boundary_points(model, pose):
    s = scene_for(model, n=2000)
    W, H = s.width, s.height
    intr, dist = list(s.intrinsics), list(s.distortion)
    x = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]) if pose == "identity" else s.T_camera_lidar_init
    T = se3.to_matrix(x)
    R, t = T[:3, :3], T[:3, 3]
    rng = np.random.default_rng(77)
    deltas = np.array([0.0, 1e-13, -1e-13, 1e-12, -1e-12, 1e-11, -1e-11, 1e-10, -1e-10, 1e-9, -1e-9, 1e-8, -1e-8])
    n = 10000
    u = rng.integers(0, W, n).astype(np.float64) + deltas[rng.integers(0, len(deltas), n)]
    v = rng.integers(0, H, n).astype(np.float64) + deltas[rng.integers(0, len(deltas), n)]
    half = rng.random(n) < 0.5
    u = np.where(half & (rng.random(n) < 0.5), rng.uniform(0, W, n), u)
    v = np.where(half & (rng.random(n) < 0.5), rng.uniform(0, H, n), v)
    nb = 1500  # the image border: trunc(u) in [0, W)  <=>  -1 < u < W
    ub = np.where(rng.random(nb) < 0.5, -1.0, float(W)) + deltas[rng.integers(0, len(deltas), nb)]
    vb = np.where(rng.random(nb) < 0.5, -1.0, float(H)) + deltas[rng.integers(0, len(deltas), nb)]
    u = np.concatenate([u, ub, rng.uniform(0, W, nb)])
    v = np.concatenate([v, rng.uniform(0, H, nb), vb])
    dist_m = rng.uniform(1.5, 25.0, u.shape[0])
    if model == "equirectangular":
        lon = (u / W - 0.5) * 2.0 * np.pi
        lat = -(v / H - 0.5) * np.pi
        pc = dist_m[:, None] * np.stack([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)], -1)
    else:
        fx, fy, cx, cy = intr[:4]
        # a bearing near the target through the ideal (undistorted) model, then Newton on (x, y) at fixed z with the oracle's own
        # projection and Jacobian
        mx, my = (u - cx) / fx, (v - cy) / fy
        rad = np.hypot(mx, my)
        theta = rad if model == "fisheye" else 2.0 * np.arctan(rad)  # omnidir with xi = 1: |m| = tan(theta / 2)
        theta = np.minimum(theta, 1.45 if model == "fisheye" else 2.6)
        k = np.where(rad > 0, np.tan(np.minimum(theta, 1.5)) / np.maximum(rad, 1e-300), 1.0)
        pc = np.stack([mx * k, my * k, np.ones_like(mx)], -1) * dist_m[:, None] / np.sqrt((mx * k) ** 2 + (my * k) ** 2 + 1.0)[:, None]
        for _ in range(12):
            uv, J = oracle_lib.project_jacobian(model, intr, dist, pc)
            r = np.stack([u, v], -1) - uv
            J2 = J.reshape(-1, 2, 3)[:, :, :2]
            ok = np.isfinite(J2).all(axis=(1, 2)) & np.isfinite(r).all(axis=1) & (np.abs(np.linalg.det(np.where(np.isfinite(J2), J2, 1.0))) > 1e-9)
            step = np.zeros_like(r)
            step[ok] = np.linalg.solve(J2[ok], r[ok][:, :, None])[:, :, 0]
            pc[:, :2] += np.clip(step, -0.5 * dist_m[:, None], 0.5 * dist_m[:, None])
    max_fov = {"fisheye": 0.9, "omnidir": 1.2, "equirectangular": 2.0}[model]  # cones that cut through the image
    nf = 3000
    dth = np.array([0.0, 1e-15, -1e-15, 1e-14, -1e-14, 1e-13, -1e-13, 1e-12, -1e-12, 1e-10, -1e-10, 1e-8, -1e-8])
    th = max_fov + dth[rng.integers(0, len(dth), nf)]
    ph = rng.uniform(0, 2 * np.pi, nf)
    rr = rng.uniform(1.5, 25.0, nf)
    cone = np.stack([rr * np.sin(th) * np.cos(ph), rr * np.sin(th) * np.sin(ph), rr * np.cos(th)], -1)
    tiny = np.array([0.0, 1e-300, -1e-300, 1e-17, -1e-17, 1e-13, -1e-13, 1e-9, -1e-9, 1e-6, -1e-6])
    ns = 600
    a, b = tiny[rng.integers(0, len(tiny), ns)], tiny[rng.integers(0, len(tiny), ns)]
    d = rng.uniform(0.5, 20.0, ns)
    special = [
        np.stack([a, b, d], -1), np.stack([a, b, -d], -1),        # the optical axis, in front of and behind the camera
        np.stack([a, d, b], -1), np.stack([a, -d, b], -1),        # the poles / the vertical axis of the equirectangular model
        np.stack([a, rng.uniform(-3, 3, ns), -d], -1),           # the +-pi seam of the longitude
        np.stack([d, rng.uniform(-3, 3, ns), a], -1), np.stack([-d, rng.uniform(-3, 3, ns), a], -1),  # z = +-0: the 90-degree plane
        -pc[:ns],                                                 # mirror images behind the camera
        np.zeros((3, 3)),                                         # |p_cam| = 0
    ]
    # the centre rule of the equirectangular model: |p|^2 on both sides of 1e-3
    dirs = rng.normal(size=(ns, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    special.append(dirs * np.sqrt(1e-3 * (1.0 + tiny[rng.integers(0, len(tiny), ns)] * 1e3))[:, None])
    pc = np.concatenate([pc, cone] + special)
    pl = (pc - t) @ R  # R^T (p_cam - t)
    pts = np.concatenate([pl, np.ones((pl.shape[0], 1))], -1)
    ints = (np.floor(rng.random(pts.shape[0]) * 256) / 256).astype(np.float64)
    return s, W, H, intr, dist, T, pts, ints, max_fov


@pytest.mark.parametrize("pose", ["identity", "general"])
@pytest.mark.parametrize("model", ["fisheye", "omnidir", "equirectangular"])
def test_nearest_fast_tier_of_the_wide_angle_models_decides_like_the_reference(model, pose):
    """Round 5: k_nearest_hist's fast decision tier for fisheye / omnidir / equirectangular -- the SPLINE kernels' cores (table
    atan2, one-Newton-step rsqrt / reciprocal) plus a per-point band from each model's own chain rule; lanes inside a band repeat
    the point in the reference's exact expression order (libm asin / atan2 included).  Points placed 0 ... 1e-8 px around pixel
    boundaries and the image border, 0 ... 1e-8 rad around the FoV cone, and at each model's own singular places -- the optical
    axis and points behind the camera (fisheye: abs(z), fisheye.hpp:16; 0 / 0 at r = 0), |p| = 0 (omnidir.hpp:19), the poles, the
    vertical axis, the +-pi seam and the |p|^2 < 1e-3 centre rule (equirectangular.hpp:16-28): the integer histogram must be
    the oracle's bit for bit, with and without the tier."""
    s, W, H, intr, dist, T, pts, ints, max_fov = _wide_angle_boundary_points(model, pose)
    proj = nid.create_camera(model, intr, dist)
    full_fov = oracle_lib.estimate_camera_fov(model, intr, dist, W, H)
    # Against the CPU the exact tier of a model with a transcendental function in it (fisheye: atan2; equirectangular: asin,
    # atan2) can only be as exact as the two libms agree: ROCm's and glibc's differ in the last place now and then, i.e. by
    # ~3e-14 px here, and a point placed closer than that to a pixel boundary may land on the other side (22-264 of these 21 403
    # adversarial points, none of 10^7 points of a real cloud: test_config_cameras_full_size_match_oracle).  So: (1) fast tier
    # against exact tier on ALL points, same GPU, same libm -- the statement the bands make; (2) against the oracle on the points
    # that are not within 1e-11 px of a pixel boundary (omnidir has no such function: all of them).
    pc = pts[:, :3] @ T[:3, :3].T + T[:3, 3]
    uv = oracle_lib.project(model, intr, dist, pc)
    with np.errstate(invalid="ignore"):
        near = (np.abs(uv[:, 0] - np.rint(uv[:, 0])) < 1e-11) | (np.abs(uv[:, 1] - np.rint(uv[:, 1])) < 1e-11)
    soft = np.ones(pts.shape[0], dtype=bool) if model == "omnidir" else ~near
    assert soft.sum() > 0.4 * pts.shape[0]
    for fov in (max_fov, full_fov):
        for bins in (256, 16):
            fast = nid.CostCalculatorNID(proj, s.image_u8, pts, ints, nid.NIDCostParams(bins), max_fov=fov)
            exact = nid.CostCalculatorNID(proj, s.image_u8, pts, ints, nid.NIDCostParams(bins), max_fov=fov, flags=_lib.FLAG_NEAREST_EXACT)
            assert fast.info()["nearest_fast"] == 1 and exact.info()["nearest_fast"] == 0 and fast.info()["float32_records"] == 0
            cf, ce = fast.calculate(T), exact.calculate(T)
            hf, inl, frac = fast.histogram_fixed()
            he = exact.histogram_fixed()[0]
            assert np.array_equal(hf, he) and cf == ce, (model, pose, fov, bins, int(np.abs(hf - he).sum()))
            assert 0.1 * pts.shape[0] < inl < 0.97 * pts.shape[0]
            fast.close()
            exact.close()
            ref_cost, ref_hist = oracle_lib.cost_calculator_nid(model, intr, dist, s.image_u8, pts[soft], ints[soft], bins, fov, T, want_hist=True)
            calc = nid.CostCalculatorNID(proj, s.image_u8, pts[soft], ints[soft], nid.NIDCostParams(bins), max_fov=fov)
            c = calc.calculate(T)
            fx_, inl, frac = calc.histogram_fixed()
            assert frac == 0 and np.array_equal(fx_, ref_hist) and inl == ref_hist.sum(), (model, pose, fov, bins, int(np.abs(fx_ - ref_hist).sum()))
            assert abs(c - ref_cost) <= 1e-12
            calc.close()
    pts32 = pts.astype(np.float32).astype(np.float64)  # float records (what PLY data gives): the placement is lost to the rounding
    ref_cost, ref_hist = oracle_lib.cost_calculator_nid(model, intr, dist, s.image_u8, pts32, ints, 256, full_fov, T, want_hist=True)
    calc = nid.CostCalculatorNID(proj, s.image_u8, pts32, ints, nid.NIDCostParams(256), max_fov=full_fov)
    assert calc.info()["float32_records"] == 1 and calc.info()["nearest_fast"] == 1
    calc.calculate(T)
    assert np.array_equal(calc.histogram_fixed()[0], ref_hist)
    calc.close()


def test_cohort_gives_concurrent_callers_one_round_of_workgroups(monkeypatch):
    """NIDREG_COHORT=1 (round 4): handles created one after the other for one MultiNIDCost -- compatible, before any of them is
    evaluated -- get chunk tables that are their SHARE of one round of workgroups, so that the reference's unchanged OpenMP loop
    over pairs (one caller per pair, visual_camera_calibration.cpp:161) fills the GPU once instead of k times.  The tables are a
    function of the cohort, never of timing: every member's results are the same bits whether the members are evaluated one
    by one, from concurrent threads, or in any order; cost and histogram equal those of a handle outside any cohort bit for
    bit, the gradient to rounding."""
    import threading

    sizes = [30000, 12000, 7000, 21000]
    scenes = [scene_for("plumb_bob", n=n, seed=170 + k) for k, n in enumerate(sizes)]
    proj = nid.create_camera(scenes[0].model, scenes[0].intrinsics, scenes[0].distortion)
    solo = [nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 256) for s in scenes]  # no cohort
    rng = np.random.default_rng(4)
    poses = [scenes[0].T_camera_lidar_init] + [synth.random_pose_near(scenes[0].T_camera_lidar_true, rng) for _ in range(5)]
    ref = [[c(x) for c in solo] for x in poses]
    monkeypatch.setenv("NIDREG_COHORT", "1")
    runs = []
    for mode in ("serial", "threads", "reverse"):
        members = [nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 256) for s in scenes]
        full = [m.info()["num_chunks"] for m in members]  # (still every member's own full round: nothing has been evaluated)
        other = nid.NIDCost(proj, scenes[0].image_f64, scenes[0].points, scenes[0].intensities, 16)  # another bin count: not of this cohort (and it ends it)
        out = [[None] * len(members) for _ in poses]
        if mode == "threads":
            bar = threading.Barrier(len(members))

            def work(i):
                for j, x in enumerate(poses):
                    bar.wait()
                    out[j][i] = members[i](x)

            th = [threading.Thread(target=work, args=(i,)) for i in range(len(members))]
            for t in th:
                t.start()
            for t in th:
                t.join()
        else:
            order = range(len(members)) if mode == "serial" else reversed(range(len(members)))
            for i in order:
                for j, x in enumerate(poses):
                    out[j][i] = members[i](x)
        share = [m.info()["num_chunks"] for m in members]
        assert sum(share) <= 4 * 256 + len(members) and all(a < b for a, b in zip(share, full)), (share, full)  # together: one round of 4 workgroups per CU
        assert other.info()["num_chunks"] >= 1 and other(poses[0])[0]
        for j in range(len(poses)):
            for i in range(len(members)):
                ok, c, g = out[j][i]
                rok, rc, rg = ref[j][i]
                assert ok and rok and c == rc and np.allclose(g, rg, rtol=1e-11, atol=1e-14)
        for i, m in enumerate(members):
            m(poses[-1])
            solo[i](poses[-1])
            assert np.array_equal(m.histogram_fixed()[0], solo[i].histogram_fixed()[0])
        runs.append(out)
        for m in members + [other]:
            m.close()
    for j in range(len(poses)):  # run-to-run, order-to-order, threads or not: the same bits (gradient included)
        for i in range(len(sizes)):
            assert runs[0][j][i][1] == runs[1][j][i][1] == runs[2][j][i][1]
            assert np.array_equal(runs[0][j][i][2], runs[1][j][i][2]) and np.array_equal(runs[0][j][i][2], runs[2][j][i][2])
    # the single grid of nidreg_eval_multi over a cohort still agrees
    members = [nid.NIDCost(proj, s.image_f64, s.points, s.intensities, 256) for s in scenes]
    multi = nid.MultiNIDCost(None)
    for m in members:
        multi.add(m)
    ok, c, g = multi(poses[1])
    assert ok and c == sum(r[1] for r in ref[1]) and np.allclose(g, sum(r[2] for r in ref[1]), rtol=1e-11, atol=1e-14)
    for m in members + solo:
        m.close()


@pytest.mark.parametrize("model", list(CAMERAS))
def test_fused_single_launch_has_the_bits_of_the_three_kernel_route(model, monkeypatch):
    """Small tables (bins <= 32), a cloud that fits on chip, an evaluation that has the device to itself: ONE launch (csrc/nid_fused.hpp:
    pass A stashes what it knows about its points in LDS, grid barrier, entropy tail, pass B from the stash).  It runs over the handle's
    own chunk table with k_spline_grad's thread <-> point mapping and reductions, so cost AND gradient are the same bits as the
    three-kernel route's (NIDREG_FUSED=0) -- for both stash formats, with outliers, when cost-only evaluations alternate with it on the
    double-buffered histogram -- and both match the oracle."""
    s = scene_for(model, n=40_000, seed=31)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    rng = np.random.default_rng(5)
    far = se3.plus(s.T_camera_lidar_true, np.array([0.4, -0.3, 0.2, 0.08, -0.05, 0.1]))  # a third of the cloud leaves the image
    poses = [s.T_camera_lidar_init, far] + [synth.random_pose_near(s.T_camera_lidar_true, rng) for _ in range(4)]
    for bins, tuning in ((16, {}), (2, {}), (7, {}), (32, {}), (16, {"target_blocks": 3}), (16, {"columns_per_group": 4})):
        monkeypatch.setenv("NIDREG_FUSED", "0")
        plain = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, bins, **tuning)
        ref = [plain(x) for x in poses]
        assert plain.info()["fused"] == 0
        monkeypatch.delenv("NIDREG_FUSED")
        for stash in ("full", "uv"):
            monkeypatch.setenv("NIDREG_FUSED_STASH", stash)
            fused = nid.NIDCost(proj, s.image_f64, s.points, s.intensities, bins, **tuning)
            got = []
            for j, x in enumerate(poses):
                if j % 2:
                    okc, cc, _ = fused(x, want_grad=False)  # (three kernels: k_entropy with its tail) between two fused launches
                    assert okc == ref[j][0] and cc == ref[j][1]
                got.append(fused(x))
            info = fused.info()
            if tuning.get("target_blocks") == 3:  # 13 333 points per chunk: beyond either stash format -- three kernels, as before
                assert info["fused"] == 0, info
            else:
                assert info["fused"] == 1 and info["fused_full_stash"] == (1 if stash == "full" else 0) and info["fused_chunks"] == info["num_chunks"], (bins, tuning, stash, info)
            for j, (a, b) in enumerate(zip(got, ref)):
                assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]), (model, bins, tuning, stash, j, a, b)
            for a, b in zip(fused.histograms(), plain.histograms()):
                assert np.array_equal(a, b)
            fused.close()
        monkeypatch.delenv("NIDREG_FUSED_STASH")
        o = oracle_nid(s, bins, poses[1])
        parity.check_cost(ref[1][1], o["cost"])
        parity.check_grad(ref[1][2], o["grad"])
        plain.close()


def test_fused_single_launch_other_shapes_and_its_fallback(monkeypatch):
    """(a) records that do not round-trip through float (Rec64 stash); (b) a cloud whose chunks only fit the (u, v) stash with two
    workgroups per CU; (c) a cloud beyond the stash: three kernels as before; (d) a grid barrier that times out (test hook): the
    kernel ends without its tag, the evaluation is repeated on the three-kernel route -- same results -- and the handle stops using the
    fused route; (e) eight evaluations through submit / wait (never fused) give the synchronous (fused) route's bits."""
    proj_of = lambda sc: nid.create_camera(sc.model, sc.intrinsics, sc.distortion)
    rng = np.random.default_rng(6)

    def both(sc, pts, bins, expect_fused, expect_full=None):
        poses = [sc.T_camera_lidar_init] + [synth.random_pose_near(sc.T_camera_lidar_true, rng) for _ in range(3)]
        monkeypatch.setenv("NIDREG_FUSED", "0")
        plain = nid.NIDCost(proj_of(sc), sc.image_f64, pts, sc.intensities, bins)
        ref = [plain(x) for x in poses]
        monkeypatch.delenv("NIDREG_FUSED")
        fused = nid.NIDCost(proj_of(sc), sc.image_f64, pts, sc.intensities, bins)
        got = [fused(x) for x in poses]
        info = fused.info()
        assert info["fused"] == expect_fused, info
        if expect_full is not None:
            assert info["fused_full_stash"] == expect_full, info
        for a, b in zip(got, ref):
            assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])
        oks, cs, gs = fused.eval_batch(np.ascontiguousarray(poses), pipelined=True)
        assert oks and [float(v) for v in cs] == [r[1] for r in ref] and np.array_equal(gs, np.array([r[2] for r in ref]))
        plain.close()
        return fused, poses, ref

    s = scene_for("plumb_bob", n=50_000, seed=32)
    pts64 = s.points.copy()
    pts64[:, :3] += 1e-9 * rng.standard_normal((pts64.shape[0], 3))  # not float32-representable: Rec64 records
    f, _, _ = both(s, pts64, 16, 1)
    assert f.info()["float32_records"] == 0
    f.close()
    big = synth.make_scene(CAMERAS["plumb_bob"], num_points=700_000, seed=33, device="cuda:0")
    f, _, _ = both(big, big.points, 16, 1, expect_full=0)
    f.close()
    huge = synth.make_scene(CAMERAS["plumb_bob"], num_points=3_000_000, seed=34, device="cuda:0")
    f, _, _ = both(huge, huge.points, 16, 0)
    f.close()
    f, _, _ = both(s, s.points, 64, 0)  # 64 bins: not a small table
    f.close()
    # (d) the barrier gives up
    monkeypatch.setenv("NIDREG_FUSED_TIMEOUT_US", "300")
    h = nid.NIDCost(proj_of(s), s.image_f64, s.points, s.intensities, 16)
    x = s.T_camera_lidar_init
    ok0, c0, g0 = h(x)
    assert h.info()["fused"] == 1
    monkeypatch.setenv("NIDREG_FUSED_TEST_HANG", "1")
    ok1, c1, g1 = h(x)
    monkeypatch.delenv("NIDREG_FUSED_TEST_HANG")
    assert ok1 == ok0 and c1 == c0 and np.array_equal(g1, g0)
    assert h.info()["fused"] == 0
    ok2, c2, g2 = h(synth.random_pose_near(s.T_camera_lidar_true, rng))
    assert ok2 and np.isfinite(c2)
    ok3, c3, g3 = h(x)
    assert c3 == c0 and np.array_equal(g3, g0)
    h.close()


# What the host dispatch can select, as (bins, tuning, planner knobs, what info() must then report).  The knobs: NIDREG_MAX_SEGS=1
# keeps every table on one column group per chunk (the straight-line kernels); eight workgroups over 256 columns with a free
# segment (NIDREG_SEG_OVERHEAD=0, no minimum gain) cannot be had without chunks across groups (the SEG kernels).
_STRAIGHT = {"NIDREG_MAX_SEGS": "1"}
_ACROSS = {"NIDREG_SEG_OVERHEAD": "0", "NIDREG_SEG_MIN_GAIN": "0"}
SPLINE_ROUTES = {
    "wide_gw1": (256, {}, _STRAIGHT, {"lds_copies": 32, "columns_per_group": 1, "segmented": 0, "segmented_hist": 0}),
    "wide_gw1_seg": (256, {"target_blocks": 8}, _ACROSS, {"lds_copies": 32, "columns_per_group": 1, "segmented": 1, "segmented_hist": 1}),
    "generic_gw1": (256, {"lds_copies": 16}, _STRAIGHT, {"lds_copies": 16, "columns_per_group": 1, "segmented": 0, "segmented_hist": 0}),
    "generic_gw1_seg": (256, {"lds_copies": 16, "target_blocks": 8}, _ACROSS, {"lds_copies": 16, "columns_per_group": 1, "segmented": 1, "segmented_hist": 0}),
    "generic_gw4": (256, {"columns_per_group": 4}, {}, {"columns_per_group": 4, "segmented": 0, "segmented_hist": 0}),
    "generic_b16": (16, {}, {"NIDREG_FUSED": "0"}, {"columns_per_group": 16, "segmented": 0, "fused": 0}),
    "fused_full": (16, {}, {"NIDREG_FUSED_STASH": "full"}, {"fused": 1, "fused_full_stash": 1}),
    "fused_uv": (16, {}, {"NIDREG_FUSED_STASH": "uv"}, {"fused": 1, "fused_full_stash": 0}),
}
NEAREST_ROUTES = {
    "straight": ({}, _STRAIGHT, {"segmented": 0}),
    "seg": ({"target_blocks": 8}, _ACROSS, {"segmented": 1}),
}
NEAREST_FAST_TIER = {"fisheye": 1, "equirectangular": 1, "atan": 0, "rational_polynomial": 0}  # (plumb_bob, omnidir: by field of view)


@pytest.mark.parametrize("rec64", [False, True], ids=["rec32", "rec64"])
@pytest.mark.parametrize("model", list(CAMERAS))
def test_every_kernel_selection_of_the_host_dispatch_matches_the_oracle(model, rec64, monkeypatch):
    """The launchers pick a kernel instantiation from (model, record type, WIDE, GW1, SEG, MULTI, fused stash); a wrong pick
    -- Rec64 read as Rec32, WIDE and SEG swapped -- compiles and is invisible to everything but a run.  Every model x record
    type goes through every selection here, on two small pairs (4096 and 3000 points: several chunks each): info() must report
    the route the case means to take, a single evaluation meets the oracle at the bars of tests/parity.py, and the two pairs
    as one grid (MULTI; never fused) give the sum of the single evaluations bit for bit (gradient: to rounding, and against the
    summed oracle).  info() describes a handle's own tables, not a group's: the group's tables are built under the same
    planner knobs (its first evaluation), which is what makes them straight or segmented, but that is not asserted."""
    scenes = [scene_for(model, n=4096, seed=41), scene_for(model, n=3000, seed=42)]
    clouds = []
    for s in scenes:
        pts = s.points.copy()
        if rec64:
            pts[:, :3] += 1e-9 * (1 + np.arange(pts.shape[0]))[:, None]  # no longer float32-exact
        clouds.append(pts)
    proj = nid.create_camera(scenes[0].model, scenes[0].intrinsics, scenes[0].distortion)
    x = scenes[0].T_camera_lidar_init
    refs = {}
    for name, (bins, tuning, env, expect) in SPLINE_ROUTES.items():
        if bins not in refs:
            refs[bins] = [oracle_lib.nid_cost(s.model, s.intrinsics, s.distortion, s.image_f64, p, s.intensities, bins, x) for s, p in zip(scenes, clouds)]
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        hs = [nid.NIDCost(proj, s.image_f64, p, s.intensities, bins, **tuning) for s, p in zip(scenes, clouds)]
        single = [h(x) for h in hs]
        for h, (ok, c, g), ref in zip(hs, single, refs[bins]):
            info = h.info()
            assert info["float32_records"] == (0 if rec64 else 1), (name, info)
            assert {k: info[k] for k in expect} == expect, (name, info)
            assert ok and ref["ok"]
            parity.check_cost(c, ref["cost"], what=name)
            parity.check_grad(g, ref["grad"], what=name)
        if not name.startswith("fused"):
            multi = nid.MultiNIDCost(None)
            for h in hs:
                multi.add(h)
            ok, c, g = multi(x)
            assert ok and c == single[0][1] + single[1][1], (name, c, single)
            assert np.allclose(g, single[0][2] + single[1][2], rtol=1e-11, atol=1e-14), name
            parity.check_grad(g, refs[bins][0]["grad"] + refs[bins][1]["grad"], what=name + " multi")
        for k in env:
            monkeypatch.delenv(k)
        for h in hs:
            h.close()
    # NEAREST: integer histogram bit for bit, single and as one grid (sum_costs)
    s0 = scenes[0]
    max_fov = oracle_lib.estimate_camera_fov(s0.model, s0.intrinsics, s0.distortion, s0.width, s0.height)
    T = se3.to_matrix(x)
    nrefs = [oracle_lib.cost_calculator_nid(s.model, s.intrinsics, s.distortion, s.image_u8, p, s.intensities, 256, max_fov, T, want_hist=True) for s, p in zip(scenes, clouds)]
    for name, (tuning, env, expect) in NEAREST_ROUTES.items():
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        calcs = [nid.CostCalculatorNID(proj, s.image_u8, p, s.intensities, nid.NIDCostParams(256), max_fov=max_fov, **tuning) for s, p in zip(scenes, clouds)]
        costs = []
        for calc, (ref_cost, ref_hist) in zip(calcs, nrefs):
            info = calc.info()
            assert info["float32_records"] == (0 if rec64 else 1), (name, info)
            assert {k: info[k] for k in expect} == expect, (name, info)
            if model in NEAREST_FAST_TIER:
                assert info["nearest_fast"] == NEAREST_FAST_TIER[model], (name, info)
            costs.append(calc.calculate(T))
            assert np.array_equal(calc.histogram_fixed()[0], ref_hist) and abs(costs[-1] - ref_cost) <= 1e-12, name
        assert nid.sum_costs(calcs, T) == costs[0] + costs[1], name
        for calc, (ref_cost, ref_hist) in zip(calcs, nrefs):
            assert np.array_equal(calc.histogram_fixed()[0], ref_hist), name
        for k in env:
            monkeypatch.delenv(k)
        for calc in calcs:
            calc.close()
