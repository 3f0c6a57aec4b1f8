"""The device record builder (csrc/nid_build.hip: k_mark_bins, k_build_keys, the trimmed radix sort, k_build_bounds, the back-fill of the empty
groups, k_build_gather) looked at directly: every record, its bin, its position, gcount and the record format, read back through the test
hook nidreg_debug_records (_lib.debug_records) and compared with tests/record_oracle.py, a restatement of the rules in Python ints.

Inputs come from tests/record_cases.py; tests/test_record_builder_host.py checks on the CPU that they meet the conditions the cases are
named after.  Every handle is built twice and the two read-backs must have the same bytes.  Every comparison here is an equality, a bar of
tests/parity.py, or isnan for NaN coordinates (record_oracle.bits maps every NaN onto one pattern)."""
import contextlib
import ctypes

import numpy as np
import pytest

import oracle_lib
import parity
import record_cases as rc
import record_oracle as ro
from direct_visual_lidar_calibration_amd import _lib, nid

pytestmark = pytest.mark.gpu

ROUTES = ("spline arrays", "spline cloud", "nearest arrays", "nearest cloud")  # NIDCost / CostCalculatorNID, from host arrays / from a nid.Cloud


def make_handle(route, pts, ints, B, cull=None, **tuning):
    s = rc.scene()
    spline = route.startswith("spline")
    image = s.levels_f64 if spline else s.levels_u8
    if route.endswith("arrays"):
        assert cull is None
        if spline:
            return nid.NIDCost(s.proj, image, pts, ints, B, **tuning)
        return nid.CostCalculatorNID(s.proj, image, pts, ints, nid.NIDCostParams(B), max_fov=rc.MAX_FOV, **tuning)
    cloud = nid.Cloud(pts, ints)
    try:
        if spline:
            return nid.NIDCost.from_cloud(s.proj, image, cloud, B, cull=cull, **tuning)
        return nid.CostCalculatorNID.from_cloud(s.proj, image, cloud, nid.NIDCostParams(B), max_fov=rc.MAX_FOV, cull=cull, **tuning)
    finally:
        cloud.close()


def record_bytes(rec):
    return rec["num_records"], rec["NG"], rec["GW"], rec["gcount"].tobytes(), rec["xyz"].tobytes(), rec["bin"].tobytes()


@contextlib.contextmanager
def built_twice(make):
    """the handle and its records; a second build of the same handle has the same bytes"""
    handles = []
    try:
        handles.append(make())
        handles.append(make())
        first, second = (_lib.debug_records(h) for h in handles)
        assert record_bytes(first) == record_bytes(second)
        assert handles[0].info()["record_bytes"] == handles[1].info()["record_bytes"]
        yield handles[0], first
    finally:
        for h in handles:
            h.close()


def rows(xyz, bins):
    return np.column_stack([ro.bits(np.asarray(xyz, dtype=np.float64).reshape(-1, 3)), np.asarray(bins, dtype=np.int64)])


def sorted_rows(a):
    return a[np.lexsort(a.T[::-1])]


def check_records(rec, pts, cols, GW, NG, order=None, what=""):
    """rec holds exactly the points pts with the columns cols: counts, gcount, every record in its group's column range, the multiset of
    (x, y, z, bin) bit for bit, and -- where the order is determined -- the stored order"""
    n = len(cols)
    assert (rec["num_records"], rec["GW"], rec["NG"]) == (n, GW, NG), (what, rec["num_records"], rec["GW"], rec["NG"])
    g = rec["gcount"]
    assert np.array_equal(g, ro.gcount(cols, GW, NG)), (what, g)
    assert g[0] == 0 and g[NG] == n and np.all(np.diff(g) >= 0), (what, g)
    group_of_record = np.searchsorted(g, np.arange(n), side="right") - 1
    assert np.array_equal(rec["bin"] // GW, group_of_record), what
    have, want = rows(rec["xyz"], rec["bin"]), rows(pts[:, :3], cols)
    assert np.array_equal(sorted_rows(have), sorted_rows(want)), what
    if order is not None:
        assert np.array_equal(have, want[order]), what


def layout_for(b, B, image_values):
    """(the column the kernels see for each point, GW, NG) with the default tuning: above 256 bins the occupied bins, compacted"""
    if B <= 256:
        cols, K = b, B
    else:
        cols, occupied = ro.compact(b)
        K = max(2, len(occupied), len(np.unique(ro.point_bins(image_values, B))))
    GW = ro.default_group_width(K)
    return cols, GW, ro.groups(K, GW)


def image_values(route):
    s = rc.scene()
    return s.levels_f64.ravel() if route.startswith("spline") else s.levels_u8.ravel() / 255.0


# ---- a: intensities on and next to the bin edges -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("B", rc.EDGE_BINS)
def test_intensities_on_and_next_to_the_bin_edges(B, route):
    """k / B and its two neighbours for every edge, +-0, subnormals, NaN, +-inf, 1e10, 2^31 / B and (2^31 - 1) / B, 1 - ulp, 1, 1.5: every
    record's bin is the rule's (the compact label at 300 bins, where the host's cast_int marks and the device's cast_int_dev reads),
    gcount is the bincount by group, hist_points is the bincount in the caller's layout and the compiled oracle's, and cost and
    gradient meet the oracle at the bars of tests/parity.py."""
    s = rc.scene()
    pts, v = rc.ladder_cloud(B)
    b = ro.point_bins(v, B)
    cols, GW, NG = layout_for(b, B, image_values(route))
    want_hp = np.bincount(b, minlength=B)
    with built_twice(lambda: make_handle(route, pts, v, B)) as (h, rec):
        check_records(rec, pts, cols, GW, NG, what=(B, route))
        assert h.info()["record_bytes"] == 16
        if route.startswith("spline"):
            ref = rc.cached(("ladder spline", B), lambda: s.o_spline(s.levels_f64, B, pts=pts, ints=v))
            ok, c, g = h(rc.IDENTITY)
            joint, hi, hp = h.histograms()
            assert ok and ref["ok"]
            assert np.array_equal(hp, want_hp) and np.array_equal(hp, ref["hist_points"]), (B, route)
            parity.check_hist(joint, ref["hist"], what=(B, route))
            parity.check_hist(hi, ref["hist_image"], kind="hist_image", what=(B, route))
            parity.check_cost(c, ref["cost"], what=(B, route))
            parity.check_grad(g, ref["grad"], what=(B, route))
        else:
            ref_cost, ref_hist = rc.cached(("ladder nearest", B), lambda: oracle_lib.cost_calculator_nid(s.model, s.intr, s.dist, s.levels_u8, pts, v, B, rc.MAX_FOV, rc.T_IDENTITY, want_hist=True))
            c = h.calculate(rc.T_IDENTITY)
            fx, inl, frac = h.histogram_fixed()
            assert frac == 0 and inl == len(v) and np.array_equal(fx, ref_hist), (B, route)
            assert np.array_equal(fx.sum(axis=0), want_hp), (B, route)
            parity.check_cost(c, ref_cost, what=(B, route))


# ---- b: more than 256 bins -----------------------------------------------------------------------------------------------------------------


def test_wide_bins_marked_on_the_device_and_on_the_host_give_the_same_records():
    """bins = 4096 with exactly 256 occupied intensity bins, bin 0 reached only through NaN and bin 4095 only through 1.5: k_mark_bins (a
    nid.Cloud) and the host loop of resolve_wide_bins (arrays) mark the same bins, and k_build_keys / k_build_gather read the table they
    built the same way -- every record carries the compact label of its bin."""
    v = rc.wide_intensities(256)
    pts = rc.pool_points(len(v))
    b = ro.point_bins(v, rc.WIDE)
    seen = {}
    for route in ROUTES:
        cols, GW, NG = layout_for(b, rc.WIDE, image_values(route))
        assert (GW, NG) == (1, 256)
        with built_twice(lambda: make_handle(route, pts, v, rc.WIDE)) as (h, rec):
            check_records(rec, pts, cols, GW, NG, what=route)
            seen[route] = record_bytes(rec)
            if route == "spline cloud":  # hist_points in the caller's 4096-bin layout (the joint histogram would be 128 MB: not fetched)
                assert h(rc.IDENTITY, want_grad=False)[0]
                hp = np.empty(rc.WIDE)
                assert _lib.load().nidreg_get_hist(h.h, None, None, hp.ctypes.data_as(_lib.c_double_p)) == _lib.NIDREG_OK
                assert np.array_equal(hp, np.bincount(b, minlength=rc.WIDE))
    assert seen["spline arrays"] == seen["spline cloud"] and seen["nearest arrays"] == seen["nearest cloud"]


@pytest.mark.parametrize("route", ROUTES)
def test_257_occupied_intensity_bins_are_refused(route):
    v = rc.wide_intensities(257)
    with pytest.raises(RuntimeError, match=r"bins = 4096 with \d+ occupied image bins and 257 occupied intensity bins: more than 256 bins per axis are supported only while at most 256 of them are occupied .* refused, not truncated"):
        make_handle(route, rc.pool_points(len(v)), v, rc.WIDE).close()


# ---- c: group bounds -----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("config", rc.GROUP_CONFIGS, ids=str)
def test_group_bounds_with_empty_groups(config):
    """k_build_bounds and the back-fill of first[]: all points in one column, only the first / only the last group occupied, the first group
    empty, alternate groups empty -- with columns_per_group that does and does not divide the bin count"""
    B, cpg = config
    GW, NG = rc.group_layout(B, cpg)
    tuning = {"columns_per_group": cpg} if cpg else {}
    for name, cols in rc.group_patterns(B, GW, NG).items():
        pts, v = rc.pool_points(len(cols)), rc.columns_to_intensities(cols, B)
        for route in ("spline arrays", "nearest cloud"):
            with built_twice(lambda: make_handle(route, pts, v, B, **tuning)) as (h, rec):
                check_records(rec, pts, cols, GW, NG, what=(config, name, route))


@pytest.mark.parametrize("config", rc.GROUP_CONFIGS, ids=str)
def test_group_bounds_at_cloud_sizes_around_one_block(config):
    B, cpg = config
    GW, NG = rc.group_layout(B, cpg)
    tuning = {"columns_per_group": cpg} if cpg else {}
    for n in rc.GROUP_SIZES:
        cols = rc.random_columns(B, n, seed=n)
        pts, v = rc.pool_points(n), rc.columns_to_intensities(cols, B)
        for route in ("spline arrays", "spline cloud", "nearest arrays"):
            with built_twice(lambda: make_handle(route, pts, v, B, **tuning)) as (h, rec):
                check_records(rec, pts, cols, GW, NG, what=(config, n, route))
                assert h.num_points == n


# ---- d: record identity and order ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("config", rc.GROUP_CONFIGS, ids=str)
def test_input_order_flag_keeps_the_callers_order_inside_every_group(config):
    B, cpg = config
    GW, NG = rc.group_layout(B, cpg)
    tuning = {"columns_per_group": cpg} if cpg else {}
    cols = rc.random_columns(B, 1025, seed=7)
    pts, v = rc.pool_points(1025, start=512), rc.columns_to_intensities(cols, B)
    order = ro.record_order(pts, cols, GW, True)
    for route in ("spline arrays", "spline cloud"):
        with built_twice(lambda: make_handle(route, pts, v, B, flags=_lib.FLAG_INPUT_ORDER, **tuning)) as (h, rec):
            check_records(rec, pts, cols, GW, NG, order=order, what=(config, route))


@pytest.mark.parametrize("config", [(16, 16), (16, 3), (256, 0)], ids=str)
def test_records_follow_group_column_morton_code_and_input_index(config):
    """Bearings at the centres of Morton cells (the device's atan2 rounding cannot move them), several points per (cell, column): the key's
    group, column and Morton fields, the bit interleaving, and the stability of the sort."""
    B, cpg = config
    GW, NG = rc.group_layout(B, cpg)
    tuning = {"columns_per_group": cpg} if cpg else {}
    pts, cols, _ = rc.lattice(B)
    v = rc.columns_to_intensities(cols, B)
    order = ro.record_order(pts, cols, GW, False)
    for route in ("spline arrays", "spline cloud"):
        with built_twice(lambda: make_handle(route, pts, v, B, **tuning)) as (h, rec):
            check_records(rec, pts, cols, GW, NG, order=order, what=(config, route))


# ---- e: the cull ---------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("B", [16, 256])  # one column group and 256: the smallest and the largest trimmed sort range
@pytest.mark.parametrize("case", ["nothing removed", "first removed", "last removed", "everything removed", "every seventh removed", "occluded points removed"])
def test_culled_points_leave_exactly_the_kept_ones_grouped(case, B):
    """from_cloud(cull=...): the records are pts[idx] grouped, idx from the oracle's ViewCulling -- a removed point's all-ones key sorts last
    and is cut off, in input order (index keys) and in Morton order"""
    s = rc.scene()
    GW, NG = rc.group_layout(B, 0)
    assert NG == (1 if B == 16 else 256)
    pts, depth = rc.cull_cases()[case]
    cols = rc.random_columns(B, len(pts), seed=3)
    v = rc.columns_to_intensities(cols, B)
    idx = oracle_lib.view_culling(s.model, s.intr, s.dist, rc.W, rc.H, pts, rc.T_IDENTITY, depth, min_z=rc.MIN_Z)
    kept_pts, kept_cols = pts[idx], cols[idx]
    cull = (rc.T_IDENTITY, rc.MIN_Z, depth)
    for flags, order in ((_lib.FLAG_INPUT_ORDER, ro.record_order(kept_pts, kept_cols, GW, True)), (0, None)):
        with built_twice(lambda: make_handle("spline cloud", pts, v, B, cull=cull, flags=flags)) as (h, rec):
            check_records(rec, kept_pts, kept_cols, GW, NG, order=order, what=(case, B, flags))
            assert h.num_points == len(idx) == h.info()["num_points"]
            if len(idx) == 0:
                assert rec["num_records"] == 0 and not rec["gcount"].any() and rec["xyz"].shape == (0, 3)
                assert not h(rc.IDENTITY)[0]


# ---- f: the record format ------------------------------------------------------------------------------------------------------------------

BF = 16  # bins of the format tests: one column group, so that under NIDREG_FLAG_INPUT_ORDER the records are the cloud in its own order


def format_cloud(n):
    pts, planted = rc.float32_cloud(n)
    cols = rc.random_columns(BF, n, seed=11)
    return pts, cols, rc.columns_to_intensities(cols, BF)


@pytest.mark.parametrize("n", rc.FORMAT_SIZES)
def test_float32_values_get_float32_records(n):
    """-0.0, FLT_MAX, +-inf, NaN and the smallest normal float are float32 values: 16-byte records, every coordinate stored bit for bit.
    Points with a non-finite coordinate are outliers: hist_points is the oracle's over the finite ones."""
    s = rc.scene()
    pts, cols, v = format_cloud(n)
    finite = np.isfinite(pts[:, :3]).all(axis=1)
    ref = s.o_spline(s.levels_f64, BF, pts=pts[finite], ints=v[finite], want_grad=False)
    for route in ("spline arrays", "spline cloud"):
        with built_twice(lambda: make_handle(route, pts, v, BF, flags=_lib.FLAG_INPUT_ORDER)) as (h, rec):
            assert h.info()["record_bytes"] == 16, route
            check_records(rec, pts, cols, BF, 1, order=np.arange(n), what=(n, route))
            assert h(rc.IDENTITY, want_grad=False)[0]
            assert np.array_equal(h.histograms()[2], ref["hist_points"]), route


@pytest.mark.parametrize("name", list(rc.NOT_FLOAT32))
@pytest.mark.parametrize("n", rc.FORMAT_SIZES)
def test_one_kept_coordinate_that_is_no_float32_value_gets_double_records(n, name):
    """... at the last index of the last block: 1 + 2^-24 (rounds), 1e39 (would become inf), FLT_MAX (1 + 2^-25) (finite above FLT_MAX,
    rounds to FLT_MAX); 16-byte records again when the cull removes that point"""
    s = rc.scene()
    z = rc.NOT_FLOAT32[name]
    base, cols, v = format_cloud(n)
    pts = rc.with_last_point(base, z)
    for route in ("spline arrays", "spline cloud"):
        with built_twice(lambda: make_handle(route, pts, v, BF, flags=_lib.FLAG_INPUT_ORDER)) as (h, rec):
            assert h.info()["record_bytes"] == 32, (name, route)
            check_records(rec, pts, cols, BF, 1, order=np.arange(n), what=(n, name, route))
    gone = rc.with_last_point(base, -z)  # behind the camera
    idx = oracle_lib.view_culling(s.model, s.intr, s.dist, rc.W, rc.H, gone, rc.T_IDENTITY, False, min_z=rc.MIN_Z)
    assert n - 1 not in idx and len(idx) >= n - 8
    with built_twice(lambda: make_handle("spline cloud", gone, v, BF, cull=(rc.T_IDENTITY, rc.MIN_Z, False), flags=_lib.FLAG_INPUT_ORDER)) as (h, rec):
        assert h.info()["record_bytes"] == 16, name
        check_records(rec, gone[idx], cols[idx], BF, 1, order=np.arange(len(idx)), what=(n, name, "culled"))


@pytest.mark.parametrize("n", rc.FORMAT_SIZES)
def test_a_float32_subnormal_coordinate_is_stored_exactly(n):
    """2^-149 at the last index: whichever format the builder chooses (not asserted), the stored coordinate has the input's bits"""
    base, cols, v = format_cloud(n)
    pts = rc.with_last_point(base, rc.FLT_DENORM)
    for route in ("spline arrays", "spline cloud"):
        with built_twice(lambda: make_handle(route, pts, v, BF, flags=_lib.FLAG_INPUT_ORDER)) as (h, rec):
            check_records(rec, pts, cols, BF, 1, order=np.arange(n), what=(n, route))
            assert rec["xyz"][-1, 2] == rc.FLT_DENORM


# ---- g: sharded masters, and the hook's own argument checks --------------------------------------------------------------------------------


def test_a_sharded_master_on_the_edge_ladder_has_the_plain_handles_sums():
    s = rc.scene()
    pts, v = rc.ladder_cloud(256)
    ref = rc.cached(("ladder spline", 256), lambda: s.o_spline(s.levels_f64, 256, pts=pts, ints=v))
    plain = nid.NIDCost(s.proj, s.levels_f64, pts, v, 256)
    sharded = nid.NIDCost(s.proj, s.levels_f64, pts, v, 256, devices=[0, 0, 0])
    try:
        assert sharded.num_shards() == 3
        ok, c, g = plain(rc.IDENTITY)
        ok2, c2, g2 = sharded(rc.IDENTITY)
        assert ok and ok2 and c2 == c
        fa, fb = plain.histogram_fixed(), sharded.histogram_fixed()
        assert np.array_equal(fa[0], fb[0]) and fa[1:] == fb[1:]
        for a, b in zip(plain.histograms(), sharded.histograms()):
            assert np.array_equal(a, b)
        parity.check_cost(c2, ref["cost"], what="sharded ladder")
        parity.check_grad(g2, ref["grad"], what="sharded ladder")
        c3 = (ctypes.c_int64 * 3)()
        assert _lib.load().nidreg_debug_records(sharded.h, c3, None, 0, None, None, 0) == _lib.NIDREG_ERR_INVALID  # plain handles only
        assert "plain handles only" in _lib.last_error()
    finally:
        plain.close()
        sharded.close()


def test_the_record_hook_refuses_bad_arguments():
    lib = _lib.load()
    cols = rc.random_columns(16, 300)
    h = make_handle("spline arrays", rc.pool_points(300), rc.columns_to_intensities(cols, 16), 16, columns_per_group=3)
    try:
        c3 = (ctypes.c_int64 * 3)()
        g = np.zeros(7, dtype=np.int64)
        xyz, b = np.zeros((300, 3)), np.zeros(300, dtype=np.int32)
        gp, xp, bp = g.ctypes.data_as(_lib.c_int64_p), xyz.ctypes.data_as(_lib.c_double_p), b.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        assert lib.nidreg_debug_records(None, c3, None, 0, None, None, 0) == _lib.NIDREG_ERR_INVALID
        assert lib.nidreg_debug_records(h.h, None, None, 0, None, None, 0) == _lib.NIDREG_ERR_INVALID
        assert lib.nidreg_debug_records(h.h, c3, gp, 6, None, None, 0) == _lib.NIDREG_ERR_INVALID  # NG + 1 = 7
        assert lib.nidreg_debug_records(h.h, c3, None, 0, xp, None, 300) == _lib.NIDREG_ERR_INVALID
        assert lib.nidreg_debug_records(h.h, c3, None, 0, xp, bp, 299) == _lib.NIDREG_ERR_INVALID
        assert not g.any() and not xyz.any() and not b.any()  # a refused call writes nothing
        assert lib.nidreg_debug_records(h.h, c3, None, 0, None, None, 0) == _lib.NIDREG_OK and list(c3) == [300, 6, 3]
        assert lib.nidreg_debug_records(h.h, c3, gp, 7, xp, bp, 300) == _lib.NIDREG_OK
        check_records(dict(num_records=300, NG=6, GW=3, gcount=g, xyz=xyz, bin=b), rc.pool_points(300), cols, 3, 6)
    finally:
        h.close()
