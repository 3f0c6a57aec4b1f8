"""CPU side of the record-builder tests: the conditions the inputs of test_record_builder_gpu.py (tests/record_cases.py) have to meet, so
that no GPU test passes vacuously, and the Python restatement of the rules (tests/record_oracle.py) against the compiled oracle."""
import numpy as np
import pytest

import oracle_lib
import record_cases as rc
import record_oracle as ro


def oracle_hist_points(pts, ints, B):
    s = rc.scene()
    return s.o_spline(s.levels_f64, B, pts=pts, ints=ints, want_grad=False)["hist_points"]


def test_every_pool_point_is_an_inlier_and_distinct():
    s = rc.scene()
    assert s.pts.shape == (rc.POOL, 4) and np.array_equal(s.pts[:, :3], s.pts[:, :3].astype(np.float32).astype(np.float64))
    assert len(np.unique(s.pts[:, :3], axis=0)) == rc.POOL  # a multiset of records identifies the points
    hp = oracle_hist_points(s.pts, s.ints, 16)
    assert hp.sum() == rc.POOL
    for img in (s.levels_f64, s.levels_u8 / 255.0):
        for B in (300, 4096):
            assert len(np.unique(ro.point_bins(img.ravel(), B))) <= 230
    assert not ro.needs_rec64(s.pts)


@pytest.mark.parametrize("B", rc.EDGE_BINS)
def test_the_ladder_reaches_every_bin_and_straddles_every_edge(B):
    v = rc.ladder(B)
    assert len(v) == 3 * (B + 1)
    b = ro.point_bins(v, B)
    assert set(b) == set(range(B))
    s = ro.point_bins(np.sort(v), B)
    assert np.all(np.diff(s) >= 0) and np.all(np.diff(s) <= 1)  # one ulp across an edge moves at most one bin, and never backwards
    for k in range(1, B):  # one ulp above the edge is in bin k, and k / B or one ulp below it in bin k - 1 -- or the product rounds onto k
        below, at, above = (ro.point_bin(x, B) for x in (np.nextafter(k / B, -np.inf), k / B, np.nextafter(k / B, np.inf)))
        assert above == k and at in (k - 1, k) and below in (k - 1, k) and below <= at
    off = rc.edges_off(B)
    assert len(off) == {100: 3, 300: 12}.get(B, 0), off  # both kinds of edge are in the ladder: k / B in bin k, and k / B in bin k - 1
    assert all(ro.point_bin(k / B, B) == k - 1 for k in off)
    if B in (2, 16, 256):  # k / B and the product are exact
        assert all(ro.point_bin(np.nextafter(k / B, -np.inf), B) == k - 1 for k in range(1, B + 1))


@pytest.mark.parametrize("B", rc.EDGE_BINS)
def test_the_special_values_land_where_the_rule_says(B):
    first, last = rc.specials(B)
    for x in (-0.0, -1e-300, 5e-324, np.nan, np.inf, -np.inf, 1e10, 2.0**31 / B):
        assert any(np.array_equal([x], [y], equal_nan=True) and np.signbit(x) == np.signbit(y) for y in first)
    for x in (1.0, np.nextafter(1.0, 0.0), 1.5, (2.0**31 - 1) / B):
        assert x in last
    assert np.all(ro.point_bins(first, B) == 0) and np.all(ro.point_bins(last, B) == B - 1)
    with np.errstate(all="ignore"):
        assert ro.cast_int(np.float64(2.0**31 / B) * B) == ro.INT_MIN and ro.cast_int(np.float64(np.nan)) == ro.INT_MIN  # the wrap, not a clamp from above
        assert ro.cast_int(np.float64((2.0**31 - 1) / B) * B) >= 2**31 - 2
        assert ro.cast_int(np.float64(-2147483649.0 / B) * B) in (ro.INT_MIN, -2147483648)


@pytest.mark.parametrize("B", rc.EDGE_BINS)
def test_the_ladder_that_goes_to_the_device(B):
    """all of it up to 256 bins; at 300 bins a part that occupies at most 256 bins and keeps every edge that k / B misses"""
    edges = rc.device_edges(B)
    pts, v = rc.ladder_cloud(B)
    assert len(v) == 3 * len(edges) + 13 and len(pts) == len(v) <= rc.POOL
    b = ro.point_bins(v, B)
    assert len(set(b)) <= 256 and {0, B - 1} <= set(b) and set(rc.edges_off(B)) <= set(edges)
    if B <= 256:
        assert edges == list(range(B + 1)) and set(b) == set(range(B))
    else:
        labels, occupied = ro.compact(b)
        assert len(occupied) > 200 and np.array_equal(occupied[labels], b) and not np.array_equal(labels, b)  # the relabelling moves bins


@pytest.mark.parametrize("B", rc.EDGE_BINS)
def test_point_bin_agrees_with_the_compiled_oracle_on_the_ladder(B):
    """hist_points of the compiled oracle (every point an inlier) = the bincount of point_bin, on the whole ladder and the special values"""
    first, last = rc.specials(B)
    v = np.concatenate([rc.ladder(B), first, last])
    pts = rc.pool_points(len(v))
    assert np.array_equal(oracle_hist_points(pts, v, B), np.bincount(ro.point_bins(v, B), minlength=B))


def test_the_wide_intensities_occupy_256_and_257_bins():
    for occupied in (256, 257):
        v = rc.wide_intensities(occupied)
        b = ro.point_bins(v, rc.WIDE)
        assert len(np.unique(b)) == occupied and len(v) == 4 * occupied
        assert np.array_equal(np.isnan(v), b == 0) and np.array_equal(v == 1.5, b == rc.WIDE - 1) and np.isnan(v).any() and (v == 1.5).any()


@pytest.mark.parametrize("config", rc.GROUP_CONFIGS, ids=str)
def test_the_group_clouds_have_the_empty_groups_they_are_named_after(config):
    B, cpg = config
    GW, NG = rc.group_layout(B, cpg)
    assert (GW, NG) == {(16, 1): (1, 16), (16, 3): (3, 6), (16, 16): (16, 1), (100, 0): (2, 50), (256, 0): (1, 256)}[config]
    pat = rc.group_patterns(B, GW, NG)
    assert len(pat) == (5 if NG > 1 else 3)
    for name, cols in pat.items():
        assert np.array_equal(ro.point_bins(rc.columns_to_intensities(cols, B), B), cols), name
        sizes = np.diff(ro.gcount(cols, GW, NG))
        assert sizes.sum() == len(cols)
        if name == "one column":
            assert (sizes > 0).sum() == 1 and len(set(cols)) == 1
        elif name == "first group":
            assert sizes[0] == len(cols)
        elif name == "last group":
            assert sizes[-1] == len(cols)
        elif name == "first group empty":
            assert sizes[0] == 0 and (sizes[1:] > 0).all()
        else:
            assert np.all(sizes[0::2] == 0) and np.all(sizes[1::2] > 0)
    cols = rc.random_columns(B, 1025)
    assert np.array_equal(ro.point_bins(rc.columns_to_intensities(cols, B), B), cols) and len(set(cols // GW)) > NG // 2


@pytest.mark.parametrize("B", [16, 256])
def test_the_lattice_bearings_sit_in_the_middle_of_their_cells(B):
    pts, cols, cells = rc.lattice(B)
    assert len(pts) == rc.LATTICE_CELLS * rc.LATTICE_COLUMNS * rc.LATTICE_REPEATS and len(set(cells)) == rc.LATTICE_CELLS
    seen = set()
    for p in pts:
        fa, fe = ro.quantised_bearing(*p[:3])
        assert 0.25 <= fa - np.floor(fa) <= 0.75 and 0.25 <= fe - np.floor(fe) <= 0.75, (p, fa, fe)  # the device's atan2 cannot move it to another cell
        seen.add((int(fa), int(fe)))
    assert seen == set(cells)
    m = [ro.morton(*p[:3]) for p in pts]
    assert len(set(m)) == rc.LATTICE_CELLS
    assert oracle_hist_points(pts, rc.columns_to_intensities(cols, B), B).sum() == len(pts)  # every lattice point is an inlier
    order = ro.record_order(pts, cols, 1, False)
    assert not np.array_equal(order, np.arange(len(pts))) and not np.array_equal(order, ro.record_order(pts, cols, 1, True))
    key = [(cols[i], m[i], i) for i in order]
    assert key == sorted(key)
    for p, code in zip(pts, m):  # qa sits in the even bits, qe in the odd ones
        fa, fe = ro.quantised_bearing(*p[:3])
        assert sum(((code >> (2 * b)) & 1) << b for b in range(16)) == int(fa) and sum(((code >> (2 * b + 1)) & 1) << b for b in range(16)) == int(fe)
    assert ro.morton(np.nan, 1.0, 1.0) == 0


def test_the_cull_cases_remove_what_they_are_named_after():
    s = rc.scene()
    cases = rc.cull_cases()
    n = len(cases["nothing removed"][0])

    def kept(name):
        pts, depth = cases[name]
        return oracle_lib.view_culling(s.model, s.intr, s.dist, rc.W, rc.H, pts, rc.T_IDENTITY, depth, min_z=rc.MIN_Z)

    assert np.array_equal(kept("nothing removed"), np.arange(n))
    assert np.array_equal(kept("first removed"), np.arange(1, n))
    assert np.array_equal(kept("last removed"), np.arange(n - 1))
    assert len(kept("everything removed")) == 0
    assert np.array_equal(kept("every seventh removed"), np.flatnonzero(np.arange(n) % 7 != 3))
    occ = kept("occluded points removed")
    gone = np.setdiff1d(np.arange(n), occ)
    assert 100 < len(gone) < n - 100 and set(gone // 256) >= {0, 1, 2, 3} and len(set(occ // 256)) == 5  # in every full 256-thread block


def test_the_format_inputs():
    for n in rc.FORMAT_SIZES:
        pts, planted = rc.float32_cloud(n)
        assert not ro.needs_rec64(pts) and planted[-1] == n - 1
        assert np.signbit(pts[3, 0]) and pts[3, 0] == 0.0 and pts[5, 2] == rc.FLT_MAX and np.isnan(pts[9, 2]) and pts[11, 0] == 2.0**-126
        for name, z in rc.NOT_FLOAT32.items():
            assert np.isfinite(z) and ro.needs_rec64(rc.with_last_point(pts, z)), name
            assert not ro.needs_rec64(rc.with_last_point(pts, z)[:-1])
        sub = rc.with_last_point(pts, rc.FLT_DENORM)
        assert not ro.needs_rec64(sub) and sub[-1, 2] == np.float64(np.float32(rc.FLT_DENORM)) != 0.0  # a float32 value: a subnormal one
    with np.errstate(all="ignore"):
        z = rc.NOT_FLOAT32["FLT_MAX (1 + 2^-25)"]
        assert z > rc.FLT_MAX and np.float32(z) == np.float32(rc.FLT_MAX)  # rounds to FLT_MAX, not to inf: |z| <= FLT_MAX is not the rule
        assert np.isinf(np.float32(1e39))
