"""The evaluation's serial stages keep their bits: histogram flush, k_entropy, the gradient kernel's prologue, the hand-over of
the idle histogram buffer's clearing between the kernels, the finalising workgroup.

tests/golden/eval_stage_parent_bits.npz (tools/make_eval_stage_golden.py) holds, for small clouds at every tiling route (16 bins:
several columns per workgroup, no entropy kernel, one-launch route and NIDREG_FUSED=0; 64: k_entropy + lane-private G copies; 256:
the WIDE histogram kernel + single-column gradient kernel, chunks running across columns at 4097 points; 300: the generic
single-column kernels), what the commit BEFORE these stages were trimmed returned: cost, gradient, ok, inlier count, digests of the
raw histogram words.  Every value must come back bit for bit -- through one handle evaluating cost-only and cost+Jacobian in a mixed
order (whichever kernel clears the next evaluation's buffer, it must be zero when that evaluation starts), through the pipelined
submit / wait route with 8 in flight, and through a two-pair nidreg_eval_multi."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_eval_stage_golden as gold  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(ROOT, "tests", "golden", "eval_stage_parent_bits.npz")
CASES = gold.case_list()
# 16 bins: the one-launch route (when the caller has the device to itself) and the three-kernel route
ROUTES = [(c, r) for c in CASES for r in (("default", "unfused") if c["bins"] == 16 else ("default",))]


@pytest.fixture(scope="module")
def fx():
    z = np.load(FIXTURE)
    data = {k: z[k] for k in z.files}
    stored = json.loads(str(data["cases"]))
    assert stored == CASES, "the fixture was written for another case list: re-run tools/make_eval_stage_golden.py on the parent build"
    assert json.loads(str(data["multi"])) == [list(m) for m in gold.MULTI]
    return data


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def check_eval(fx, i, p, wg, ok, c, g, where):
    assert bool(ok) == bool(fx["r_ok"][i, p, wg]), (where, ok)
    assert bits([c])[0] == bits(fx["r_cost"][i, p, wg : wg + 1])[0], (where, c, float(fx["r_cost"][i, p, wg]))
    if wg:
        assert np.array_equal(bits(g), bits(fx["r_grad"][i, p, wg])), (where, g, fx["r_grad"][i, p, wg])


def check_hist(fx, i, p, wg, cost, where):
    inl, d_fixed, d_f64 = gold.hist_record(cost)
    assert inl == int(fx["r_inl"][i, p, wg]), (where, inl)
    assert np.array_equal(d_fixed, fx["r_dfixed"][i, p, wg]), (where, "fixed-point joint histogram words")
    assert np.array_equal(d_f64, fx["r_df64"][i, p, wg]), (where, "joint / image / points histograms")


class _Route:
    """NIDREG_FUSED=0 in the environment while the handle plans its route (read at its first cost+Jacobian evaluation)."""

    def __init__(self, route):
        self.off = route == "unfused"

    def __enter__(self):
        self.old = os.environ.get("NIDREG_FUSED")
        if self.off:
            os.environ["NIDREG_FUSED"] = "0"

    def __exit__(self, *exc):
        if self.off:
            if self.old is None:
                os.environ.pop("NIDREG_FUSED", None)
            else:
                os.environ["NIDREG_FUSED"] = self.old


@pytest.mark.parametrize("case,route", ROUTES, ids=[f"{c['name']}-{r}" for c, r in ROUTES])
def test_mixed_sequence_and_pipelined(fx, case, route):
    from direct_visual_lidar_calibration_amd import nid

    i = CASES.index(case)
    poses = fx["poses"]
    with _Route(route):
        cost = gold.make_cost(nid, fx, case)
        try:
            # grad, cost, grad, grad, cost, cost, grad over the three poses: the clearing of the idle buffer changes hands
            for step, (p, wg) in enumerate(gold.SEQUENCE):
                ok, c, g = cost(poses[p], want_grad=bool(wg))
                where = (case["name"], route, "step", step, "pose", p, "want_grad", wg)
                check_eval(fx, i, p, wg, ok, c, g, where)
                check_hist(fx, i, p, wg, cost, where)
            # the same poses through submit / wait, 8 in flight (7 queued ahead of the one being collected)
            order = [k % 3 for k in range(10)]
            for wg in (1, 0, 1):
                all_ok, cs, gs = cost.eval_batch(poses[order], want_grad=bool(wg), pipelined=True)
                assert bool(all_ok) == bool(all(fx["r_ok"][i, p, wg] for p in order))
                for k, p in enumerate(order):
                    where = (case["name"], route, "pipelined", k, "pose", p, "want_grad", wg)
                    assert bits([cs[k]])[0] == bits(fx["r_cost"][i, p, wg : wg + 1])[0], where
                    if wg:
                        assert np.array_equal(bits(gs[k]), bits(fx["r_grad"][i, p, wg])), where
                check_hist(fx, i, order[-1], wg, cost, (case["name"], route, "after pipelined", wg))
            # and a synchronous evaluation behind the pipelined ones
            ok, c, g = cost(poses[0], want_grad=True)
            check_eval(fx, i, 0, 1, ok, c, g, (case["name"], route, "after pipelined"))
        finally:
            cost.close()


@pytest.mark.parametrize("group", range(len(gold.MULTI)), ids=["+".join(m) for m in gold.MULTI])
def test_two_pair_multi(fx, group):
    """nidreg_eval_multi over two pairs: every pair's histogram and inlier count equal its single-handle evaluation's; the summed
    cost is the sum of the two single-handle costs; cost and gradient equal what the group returned before (the group's gradient
    follows its own chunk table, so its bits are the group's, not the sum of the single-handle gradients)."""
    from direct_visual_lidar_calibration_amd import nid

    names = gold.MULTI[group]
    idx = [next(k for k, c in enumerate(CASES) if c["name"] == n) for n in names]
    poses = fx["poses"]
    hs = [gold.make_cost(nid, fx, CASES[k]) for k in idx]
    try:
        multi = nid.MultiNIDCost(None)
        for h in hs:
            multi.add(h)
        for p, wg in gold.SEQUENCE:
            ok, c, g = multi(poses[p], want_grad=bool(wg))
            where = (names, "pose", p, "want_grad", wg)
            assert bool(ok) == bool(fx["m_ok"][group, p, wg]), where
            assert bits([c])[0] == bits(fx["m_cost"][group, p, wg : wg + 1])[0], where
            single = fx["r_cost"][idx[0], p, wg] + fx["r_cost"][idx[1], p, wg]
            assert bits([c])[0] == bits([single])[0], where
            if wg:
                assert np.array_equal(bits(g), bits(fx["m_grad"][group, p, wg])), where
            for h, k in zip(hs, idx):
                check_hist(fx, k, p, wg, h, where + (CASES[k]["name"],))
        # a pair evaluated alone right behind the group's evaluations (its buffers were last cleared by the group's kernels)
        for h, k in zip(hs, idx):
            ok, c, g = h(poses[2], want_grad=True)
            check_eval(fx, k, 2, 1, ok, c, g, (names, "single after multi", CASES[k]["name"]))
            check_hist(fx, k, 2, 1, h, (names, "single after multi", CASES[k]["name"]))
    finally:
        for h in hs:
            h.close()
