"""``evaluate`` end to end on a synthetic two-bag directory (12 000 points a bag): every replicate it reports is the calibration a
caller gets from ``calibrate`` / ``calibrate_pairs`` on the same points, bit for bit, and its summaries follow from the replicates."""
import json
import math
import os
import shutil

import numpy as np
import pytest

import fold_oracle as fo
from direct_visual_lidar_calibration_amd import calibrate, calibration, dataset, evaluate, nid, se3
from test_dataset import _write_synthetic_dir

pytestmark = pytest.mark.gpu

ARGS = ["--folds", "4", "--restarts", "3", "--sweep_steps", "5"]
QUIET = lambda *_: None  # noqa: E731


def strip_seconds(o):
    if isinstance(o, dict):
        return {k: strip_seconds(v) for k, v in o.items() if k != "seconds"}
    if isinstance(o, list):
        return [strip_seconds(v) for v in o]
    return o


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("evaluate") / "data")
    scenes, _ = _write_synthetic_dir(d, n=12000, bags=2, seed=21)
    _, init_x, x_full = calibrate.run(calibrate.build_parser().parse_args([d]), log=QUIET)  # writes results.T_lidar_camera
    calib_bytes = open(os.path.join(d, "calib.json"), "rb").read()
    lines = []
    out = evaluate.run(evaluate.build_parser().parse_args([d] + ARGS), log=lines.append)
    _, bags = dataset.load_dataset(d)
    s = scenes[0]
    return dict(d=d, scenes=scenes, init_x=init_x, x_full=x_full, calib_bytes=calib_bytes, out=out, lines=lines, bags=bags, proj=nid.create_camera(s.model, s.intrinsics, s.distortion))


def gathered_pairs(case, K, k, complement, seed=0, cell=1.0):
    pairs = []
    for p, b in enumerate(case["bags"]):
        idx = fo.fold_indices(b.points, seed + p, K, k, complement, cell)
        pairs.append((b.image, np.ascontiguousarray(b.points[idx]), np.ascontiguousarray(b.intensities[idx])))
    return pairs


def test_calib_json_is_untouched_and_full_is_calibrates_pose(case):
    d, out = case["d"], case["out"]
    assert open(os.path.join(d, "calib.json"), "rb").read() == case["calib_bytes"]
    saved = json.load(open(os.path.join(d, "calib.json")))["results"]["T_lidar_camera"]
    assert out["full"]["T_lidar_camera"] == saved == dataset.T_camera_lidar_to_tum(case["x_full"])  # bit for bit
    assert out["stored_vs_full"]["trans"] < 1e-12 and out["stored_vs_full"]["rot"] < 1e-7  # (the TUM round trip re-normalises the quaternion)
    assert json.load(open(os.path.join(d, "evaluate.json"))) == json.loads(json.dumps(out))
    assert out["bags"] == ["bag0", "bag1"] and out["points"] == [12000, 12000]
    # one log line per replicate
    for what in ["fold 0", "fold 3", "without bag0", "without bag1", "restart 0", "restart 2", "sweep tx", "sweep rz"]:
        assert any(ln.startswith(what) for ln in case["lines"]), what


def test_fold_sizes_and_replicate_one_against_the_host_gathered_complements(case):
    import oracle_lib
    from test_calibration import OracleNIDCost, OracleNearest, oracle_cull

    out = case["out"]
    folds = out["folds"]
    assert folds["mode"] == "jackknife" and folds["num_folds"] == 4 and folds["cell"] == 1.0 and "lower bound" in folds["note"] and "approximate" in folds["note"]
    for p, b in enumerate(case["bags"]):
        assert folds["sizes"][p] == fo.fold_ids(b.points, p, 4, 1.0)[1].tolist()
    pairs = gathered_pairs(case, 4, 1, True)
    rep = folds["replicates"][1]
    assert rep["fold"] == 1 and rep["points"] == [len(p[1]) for p in pairs] == [12000 - folds["sizes"][p][1] for p in range(2)]
    params = calibration.VisualCameraCalibrationParams()
    x, cal = calibrate.calibrate_pairs(case["proj"], pairs, case["init_x"], params)
    assert rep["T_lidar_camera"] == dataset.T_camera_lidar_to_tum(x) and rep["final_cost"] == cal.log[-1]["final_cost"]  # bit for bit
    assert rep["evaluations"] == sum(e["evaluations"] for e in cal.log)
    assert rep["d"] == evaluate.pose_delta(case["x_full"], x)
    # the same replicate on the CPU oracle driver, within the project's bar
    s = case["scenes"][0]
    max_fov = oracle_lib.estimate_camera_fov(s.model, s.intrinsics, s.distortion, s.width, s.height)
    ref = calibration.VisualCameraCalibration(
        pairs, params, nid_cost_factory=lambda i, pt, it, b: OracleNIDCost(s, i, pt, it, b), nearest_cost_factory=lambda i, pt, it, b: OracleNearest(s, i, pt, it, b, max_fov),
        cull=oracle_cull(s))
    dt, dr = se3.delta_trans_rot(ref.calibrate(case["init_x"]), x)
    print(f"fold replicate 1 against the CPU oracle driver: {dt:.3e} m, {dr:.3e} rad")
    assert dt <= 1e-3 and dr <= 1e-3, (dt, dr)


def test_leaving_out_bag_one_is_calibrate_on_the_first_bag(case, tmp_path):
    d2 = str(tmp_path / "copy")
    shutil.copytree(case["d"], d2)
    _, _, x = calibrate.run(calibrate.build_parser().parse_args([d2, "--first_n_bags", "1"]), log=QUIET)
    loo = case["out"]["leave_one_out"]
    assert [r["left_out"] for r in loo["replicates"]] == ["bag0", "bag1"]
    assert loo["replicates"][1]["T_lidar_camera"] == dataset.T_camera_lidar_to_tum(x)  # bit for bit
    assert (loo["max_trans"], loo["max_rot"]) == evaluate.maxima([r["d"] for r in loo["replicates"]])


def test_summaries_follow_from_the_listed_replicates(case):
    out = case["out"]
    ds = np.array([r["d"] for r in out["folds"]["replicates"]])
    assert ds.shape == (4, 6)
    mean = ds.mean(axis=0)
    se = np.sqrt(3.0 / 4.0 * ((ds - mean) ** 2).sum(axis=0))
    assert np.allclose(out["folds"]["se"], se, rtol=1e-12, atol=0) and np.allclose(out["folds"]["mean_d"], mean, rtol=1e-12, atol=1e-300)
    assert out["folds"]["max_trans"] == float(np.linalg.norm(ds[:, :3], axis=1).max()) and out["folds"]["max_rot"] == float(np.linalg.norm(ds[:, 3:], axis=1).max())
    rs = out["restarts"]
    assert len(rs["replicates"]) == 3
    for r in rs["replicates"]:
        start = evaluate.restart_pose(case["x_full"], 0, r["r"], 0.05, 1.0)
        assert r["start_T_lidar_camera"] == dataset.T_camera_lidar_to_tum(start)
        assert r["agrees"] == bool(np.linalg.norm(r["d"][:3]) <= 0.01 and np.linalg.norm(r["d"][3:]) <= math.radians(0.1))
    assert rs["agree_share"] == sum(r["agrees"] for r in rs["replicates"]) / 3


def test_every_sweep_sample_is_a_direct_multi_call(case):
    out, x_full, proj = case["out"], case["x_full"], case["proj"]
    size = (case["bags"][0].image.shape[1], case["bags"][0].image.shape[0])
    min_z = math.cos(nid.estimate_camera_fov(proj, size))
    clouds = [nid.Cloud(b.points, b.intensities) for b in case["bags"]]
    costs = [nid.NIDCost.from_cloud(proj, b.image.astype(np.float64) * (1.0 / 255.0), c, 16, cull=(se3.to_matrix(x_full), min_z, True)) for b, c in zip(case["bags"], clouds)]
    multi = calibrate._Multi(x_full, costs)
    centre = multi(x_full, want_grad=False)[1]
    sw = out["sweeps"]
    assert sw["steps"] == 5 and sw["centre_cost"] == centre and sorted(sw["axes"]) == sorted(evaluate.AXES)
    for a, name in enumerate(evaluate.AXES):
        ax = sw["axes"][name]
        assert ax["delta"] == evaluate.sweep_deltas(5, 0.05 if a < 3 else math.radians(1.0)) and ax["delta"][2] == 0.0
        for j, delta in enumerate(ax["delta"]):
            ok, c, _ = multi(evaluate.sweep_pose(x_full, a, delta), want_grad=False)
            assert ok and ax["cost"][j] == c, (name, j)  # bit for bit
        assert ax["cost"][2] == centre
        assert ax["argmin"] == int(np.argmin(ax["cost"])) and ax["interior"] == (0 < ax["argmin"] < 4)
    for h in costs + clouds:
        h.close()


def test_a_second_run_writes_the_same_json_apart_from_the_seconds(case, tmp_path):
    dst = str(tmp_path / "again")
    again = evaluate.run(evaluate.build_parser().parse_args([case["d"]] + ARGS + ["--dst_path", dst]), log=QUIET)
    assert not os.path.exists(os.path.join(dst, "calib.json"))
    a, b = strip_seconds(json.load(open(os.path.join(dst, "evaluate.json")))), strip_seconds(json.loads(json.dumps(case["out"])))
    assert a["arguments"].pop("dst_path") == dst and b["arguments"].pop("dst_path") is None
    assert a == b
    assert "seconds" in again["full"] and all("seconds" in again[k] for k in ("folds", "leave_one_out", "restarts", "sweeps", "upload"))


def test_another_seed_gives_other_fold_sizes(case, tmp_path):
    small = ["--folds", "2", "--restarts", "0", "--sweep_steps", "0", "--no_leave_one_out", "--dst_path", str(tmp_path)]
    a = evaluate.run(evaluate.build_parser().parse_args([case["d"]] + small + ["--seed", "1"]), log=QUIET)
    b = evaluate.run(evaluate.build_parser().parse_args([case["d"]] + small + ["--seed", "2", "--fold_mode", "subset"]), log=QUIET)
    assert a["folds"]["sizes"] != b["folds"]["sizes"] and a["folds"]["sizes"][0] == fo.fold_ids(case["bags"][0].points, 1, 2, 1.0)[1].tolist()
    assert a["leave_one_out"] is None and a["restarts"] is None and a["sweeps"] is None
    # subset mode: replicate k holds fold k alone, and reports no se
    assert b["folds"]["replicates"][1]["points"] == [s[1] for s in b["folds"]["sizes"]] and b["folds"]["se"] is None and b["folds"]["max_trans"] is not None


def test_with_a_mask_the_replicates_go_through_the_select_route(case, tmp_path):
    H, W = case["bags"][0].image.shape
    mask = np.full((H, W), 255, dtype=np.uint8)
    mask[:, : W // 4] = 0
    path = str(tmp_path / "mask.png")
    dataset.write_png_gray(path, mask)
    lines = []
    out = evaluate.run(evaluate.build_parser().parse_args([case["d"], "--mask", path, "--folds", "2", "--restarts", "0", "--sweep_steps", "0", "--no_leave_one_out", "--dst_path", str(tmp_path)]),
                       log=lines.append)
    sel = {"masks": [mask, mask], "margin": 2, "min_range": 0.0, "max_range": math.inf}
    pairs = gathered_pairs(case, 2, 0, True)
    selects = []
    x, cal = calibrate.calibrate_pairs(case["proj"], pairs, case["init_x"], calibration.VisualCameraCalibrationParams(), selection=sel, log=selects.append)
    rep = out["folds"]["replicates"][0]
    assert rep["T_lidar_camera"] == dataset.T_camera_lidar_to_tum(x) and rep["final_cost"] == cal.log[-1]["final_cost"]  # bit for bit
    assert selects and all("the mask removed" in ln for ln in selects) and not any(" the mask removed 0," in ln for ln in selects)
    # and the mask matters: the unmasked full calibration ends elsewhere
    assert out["full"]["T_lidar_camera"] != case["out"]["full"]["T_lidar_camera"]
