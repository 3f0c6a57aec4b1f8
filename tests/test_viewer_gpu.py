"""The headless viewer end to end (python -m direct_visual_lidar_calibration_amd.viewer) on a small synthetic bag: 20 000 points, a
160 x 120 distorted pinhole, calib.json with the TRUE pose as results.T_lidar_camera and a perturbed one as
results.init_T_lidar_camera_auto.

The perturbation (10 / -5 / 5 cm, 2 / -3 / 2.5 deg) is chosen so that the CPU oracle's NID (CostCalculatorNID, 16 bins, on the oracle's
own culled cloud) is larger at the guess than at the truth: 0.998062 at the guess against 0.903785 at the truth, checked on the CPU
by test_the_guess_scores_worse_than_the_truth_on_the_oracle.  Files are compared with what the CPU oracles compose from the same
inputs: exactly."""
import json
import math
import os

import numpy as np
import pytest

import oracle_lib
import parity
import viewer_oracle
from direct_visual_lidar_calibration_amd import dataset, nid, render, se3, synth, viewer

CAMERA = ("plumb_bob", [100.0, 100.0, 80.0, 60.0], [-0.04, 0.08, 1e-4, -3e-4, -0.04], 160, 120)
BAG = "bag0"
DELTA = np.array([0.10, -0.05, 0.05, math.radians(2.0), math.radians(-3.0), math.radians(2.5)])
VIEW = (96, 64)
ORBIT = [-20.0, 20.0]
LABELS = {"result": "T_lidar_camera", "init_auto": "init_T_lidar_camera_auto"}

_cache = {}


def scene():
    if "scene" not in _cache:
        _cache["scene"] = synth.make_scene(CAMERA, num_points=20000, seed=77)
    return _cache["scene"]


def tums():
    sc = scene()
    return {"result": dataset.T_camera_lidar_to_tum(sc.T_camera_lidar_true), "init_auto": dataset.T_camera_lidar_to_tum(se3.plus(sc.T_camera_lidar_true, DELTA))}


def T_camera_lidar(label):
    """as the command derives it from calib.json (json round-trips doubles exactly)"""
    return np.linalg.inv(viewer.tum_to_pose(tums()[label]))


def oracle_views(label):
    """What the CPU oracles make of one transform: culled indices, NID, overlay and its index image, the quantised colours"""
    if label not in _cache:
        sc = scene()
        model, intr, dist, W, H = CAMERA
        T = T_camera_lidar(label)
        keep = oracle_lib.view_culling(model, intr, dist, W, H, sc.points, T, True)
        fov = oracle_lib.estimate_camera_fov(model, intr, dist, W, H)
        value, _ = oracle_lib.cost_calculator_nid(model, intr, dist, sc.image_u8, sc.points[keep], sc.intensities[keep], 16, fov, T)
        proj = nid.create_camera(model, intr, dist)
        min_nz = math.cos(nid.estimate_camera_fov(proj, (W, H)) + 0.5 * math.pi / 180.0)  # (host code: the gate SplatRenderer.draw derives)
        grey = np.repeat(sc.image_u8[:, :, None], 3, axis=2)
        overlay, index = viewer_oracle.draw(model, intr, dist, sc.points[keep], render.quantize_colors(render.colormap_turbo(sc.intensities[keep])), T, W, H, min_nz, radius=1,
                                            background=grey, alpha=178)
        rgba = render.quantize_colors(oracle_lib.points_color_update(model, intr, dist, sc.image_u8, sc.points, render.colormap_turbo(sc.intensities), T, 0.7)[0])
        _cache[label] = dict(keep=keep, nid=value, overlay=overlay, index=index, rgba=rgba, T=T)
    return _cache[label]


def test_the_guess_scores_worse_than_the_truth_on_the_oracle():
    """(CPU) the condition the GPU test's ordering check rests on, and the two values its docstring quotes"""
    truth, guess = oracle_views("result"), oracle_views("init_auto")
    print(f"oracle NID: truth {truth['nid']:.6f}, guess {guess['nid']:.6f}; culled {len(truth['keep'])} / {len(guess['keep'])}")
    assert truth["nid"] < guess["nid"] - 0.05
    assert abs(truth["nid"] - 0.903785) < 1e-6 and abs(guess["nid"] - 0.998062) < 1e-6
    assert (truth["rgba"][:, 3] > 0).sum() > 10000 and (guess["rgba"][:, 3] == 0).sum() > 0  # the guess pushes some points out of the image


@pytest.fixture(scope="module")
def run_all(tmp_path_factory):
    sc = scene()
    d = str(tmp_path_factory.mktemp("viewer_data"))
    config = dataset.write_preprocessed(d, CAMERA[:3], [(BAG, sc.image_u8, sc.points, sc.intensities)])
    config["results"] = {LABELS[k]: v for k, v in tums().items()}
    dataset.write_calib(d, config)
    before = sorted(os.listdir(d))
    rc = viewer.main([d, "--transformation", "all", "--save_ply", "--view_size", f"{VIEW[0]}x{VIEW[1]}", "--orbit_deg", ",".join(str(a) for a in ORBIT)], )
    assert rc == 0 and sorted(os.listdir(d)) == before + ["viewer"]
    return d, os.path.join(d, "viewer")


@pytest.mark.gpu
def test_every_named_file_exists_with_the_right_size(run_all):
    _, out = run_all
    n = len(scene().points)
    want = ["viewer.json"]
    for label in LABELS:
        want += [f"{BAG}_{label}_overlay.png", f"{BAG}_{label}_colored.ply"] + [f"{BAG}_{label}_orbit{k}.png" for k in range(len(ORBIT))]
    assert sorted(os.listdir(out)) == sorted(want)
    for label in LABELS:
        img, depth = dataset.read_png(os.path.join(out, f"{BAG}_{label}_overlay.png"))
        assert img.shape == (CAMERA[4], CAMERA[3], 3) and depth == 8
        views = []
        for k in range(len(ORBIT)):
            img, depth = dataset.read_png(os.path.join(out, f"{BAG}_{label}_orbit{k}.png"))
            assert img.shape == (VIEW[1], VIEW[0], 3) and depth == 8 and img.any()
            views.append(img)
        assert not np.array_equal(views[0], views[1])
        data = open(os.path.join(out, f"{BAG}_{label}_colored.ply"), "rb").read()
        assert len(data) == data.index(b"end_header\n") + len(b"end_header\n") + 15 * n and f"element vertex {n}\n".encode() in data


@pytest.mark.gpu
def test_each_overlay_equals_the_oracles_composition(run_all):
    _, out = run_all
    for label in LABELS:
        img, _ = dataset.read_png(os.path.join(out, f"{BAG}_{label}_overlay.png"))
        want = oracle_views(label)["overlay"]
        assert np.array_equal(img, want), f"{label}: {np.argwhere(img != want)[:8].tolist()}"
    assert not np.array_equal(oracle_views("result")["overlay"], oracle_views("init_auto")["overlay"])


@pytest.mark.gpu
def test_viewer_json_counts_and_orders_the_nids_as_the_oracle_does(run_all):
    _, out = run_all
    with open(os.path.join(out, "viewer.json")) as f:
        report = json.load(f)
    assert sorted(report["transformations"]) == sorted(LABELS) and report["nid_bins"] == 16
    for label in LABELS:
        entry, o = report["transformations"][label], oracle_views(label)
        bag = entry["bags"][BAG]
        assert bag["points"] == len(scene().points) and bag["culled"] == len(o["keep"]) and bag["overlay_pixels_covered"] == int((o["index"] >= 0).sum())
        assert bag["colored"] == int((o["rgba"][:, 3] > 0).sum())
        assert entry["nid_sum"] == bag["nid"] and abs(bag["nid"] - o["nid"]) < parity.COST_ATOL  # (the bar the cost paths' own tests hold against the oracle)
        assert np.array_equal(np.array(entry["T_lidar_camera"]).reshape(4, 4), viewer.tum_to_pose(tums()[label]))
    nids = {label: report["transformations"][label]["nid_sum"] for label in LABELS}
    assert (nids["result"] < nids["init_auto"]) == (oracle_views("result")["nid"] < oracle_views("init_auto")["nid"]) and nids["result"] < nids["init_auto"]


@pytest.mark.gpu
def test_the_ply_colours_are_the_quantised_colour_update(run_all):
    _, out = run_all
    sc = scene()
    for label in LABELS:
        data = open(os.path.join(out, f"{BAG}_{label}_colored.ply"), "rb").read()
        body = np.frombuffer(data, dtype=np.uint8, offset=data.index(b"end_header\n") + len(b"end_header\n")).reshape(-1, 15)
        assert body[:, :12].tobytes() == sc.points[:, :3].astype("<f4").tobytes()
        assert np.array_equal(body[:, 12:], oracle_views(label)["rgba"][:, :3])


@pytest.mark.gpu
def test_an_orbit_view_equals_the_oracles(run_all):
    """The first orbit view of the result: the coloured subset of the cloud through the distortion-free view camera at the orbit pose."""
    _, out = run_all
    sc, o = scene(), oracle_views("result")
    seen = o["rgba"][:, 3] > 0
    cam = viewer.view_camera(VIEW, 60.0)
    intr, dist = [float(v) for v in cam._intr5[:4]], [0.0] * 5
    min_nz = math.cos(nid.estimate_camera_fov(cam, VIEW) + 0.5 * math.pi / 180.0)
    T = viewer.orbit_pose(o["T"], ORBIT[0], sc.points[seen, :3].mean(axis=0))
    want, _ = viewer_oracle.draw("plumb_bob", intr, dist, sc.points[seen], o["rgba"][seen], T, VIEW[0], VIEW[1], min_nz, radius=1)
    img, _ = dataset.read_png(os.path.join(out, f"{BAG}_result_orbit0.png"))
    assert want.any() and np.array_equal(img, want)


@pytest.mark.gpu
def test_the_default_writes_only_the_result(run_all, tmp_path):
    d, _ = run_all
    dst = str(tmp_path / "last")
    assert viewer.main([d, "--dst_path", dst, "--view_size", "48x32", "--orbit_deg=10"]) == 0
    assert sorted(os.listdir(dst)) == sorted([f"{BAG}_result_overlay.png", f"{BAG}_result_orbit0.png", "viewer.json"])
    with open(os.path.join(dst, "viewer.json")) as f:
        assert list(json.load(f)["transformations"]) == ["result"]
