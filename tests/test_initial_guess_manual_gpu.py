"""The headless initial_guess_manual on the GPU (python -m direct_visual_lidar_calibration_amd.initial_guess_manual).

Small scene (20 000 points, pinhole_vga; and a 256 x 128 equirectangular camera): the sheets equal the CPU oracle's restatement of the
splat renderer (tests/viewer_oracle.py) byte for byte, a pick returns the point that was drawn, the candidates' pictures and NIDs are
the viewer's.

End to end on the scene the project's pose bars were measured on (tests/find_matches_scene.py: 1M points, 512 x 512 ``lidar`` sheet): 24
hand picks -- ground-truth projections rounded to integer pixels -- give bit for bit the pose ``initial_guess_auto`` gives for the same
pairs; that pose lies within the matcher's recorded guess error (profiles/find_matches.json: 2.33e-2 m / 1.90e-3 rad, a start from which
``calibrate`` is measured to converge); ``calibrate`` from it ends where it ends from the scene's own initial guess; turning the camera
sheet changes nothing; one gross outlier among the 24 is flagged and does not move the pose out of the bound.

Measured on an MI355X (profiles/initial_guess_manual.json; the test prints each figure before it asserts): 84 991 covered pixels, 48 of
the 144 grid pixels covered, all 48 survive, every 2nd is a pick.  24 picks: 3.447e-3 m / 5.374e-4 rad from the truth, 24 RANSAC inliers,
worst residual 0.54 px -- the minimum the least squares reaches from the TRUE rotation on these picks, so the RANSAC winner's rotation is
start enough.  With pick 7 moved 200 px: 3.223e-3 m / 3.256e-4 rad, 23 inliers, the moved pick's residual 199.7 px.  Bound 2.328e-2 m /
1.895e-3 rad.  calibrate: existing code's two ends 1.045e-3 m / 8.554e-5 rad apart -> bars 2.091e-3 m / 1e-3 rad; from the manual guess it
ends 2.359e-4 m / 1.882e-5 rad from where it ends from the scene's own guess."""
import json
import math
import os

import numpy as np
import pytest

import find_matches_scene as fms
import manual_guess_scene as mgs
import oracle_lib
import viewer_oracle
from direct_visual_lidar_calibration_amd import dataset, initial_guess_manual as igm, matching, nid, pose, preprocess, se3, synth, viewer

pytestmark = pytest.mark.gpu

BAG = "bag0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQUIRECT = ("equirectangular", [256.0, 128.0], [], 256, 128)
# default, candidate:5 and panorama are the views this check was specified with.  The scene's cloud lies within the camera's field of view about the LiDAR's +x, so
# candidate 5 (facing +y) sees nothing: its sheets must be as blank as the oracle's.  candidate:1 adds a rolled view that does see the cloud.
VIEWS = ["default", "candidate:5", "panorama", "candidate:1"]
DELTA_T_BAR = 1e-3  # the project's bar on a calibration result [m] and [rad] (tests/test_find_matches_e2e.py)


# ------------------------------------------------------------------------------------------------ the small scene
def write_scene(d, camera):
    sc = synth.make_scene(camera, num_points=20000, seed=7)
    dataset.write_preprocessed(d, (sc.model, sc.intrinsics, sc.distortion), [(BAG, sc.image_u8, sc.points, sc.intensities)])
    return sc


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """Both small directories with their sheets drawn: {name: (directory, sheets directory, sheets.json, the bag as the command loads it)}"""
    out = {}
    for name, camera, views in (("pinhole", "pinhole_vga", VIEWS), ("equirect", EQUIRECT, ["default"])):
        d = str(tmp_path_factory.mktemp(f"manual_{name}") / "data")
        write_scene(d, camera)
        argv = [d, "--sheets"]
        for v in views:
            argv += ["--view", v]
        before = sorted(os.listdir(d))
        assert igm.run(igm.parse_args(argv), log=lambda *_: None) == 0 and sorted(os.listdir(d)) == before + ["manual"]
        with open(os.path.join(d, "manual", "sheets.json")) as f:
            sheets = json.load(f)
        out[name] = (d, os.path.join(d, "manual"), sheets, dataset.load_dataset(d)[1][0])
    return out


def every_sheet(small):
    for name, (d, dst, sheets, bag) in small.items():
        for view in sheets["views"]:
            yield name, d, dst, bag, view, view["bags"][BAG]


def test_the_sheets_equal_the_oracle(small):
    assert [v["spec"] for v in small["pinhole"][2]["views"]] == VIEWS and [v["name"] for v in small["pinhole"][2]["views"]] == ["v0", "v1", "v2", "v3"]
    assert sorted(os.listdir(small["equirect"][1])) == sorted([f"{BAG}_camera.png", f"{BAG}_v0.png", f"{BAG}_v0_indices.png", "sheets.json"])
    for name, d, dst, bag, view, entry in every_sheet(small):
        config = dataset.read_calib(d)
        model = config["camera"]["camera_model"]
        k = {"default": 0, "candidate:5": 5, "candidate:1": 1}.get(view["spec"])
        if k is None:  # the panorama: preprocess.lidar_camera's equirectangular camera
            assert (view["camera_model"], view["intrinsics"], entry["size"]) == ("equirectangular", [1920.0, 960.0], [1920, 960])
            T_lidar_camera = preprocess.lidar_camera(math.pi)[3]
        else:  # through the camera's own model and image size
            assert (view["camera_model"], view["intrinsics"], entry["size"]) == (model, config["camera"]["intrinsics"], [bag.image.shape[1], bag.image.shape[0]])
            T_lidar_camera = igm.candidate_pose(k, model)
        T = np.linalg.inv(T_lidar_camera)
        assert np.array_equal(np.array(entry["T_view_lidar"]).reshape(4, 4), T) and entry["cloud_length"] == 20000 and view["radius"] == 1
        W, H = entry["size"]
        proj = nid.create_camera(view["camera_model"], view["intrinsics"], view["distortion_coeffs"])
        min_nz = math.cos(nid.estimate_camera_fov(proj, (W, H)) + 0.5 * math.pi / 180.0)  # (host code: the gate SplatRenderer.draw derives)
        grey = np.clip(np.rint(bag.intensities * 255.0), 0, 255).astype(np.uint8)
        rgba = np.stack([grey, grey, grey, np.full_like(grey, 255)], axis=1)
        want_rgb, want_index = viewer_oracle.draw(view["camera_model"], view["intrinsics"], view["distortion_coeffs"], bag.points, rgba, T, W, H, min_nz, radius=1)
        rgb, depth = dataset.read_png(os.path.join(dst, f"{BAG}_{view['name']}.png"))
        index = pose.read_index_image(os.path.join(dst, f"{BAG}_{view['name']}_indices.png"))  # the sheet is accepted as an index image
        covered = int((want_index >= 0).sum())
        print(f"{name} {view['name']} [{view['spec']}]: {W}x{H}, {covered} pixels covered")
        assert entry["pixels_covered"] == covered and (covered > 500 or view["spec"] == "candidate:5"), "void: next to nothing is drawn"
        assert depth == 8 and np.array_equal(rgb, want_rgb), np.argwhere(rgb != want_rgb)[:8].tolist()
        assert index.dtype == np.int32 and np.array_equal(index, want_index), np.argwhere(index != want_index)[:8].tolist()
        assert np.array_equal(rgb[:, :, 0], rgb[:, :, 1]) and np.array_equal(rgb[:, :, 0], rgb[:, :, 2]) and not rgb[index < 0].any()
    d, dst, _, bag = small["pinhole"]
    assert np.array_equal(dataset.read_png(os.path.join(dst, f"{BAG}_camera.png"))[0], bag.image)


def test_a_pick_returns_what_was_drawn(small):
    for name, d, dst, bag, view, entry in every_sheet(small):
        index = pose.read_index_image(os.path.join(dst, f"{BAG}_{view['name']}_indices.png"))
        vs, us = np.nonzero(index >= 0)
        if len(vs) == 0:  # (candidate:5) nothing to pick: a pick anywhere is refused
            with pytest.raises(igm.PickError, match="nothing is drawn within 2 px"):
                igm.resolve_picks([igm.Pick(BAG, 0.0, 0.0, view["name"], U=320, V=240)], d, dst, [bag], snap_radius=2)
            continue
        vs, us = vs[::97], us[::97]
        picks = [igm.Pick(BAG, 0.0, 0.0, view["name"], U=int(u), V=int(v)) for u, v in zip(us, vs)]
        _, points, records = igm.resolve_picks(picks, d, dst, [bag], snap_radius=2)
        assert len(picks) > 5 and [r["index"] for r in records] == index[vs, us].tolist() and [r["snapped_pixel"] for r in records] == [[int(u), int(v)] for u, v in zip(us, vs)]
        assert np.array_equal(points, bag.points[index[vs, us]])
        # the point's own pixel is trunc(projection), and the splat covers that pixel +- radius: per axis the projection lies in
        # [U - radius, U + radius + 1)
        T = np.array(entry["T_view_lidar"]).reshape(4, 4)
        uv = oracle_lib.project(view["camera_model"], view["intrinsics"], view["distortion_coeffs"], points[:, :3] @ T[:3, :3].T + T[:3, 3])
        off = np.abs(uv - np.stack([us, vs], axis=1)).max()
        print(f"{name} {view['name']}: {len(picks)} picks, largest |projection - pick| per axis {off:.3f} px")
        assert off <= view["radius"] + 1
        # a blank pixel whose right neighbour is covered while the pixels above and to the left are blank snaps to the right
        blank = index < 0
        spot = blank[1:, 1:-1] & ~blank[1:, 2:] & blank[:-1, 1:-1] & blank[1:, :-2]
        V, U = (int(c) for c in np.argwhere(spot)[0] + 1)
        _, _, (record,) = igm.resolve_picks([igm.Pick(BAG, 0.0, 0.0, view["name"], U=U, V=V)], d, dst, [bag], snap_radius=2)
        assert record["snapped_pixel"] == [U + 1, V] and record["index"] == index[V, U + 1] and record["point"] == list(bag.points[index[V, U + 1], :3])
        with pytest.raises(igm.PickError, match="nothing is drawn within 0 px"):
            igm.resolve_picks([igm.Pick(BAG, 0.0, 0.0, view["name"], U=U, V=V)], d, dst, [bag], snap_radius=0)


def test_the_candidates_are_the_viewers_pictures_and_numbers(small, tmp_path):
    d, _, _, bag = small["pinhole"]
    dst = str(tmp_path / "candidates")
    before = open(os.path.join(d, "calib.json"), "rb").read()
    lines = []
    assert igm.run(igm.parse_args([d, "--candidates", "--first_n_bags", "1", "--dst_path", dst]), log=lines.append) == 0
    assert open(os.path.join(d, "calib.json"), "rb").read() == before  # looking changes nothing
    with open(os.path.join(dst, "candidates.json")) as f:
        report = json.load(f)
    entries = report["candidates"]
    assert len(entries) == 24 and sorted(os.listdir(dst)) == sorted(["candidates.json"] + [f"candidate_{k:02d}_{BAG}.png" for k in range(24)])
    proj = nid.create_camera(*dataset.camera_from_calib(dataset.read_calib(d)))
    size = (bag.image.shape[1], bag.image.shape[0])
    scored = 0
    for k, e in enumerate(entries):
        T_lidar_camera = igm.candidate_pose(k, "plumb_bob")
        assert (e["k"], e["facing"], e["roll"], e["repeats"]) == (k, igm.FACINGS[k // 4], k % 4, None) and e["T_lidar_camera"] == igm.pose_to_tum(T_lidar_camera)
        T = np.linalg.inv(T_lidar_camera)
        keep = nid.ViewCulling(proj, size, nid.ViewCullingParams(True), device=0).cull(bag.points, T)
        want = float("nan")
        if len(keep):
            cost = nid.CostCalculatorNID(proj, bag.image, np.ascontiguousarray(bag.points[keep]), np.ascontiguousarray(bag.intensities[keep]), nid.NIDCostParams(16), device=0)
            want = cost.calculate(T)
            cost.close()
            scored += 1
        print(f"candidate {k:2d} {e['facing']} roll {e['roll']}: {len(keep)} points, NID {e['nid'][BAG]!r} (direct {want!r})")
        assert list(e["nid"]) == [BAG] and (e["nid"][BAG] == want or (math.isnan(want) and math.isnan(e["nid"][BAG])))
        assert e["nid_mean"] == e["nid"][BAG] or math.isnan(want)
    assert scored >= 4, "void: fewer than four mountings see a point"
    table = [ln for ln in lines if ln[:2].strip().isdigit()]
    means = [float(ln.split()[-1]) for ln in table]
    assert len(table) == 24 and means == sorted(means, key=lambda v: (math.isnan(v), v)) and any("not claimed" in ln for ln in lines)

    # the overlay of candidate 0 is the viewer's overlay under the same pose
    vdst = str(tmp_path / "viewer")
    os.makedirs(vdst)
    vargs = viewer.parse_args([d, "--view_size", "48x32", "--orbit_deg=10"])
    entry = viewer._bag_views(vargs, proj, bag, "x", igm.candidate_pose(0, "plumb_bob"), vdst, lambda *_: None)
    assert entry["culled"] > 1000 and entry["nid"] == entries[0]["nid"][BAG]
    assert open(os.path.join(vdst, f"{BAG}_x_overlay.png"), "rb").read() == open(os.path.join(dst, f"candidate_00_{BAG}.png"), "rb").read()

    assert igm.main([d, "--choose", "3"]) == 0
    assert dataset.read_calib(d)["results"] == {"init_T_lidar_camera": entries[3]["T_lidar_camera"]}


# ------------------------------------------------------------------------------------------------ end to end
def manual(d, picks, *options):
    """The command on the picks: (T_camera_lidar 4x4 as report.json holds it, report.json, dt, dr against the truth)"""
    argv = [d] + [a for p in picks for a in ("--pick", p)] + list(options)
    assert igm.run(igm.parse_args(argv), log=lambda *_: None) == 0
    with open(os.path.join(d, "manual", "report.json")) as f:
        report = json.load(f)
    T = np.array(report["T_camera_lidar"]).reshape(4, 4)
    assert dataset.read_calib(d)["results"]["init_T_lidar_camera"] == dataset.T_camera_lidar_to_tum(se3.from_matrix(T)) == report["init_T_lidar_camera"]
    dt, dr = se3.delta_trans_rot(fms.scene().T_camera_lidar_true, se3.from_matrix(T))
    return T, report, dt, dr


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    s = fms.scene()
    inten, idx = fms.render_lidar(s, device=0)
    d = str(tmp_path_factory.mktemp("manual_e2e") / "data")
    fms.write_directory(d, s, inten, idx)

    cam, lid, gt = mgs.grid_picks(s, idx)
    picks = mgs.pick_texts(cam, lid)
    assert len(picks) == 24

    # existing code, twice: calibrate from initial_guess_auto on the ground-truth matches of every surviving grid pixel, and from the scene's guess
    fms.write_matches(d, gt)
    fms.initial_guess(d, s)
    x_gt = fms.run_calibrate(d)
    fms.set_manual_guess(d, s.T_camera_lidar_init)
    x_init = fms.run_calibrate(d)
    # the same 24 pairs through initial_guess_auto
    fms.clear_guesses(d)
    fms.write_matches(d, {"kpts0": cam.reshape(-1).tolist(), "kpts1": lid.reshape(-1).tolist(), "matches": list(range(24)), "confidence": [1.0] * 24})
    auto = fms.initial_guess(d, s)
    # and through the command; calibrate then starts from results.init_T_lidar_camera, which takes precedence
    T, report, dt, dr = manual(d, picks)
    x_manual = fms.run_calibrate(d)
    with open(os.path.join(ROOT, "profiles", "find_matches.json")) as f:
        recorded = json.load(f)["end_to_end"]["matcher"]
    return dict(s=s, d=d, idx=idx, picks=picks, cam=cam, lid=lid, auto=auto, T=T, report=report, dt=dt, dr=dr, x_gt=x_gt, x_init=x_init, x_manual=x_manual,
                bound=(recorded["dt_m"], recorded["dr_rad"]))


def test_the_same_pairs_give_the_pose_initial_guess_auto_gives(e2e):
    assert np.array_equal(e2e["T"], e2e["auto"]["T"]), (e2e["T"] - e2e["auto"]["T"]).tolist()
    records = e2e["report"]["picks"]
    assert [r["ransac_inlier"] for r in records] == e2e["auto"]["inliers"].tolist()
    assert [r["snapped_pixel"] for r in records] == e2e["lid"].tolist() and [r["index"] for r in records] == e2e["idx"][e2e["lid"][:, 1], e2e["lid"][:, 0]].tolist()
    assert [r["camera_pixel_stored"] for r in records] == e2e["cam"].astype(float).tolist()


def test_the_manual_guess_lies_within_the_matchers_recorded_guess_error(e2e):
    bound_t, bound_r = e2e["bound"]
    worst = max(r["residual_px"] for r in e2e["report"]["picks"])
    print(f"manual guess from 24 picks: {e2e['dt']:.3e} m, {e2e['dr']:.3e} rad from the truth (bound {bound_t:.3e} m, {bound_r:.3e} rad); {e2e['report']['num_inliers']} inliers, "
          f"worst residual {worst:.2f} px")
    assert (round(bound_t, 4), round(bound_r, 5)) == (2.33e-2, 1.90e-3)  # the recorded figures the bound is
    assert e2e["dt"] <= bound_t and e2e["dr"] <= bound_r


def test_calibrate_from_the_manual_guess_ends_where_it_ends_from_the_scenes_guess(e2e):
    dt0, dr0 = se3.delta_trans_rot(e2e["x_gt"], e2e["x_init"])  # two runs of existing code
    bar_t, bar_r = max(DELTA_T_BAR, 2.0 * dt0), max(DELTA_T_BAR, 2.0 * dr0)
    dt, dr = se3.delta_trans_rot(e2e["x_init"], e2e["x_manual"])
    print(f"existing code: {dt0:.3e} m, {dr0:.3e} rad apart -> bars {bar_t:.3e} m, {bar_r:.3e} rad; manual start: {dt:.3e} m, {dr:.3e} rad")
    assert dt <= bar_t and dr <= bar_r, (dt, bar_t, dr, bar_r)


def test_a_turned_camera_sheet_gives_the_same_pose_bit_for_bit(e2e):
    s = e2e["s"]
    # the inverse of unrotate_points at 90 degrees: stored (x, y) is sheet (H - 1 - y, x)
    turned = np.stack([s.height - 1 - e2e["cam"][:, 1], e2e["cam"][:, 0]], axis=1)
    assert np.array_equal(matching.unrotate_points(turned, 90, s.width, s.height), e2e["cam"])
    T, report, _, _ = manual(e2e["d"], mgs.pick_texts(turned, e2e["lid"]), "--rotate_camera", "90")
    assert report["rotate_camera"] == 90 and np.array_equal(T, e2e["T"])


def test_one_gross_outlier_is_flagged_and_does_not_move_the_pose_out_of_the_bound(e2e):
    k = 7
    cam = mgs.with_outlier(e2e["s"], e2e["cam"], k, 200)
    assert abs(cam[k, 0] - e2e["cam"][k, 0]) == 200 and (np.delete(cam, k, axis=0) == np.delete(e2e["cam"], k, axis=0)).all()
    T, report, dt, dr = manual(e2e["d"], mgs.pick_texts(cam, e2e["lid"]))
    bound_t, bound_r = e2e["bound"]
    flags = [r["ransac_inlier"] for r in report["picks"]]
    print(f"with pick {k} moved 200 px: {dt:.3e} m, {dr:.3e} rad from the truth (bound {bound_t:.3e} m, {bound_r:.3e} rad); residual of the outlier "
          f"{report['picks'][k]['residual_px']:.1f} px, {sum(flags)} inliers")
    assert not flags[k] and report["picks"][k]["residual_px"] > report["ransac_error_thresh"] == 10.0
    assert dt <= bound_t and dr <= bound_r
