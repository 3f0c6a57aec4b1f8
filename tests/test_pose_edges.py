"""The rotation RANSAC (nidreg_estimate_rotation_ransac, csrc/nid_pose_kernels.hpp) at the edges its first tests
(tests/test_pose_gpu.py) leave out: the four camera models compared with no oracle there, degenerate hypotheses, forced ties, and
the sizes at which a tile of correspondences or of hypotheses is exactly full or one over.

Counts are compared with the band of tests/test_pose_gpu.py (pose_oracle.DELTA_PX) given the SAME dictated hypotheses; what the
issue of a degenerate hypothesis or of a tie is, is compared exactly."""
import numpy as np
import pytest

import pose_oracle
from direct_visual_lidar_calibration_amd import nid, pose
from test_pose_gpu import THRESH, band_counts, parity_case

_cases = {}

MODEL_CAMERAS = ["fisheye_1080p", "omnidir_2k", "atan_1080p", "rational_1080p"]
MODEL_N, MODEL_ITERATIONS = 400, 256


def oracle_side(cam, kpts, dirs_camera, dirs_lidar, pairs):
    Rs = np.array([pose_oracle.rotation_svd(dirs_camera[i], dirs_camera[j], dirs_lidar[i], dirs_lidar[j]) for i, j in pairs])
    err = np.array([pose_oracle.errors(cam, kpts, dirs_lidar, R) for R in Rs])
    ill = np.array([min(pose_oracle.angle_between(dirs_camera[i], dirs_camera[j]), pose_oracle.angle_between(dirs_lidar[i], dirs_lidar[j])) < 1e-3 for i, j in pairs])
    return Rs, err, ill


def model_case(camera):
    """400 correspondences (40 % uniform outliers, up to 1 px of noise on the inliers) and 256 dictated hypotheses of one camera
    model, with the oracle's side of the comparison"""
    if camera not in _cases:
        cam, kpts, pts, _ = pose_oracle.make_correspondences_without_image(camera, MODEL_N, 0.4, seed=21, noise_px=1.0)
        proj = nid.create_camera(*cam)
        dirs_camera = pose.estimate_directions(proj, kpts)
        dirs_lidar = pose_oracle.unit(pts)
        rng = np.random.default_rng(22)
        pairs = np.array([rng.choice(MODEL_N, size=2, replace=False) for _ in range(MODEL_ITERATIONS)], dtype=np.int32)
        Rs, err, ill = oracle_side(cam, kpts, dirs_camera, dirs_lidar, pairs)
        _cases[camera] = dict(proj=proj, cam=cam, kpts=kpts, dirs_camera=dirs_camera, dirs_lidar=dirs_lidar, pairs=pairs, Rs=Rs, err=err, ill=ill)
    return _cases[camera]


# ---- B1: the four remaining camera models ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("camera", MODEL_CAMERAS)
def test_the_oracle_alone_leaves_the_band_almost_empty_on_the_remaining_models(camera):
    """(CPU) The caps of test_pose_gpu.test_the_oracle_alone_leaves_the_band_almost_empty on the smaller scene of each model: under
    0.1 % of the pairs inside the band, at most 1 % ill-conditioned hypotheses; and some hypothesis fits a tenth of the scene."""
    c = model_case(camera)
    with np.errstate(invalid="ignore"):
        inside = (np.abs(c["err"] - THRESH) <= pose_oracle.DELTA_PX).sum()
    lo, _ = band_counts(c["err"])
    print(f"{camera}: {int(inside)} of {c['err'].size} pairs inside the band, {int(c['ill'].sum())} ill-conditioned hypotheses, best count {int(lo.max())}")
    assert inside < 1e-3 * c["err"].size
    assert c["ill"].sum() <= 0.01 * len(c["pairs"])
    assert lo.max() > 0.1 * MODEL_N  # (two correspondences fit any hypothesis; the comparison on the device is not one of zeros)


@pytest.mark.gpu
@pytest.mark.parametrize("camera", MODEL_CAMERAS)
def test_hypothesis_parity_winner_and_flags_on_the_remaining_models(camera):
    """The assertions of test_pose_gpu.test_hypothesis_parity_winner_and_flags for the instantiations of k_ransac_score and
    k_ransac_flags it does not reach.  (400 correspondences: one tile of kPoseTileC; 256 hypotheses: 16 workgroups of kPoseTileH.)"""
    c = model_case(camera)
    R, best_k, best_n, flags, counts = pose.ransac_rotation(c["proj"], c["kpts"], c["dirs_camera"], c["dirs_lidar"], MODEL_ITERATIONS, THRESH, device=0, pairs=c["pairs"])
    lo, hi = band_counts(c["err"])
    with np.errstate(invalid="ignore"):
        inside = (np.abs(c["err"] - THRESH) <= pose_oracle.DELTA_PX).sum()
    print(f"{camera}: counts {counts.min()}..{counts.max()}, {int((counts != lo).sum())} differ from the lower band count, {int(inside)} pairs inside the band")
    assert inside < 1e-3 * c["err"].size and c["ill"].sum() <= 0.01 * len(c["pairs"])
    assert ((lo <= counts) & (counts <= hi)).all(), np.flatnonzero((counts < lo) | (counts > hi))[:10]
    assert best_k == int(np.flatnonzero(counts == counts.max())[0]) and best_n == int(counts[best_k])
    assert not c["ill"][best_k]
    dR = np.linalg.norm(R - c["Rs"][best_k])
    print(f"{camera}: winner {best_k} with {best_n} inliers, |R - R_numpy|_F {dR:.3e}")
    assert dR <= 1e-9
    assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.allclose(R @ R.T, np.eye(3), atol=1e-12)
    e = c["err"][best_k]
    with np.errstate(invalid="ignore"):
        decided = ~(np.abs(e - THRESH) <= pose_oracle.DELTA_PX)
        assert np.array_equal(flags[decided], (e < THRESH)[decided])
    assert best_n == int(flags.sum())


# ---- B2: degenerate hypotheses -------------------------------------------------------------------------------------------------------

# position -> kind: first and second wave of workgroup 0 (kPoseTileH = 16 hypotheses per workgroup, four per wave), the first of
# workgroup 1, both sides of the boundary between two blocks of k_ransac_hypotheses / k_ransac_best (kPoseThreads = 256), the last
DEGENERATE_AT = {0: "same", 1: "copy", 4: "opposite", 16: "copy", 17: "same", 255: "opposite", 256: "same", 257: "copy", 1022: "opposite", 1023: "copy"}


def degenerate_case():
    """The parity case of test_pose_gpu (pinhole, 1500 correspondences, 1024 hypotheses) with two rows appended: row 1500 an exact
    copy of correspondence 3 (keypoint, camera bearing, LiDAR bearing), row 1501 the keypoint and LiDAR bearing of correspondence
    6 with the NEGATED camera bearing of correspondence 5: in the pair (5, 1501) only the sum of the camera bearings vanishes
    (a+ = 0 in two_vector_rotation; a-, b+ and b- are ordinary).  Neither row is named by an ordinary hypothesis; the scores of
    the ordinary ones gain the two columns."""
    if "degenerate" not in _cases:
        c = parity_case("pinhole_vga")
        n = len(c["kpts"])
        src = np.array([3, 6])
        kpts = np.concatenate([c["kpts"], c["kpts"][src]])
        dirs_lidar = np.concatenate([c["dirs_lidar"], c["dirs_lidar"][src]])
        dirs_camera = np.concatenate([c["dirs_camera"], c["dirs_camera"][src]])
        dirs_camera[n + 1] = -dirs_camera[5]
        kinds = {"same": (3, 3), "copy": (3, n), "opposite": (5, n + 1)}
        pairs = c["pairs"].copy()
        for k, kind in DEGENERATE_AT.items():
            pairs[k] = kinds[kind]
        err = np.concatenate([c["err"], c["err"][:, src]], axis=1)  # (the score reads keypoint and LiDAR bearing only)
        _cases["degenerate"] = dict(proj=c["proj"], kpts=kpts, dirs_camera=dirs_camera, dirs_lidar=dirs_lidar, pairs=pairs, err=err, kinds=kinds, n=n)
    return _cases["degenerate"]


def test_the_degenerate_pairs_are_exactly_degenerate():
    """(CPU) The dictated pairs name one index twice, or two rows whose bearings are bit-identical, or two camera bearings whose
    sum is exactly zero; every ordinary hypothesis keeps its pair, and the best ordinary one is far ahead of 0 inliers."""
    d = degenerate_case()
    dc, dl, n = d["dirs_camera"], d["dirs_lidar"], d["n"]
    assert np.array_equal(dc[3], dc[n]) and np.array_equal(dl[3], dl[n]) and np.array_equal(d["kpts"][3], d["kpts"][n])
    assert np.array_equal(dc[5] + dc[n + 1], np.zeros(3))
    # ... and nothing else of that pair is degenerate: the LiDAR bearings are those of two different correspondences, neither
    # close nor opposite, so a- = 2 a_5, b+ and b- are ordinary and the NaN can only come from a+ = 0
    assert np.array_equal(dl[6], dl[n + 1]) and np.array_equal(d["kpts"][6], d["kpts"][n + 1])
    angle = pose_oracle.angle_between(dl[5], dl[n + 1])
    print(f"angle between the LiDAR bearings of the opposite pair {angle:.3f} rad")
    assert 1e-2 < angle < np.pi - 1e-2
    ordinary = np.setdiff1d(np.arange(1024), list(DEGENERATE_AT))
    assert np.array_equal(d["pairs"][ordinary], parity_case("pinhole_vga")["pairs"][ordinary]) and d["pairs"][ordinary].max() < n
    lo, _ = band_counts(d["err"][ordinary])
    assert lo.max() > 500


@pytest.mark.gpu
def test_degenerate_hypotheses_count_no_inlier_among_ordinary_ones():
    """(i, i), (i, exact copy of i) and a pair of exactly opposite camera bearings, at hypotheses 0, 1, 4, 16, 17 (waves and
    workgroups of k_ransac_score: kPoseTileH = 16 per workgroup, four per wave), 255, 256, 257 (blocks of kPoseThreads = 256) and the
    last two: 0 inliers each without a band, every ordinary hypothesis in band, an ordinary winner."""
    d = degenerate_case()
    R, best_k, best_n, flags, counts = pose.ransac_rotation(d["proj"], d["kpts"], d["dirs_camera"], d["dirs_lidar"], 1024, THRESH, device=0, pairs=d["pairs"])
    deg = np.array(sorted(DEGENERATE_AT))
    assert counts[deg].tolist() == [0] * len(deg)
    ordinary = np.setdiff1d(np.arange(1024), deg)
    lo, hi = band_counts(d["err"])
    assert ((lo <= counts) & (counts <= hi))[ordinary].all(), ordinary[((counts < lo) | (counts > hi))[ordinary]][:10]
    assert best_k in ordinary and best_k == int(np.flatnonzero(counts == counts.max())[0]) and best_n == int(counts[best_k]) == int(flags.sum()) > 0
    assert np.isfinite(R).all() and np.linalg.norm(R - parity_case("pinhole_vga")["Rs"][best_k]) <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("iterations, first", [(1, "opposite"), (16, "same"), (300, "copy"), (300, "opposite")])
def test_only_degenerate_hypotheses_leave_iteration_0_with_no_inlier(iterations, first):
    """1, 16 (one full workgroup of kPoseTileH) and 300 (two blocks of kPoseThreads = 256) hypotheses, all degenerate, the three
    kinds in turn starting with ``first`` (the kind of iteration 0, whose rotation is handed back): the winner is iteration 0 with
    0 inliers, no flag is set and the rotation is not finite -- the state PoseEstimation.estimate_rotation_ransac refuses
    (tests/test_pose_host.py)."""
    d = degenerate_case()
    names = list(d["kinds"])
    kinds = [d["kinds"][names[(names.index(first) + k) % 3]] for k in range(3)]
    pairs = np.array([kinds[k % 3] for k in range(iterations)], dtype=np.int32)
    R, best_k, best_n, flags, counts = pose.ransac_rotation(d["proj"], d["kpts"], d["dirs_camera"], d["dirs_lidar"], iterations, THRESH, device=0, pairs=pairs)
    assert (best_k, best_n) == (0, 0) and not counts.any() and not flags.any() and counts.shape == (iterations,)
    assert not np.isfinite(R).any()
    pe = pose.PoseEstimation(pose.PoseEstimationParams(ransac_iterations=iterations))
    pts = np.concatenate([d["dirs_lidar"], np.ones((len(d["kpts"]), 1))], axis=1)  # points at unit range: their bearings are dirs_lidar again
    with pytest.raises(ValueError, match="no hypothesis with an inlier"):
        pe.estimate_rotation_ransac(d["proj"], d["kpts"], pts, device=0, pairs=np.tile([[3, 3]], (iterations, 1)))


# ---- B3: forced ties -------------------------------------------------------------------------------------------------------------------


def tie_case():
    """The hypothesis with the most inliers of the parity case, and 600 of the others"""
    c = parity_case("pinhole_vga")
    lo, hi = band_counts(c["err"])
    w = int(np.argmax(lo))
    others = np.delete(np.arange(1024), w)[:600]
    return c, w, others, lo, hi


def test_the_winning_pair_of_the_parity_case_wins_by_more_than_the_band():
    """(CPU) Its lower band count exceeds the upper band count of each of the 600 other hypotheses: wherever its copies stand,
    one of them wins, and which one is the tie rule alone."""
    c, w, others, lo, hi = tie_case()
    assert not c["ill"][w] and lo[w] > hi[others].max()
    assert not (c["pairs"][others] == c["pairs"][w]).all(axis=1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("copies, winner", [((300, 7, 599), 7), ((256, 257), 256), ((255, 256), 255), ((599,), 599)])
def test_ties_go_to_the_lowest_iteration_across_waves_and_blocks(copies, winner):
    """600 hypotheses (three blocks of kPoseThreads = 256 in k_ransac_best, 38 workgroups of kPoseTileH = 16 in k_ransac_score) with
    the winning pair dictated at several iterations: bit-identical counts there, and the packed 64-bit atomicMax key hands the tie
    to the lowest of them -- across blocks (300, 7, 599), in adjacent blocks (256, 257; 255, 256)."""
    c, w, others, lo, hi = tie_case()
    pairs = c["pairs"][others].copy()
    for k in copies:
        pairs[k] = c["pairs"][w]
    R, best_k, best_n, flags, counts = pose.ransac_rotation(c["proj"], c["kpts"], c["dirs_camera"], c["dirs_lidar"], 600, THRESH, device=0, pairs=pairs)
    assert len(set(counts[list(copies)].tolist())) == 1 and lo[w] <= counts[winner] <= hi[w]
    assert best_k == winner and best_n == int(counts[winner]) == int(flags.sum())
    assert (np.delete(counts, list(copies)) < counts[winner]).all()
    assert np.linalg.norm(R - c["Rs"][w]) <= 1e-9


# ---- B4: tile edges ----------------------------------------------------------------------------------------------------------------------


def tile_scene():
    if "tiles" not in _cases:
        scene, kpts, pts, _ = pose_oracle.make_correspondences("pinhole_vga", 2048, 0.4, seed=23, noise_px=1.0)
        proj = nid.create_camera(scene.model, scene.intrinsics, scene.distortion)
        _cases["tiles"] = dict(proj=proj, cam=(scene.model, scene.intrinsics, scene.distortion), kpts=kpts, dirs_camera=pose.estimate_directions(proj, kpts), dirs_lidar=pose_oracle.unit(pts))
    return _cases["tiles"]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1024, 1025, 2048])
def test_shapes_at_the_edges_of_the_correspondence_and_hypothesis_tiles(n):
    """n in {1024 (the last size with one tile of kPoseTileC = 1024: plain store), 1025 (a second tile of ONE correspondence: atomic
    path), 2048 (two full tiles)} x iterations in {16, 17 (kPoseTileH = 16 per workgroup), 256, 257 (kPoseThreads = 256 per block of
    k_ransac_hypotheses / k_ransac_best)}: the rules of test_shapes_single_tile_multi_tile_and_partial_tiles, the banded count
    on at most 64 hypotheses."""
    t = tile_scene()
    kp, dc, dl = t["kpts"][:n], t["dirs_camera"][:n], t["dirs_lidar"][:n]
    rng = np.random.default_rng(n)
    for iterations in (16, 17, 256, 257):
        seed = 1000 * n + iterations
        R, best_k, best_n, flags, counts = pose.ransac_rotation(t["proj"], kp, dc, dl, iterations, THRESH, device=0, seed=seed)
        pairs = pose.sample_pairs(seed, n, iterations)
        assert counts.shape == (iterations,) and flags.shape == (n,)
        assert best_k == int(np.flatnonzero(counts == counts.max())[0]) and best_n == int(counts[best_k]) == int(flags.sum())
        sub = np.unique(np.concatenate([[0, 15, iterations - 1, best_k], rng.choice(iterations, size=min(iterations, 60), replace=False)]))
        for k in sub:
            i, j = pairs[k]
            err = pose_oracle.errors(t["cam"], kp, dl, pose_oracle.rotation_svd(dc[i], dc[j], dl[i], dl[j]))
            lo, hi = pose_oracle.count_band(err, THRESH)
            assert lo <= counts[k] <= hi, (n, iterations, int(k), lo, int(counts[k]), hi)


def second_tile_element_errors():
    """the oracle's error of correspondence 1024 under each of 257 hypotheses dictated among the first 1024"""
    if "element" not in _cases:
        t = tile_scene()
        pairs = pose.sample_pairs(77, 1024, 257)
        dc, dl = t["dirs_camera"], t["dirs_lidar"]
        e = np.array([pose_oracle.errors(t["cam"], t["kpts"][1024:1025], dl[1024:1025], pose_oracle.rotation_svd(dc[i], dc[j], dl[i], dl[j]))[0] for i, j in pairs])
        _cases["element"] = (pairs, e)
    return _cases["element"]


def test_correspondence_1024_is_decided_both_ways_outside_the_band():
    """(CPU) Under the 257 dictated hypotheses correspondence 1024 is an inlier of some and an outlier of others, and at most two of
    its errors lie inside the band."""
    pairs, e = second_tile_element_errors()
    assert pairs.max() < 1024
    with np.errstate(invalid="ignore"):
        decided = ~(np.abs(e - THRESH) <= pose_oracle.DELTA_PX)
        inl = int((e < THRESH)[decided].sum())
    print(f"{int(decided.sum())} of 257 decided, {inl} of them inliers")
    assert decided.sum() >= 255 and 0 < inl < decided.sum()


@pytest.mark.gpu
def test_the_single_element_of_a_second_tile_is_counted_once():
    """n = 1024 against n = 1025 (kPoseTileC = 1024) on the same first 1024 correspondences and the same 257 dictated pairs, all
    below 1024: counts(1025) - counts(1024) is the decision for correspondence 1024 alone -- 0 or 1, and the oracle's wherever
    that error is outside the band."""
    t = tile_scene()
    iterations = 257
    pairs, e = second_tile_element_errors()
    out = {}
    for n in (1024, 1025):
        out[n] = pose.ransac_rotation(t["proj"], t["kpts"][:n], t["dirs_camera"][:n], t["dirs_lidar"][:n], iterations, THRESH, device=0, pairs=pairs)
    diff = out[1025][4] - out[1024][4]
    assert np.isin(diff, (0, 1)).all()
    with np.errstate(invalid="ignore"):
        decided = ~(np.abs(e - THRESH) <= pose_oracle.DELTA_PX)
        assert decided.sum() >= iterations - 2 and np.array_equal(diff[decided], (e < THRESH)[decided].astype(diff.dtype))
    print(f"correspondence 1024 is an inlier of {int(diff.sum())} of {iterations} hypotheses")
    assert 0 < diff.sum() < iterations
