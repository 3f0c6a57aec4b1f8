"""The 24 hand picks of the end-to-end check of initial_guess_manual (tests/test_initial_guess_manual_gpu.py,
tools/manual_guess_time.py) on the scene of tests/find_matches_scene.py -- TEST INFRASTRUCTURE ONLY."""
import numpy as np

import find_matches_scene as fms

NUM_PICKS = 24


def grid_picks(s, idx):
    """A 12 x 12 grid of pixels of the 512 x 512 ``lidar`` sheet; the covered ones; of those the ones whose 3D point projects into the
    camera image under the true pose (``fms.ground_truth_matches``: the camera pixel is that projection rounded to integer pixels);
    every (m // 24)-th of the m survivors, the first 24.  Returns ``(camera pixels (24, 2) int, LiDAR pixels (24, 2) int, the
    ground-truth matches of all m survivors)``."""
    grid = np.linspace(40, 471, 12).astype(int)
    candidates = np.array([(x, y) for y in grid for x in grid])
    covered = candidates[idx[candidates[:, 1], candidates[:, 0]] >= 0]
    gt = fms.ground_truth_matches(s, idx, covered)
    m = len(gt["matches"])
    print(f"{int((idx >= 0).sum())} covered pixels, {len(covered)} of {len(candidates)} grid pixels covered, {m} survive the projection")
    assert m >= NUM_PICKS, "void: fewer than 24 picks"
    chosen = list(range(0, m, m // NUM_PICKS))[:NUM_PICKS]
    cam = np.array(gt["kpts0"]).reshape(-1, 2)[chosen]
    lid = covered[np.array(gt["matches"])[chosen]]
    return cam, lid, gt


def pick_texts(cam, lid):
    return [f"{fms.BAG}:{u},{v}:lidar:{U},{V}" for (u, v), (U, V) in zip(np.asarray(cam).tolist(), np.asarray(lid).tolist())]


def with_outlier(s, cam, k=7, shift=200):
    """The camera pixels with pick ``k`` moved ``shift`` px along x, to whichever side stays inside the image"""
    cam = np.array(cam)
    cam[k, 0] += shift if cam[k, 0] + shift < s.width else -shift
    return cam
