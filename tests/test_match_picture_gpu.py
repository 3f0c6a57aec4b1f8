"""The picture options of find_matches and initial_guess_auto end to end on the GPU, on a small directory this test writes itself with
the dataset writers: one bag, a 96 x 64 camera image, 64 x 64 LiDAR intensity and index images, a 2 000-point cloud and calib.json.
Every picture has to equal tests/draw_oracle.py applied to the primitives of the same run, byte for byte, and nothing else in the
directory may depend on the options."""
import json
import os

import numpy as np
import pytest

import draw_oracle as do
from direct_visual_lidar_calibration_amd import dataset, draw, find_matches, initial_guess_auto, nid, pose

pytestmark = pytest.mark.gpu

W, H, LW, LH, N = 96, 64, 64, 64, 2000
INTR = [80.0, 80.0, 48.0, 32.0]


def _texture(w, h, seed):
    """4 x 4 blocks of random gray: corners for FAST"""
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 256, ((h + 3) // 4, (w + 3) // 4), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(blocks, np.ones((4, 4), dtype=np.uint8))[:h, :w])


def _listing(d):
    return {name: open(os.path.join(d, name), "rb").read() for name in sorted(os.listdir(d))}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """The whole sequence, once; every step's directory listing (names and bytes) is kept for the tests."""
    d = str(tmp_path_factory.mktemp("match_picture") / "data")
    camera = _texture(W, H, 1)
    lidar = np.ascontiguousarray(camera[:, 16:16 + LW])  # the LiDAR image shows the camera image's middle: there are matches
    index = (np.arange(LW * LH, dtype=np.int32) % N).reshape(LH, LW)  # every pixel holds a point
    # a pose near the identity, and points that project into the camera image under it
    rng = np.random.default_rng(2)
    T = np.eye(4)
    rv = np.array([0.02, -0.03, 0.01])
    K = np.array([[0.0, -rv[2], rv[1]], [rv[2], 0.0, -rv[0]], [-rv[1], rv[0], 0.0]])
    a = np.linalg.norm(rv)
    T[:3, :3] = np.eye(3) + np.sin(a) / a * K + (1.0 - np.cos(a)) / (a * a) * (K @ K)
    T[:3, 3] = [0.05, -0.02, 0.03]
    z = rng.uniform(2.0, 6.0, N)
    pc = np.stack([(rng.uniform(4.0, W - 4.0, N) - INTR[2]) / INTR[0] * z, (rng.uniform(4.0, H - 4.0, N) - INTR[3]) / INTR[1] * z, z], axis=1)
    points = np.ones((N, 4))
    points[:, :3] = (pc - T[:3, 3]) @ T[:3, :3]  # R^T (pc - t)
    dataset.write_preprocessed(d, ("plumb_bob", INTR, [0.0] * 5), [("bag0", camera, points, rng.uniform(0.0, 1.0, N))], lidar_images={"bag0": (lidar / 255.0, index)})
    out = dict(d=d, camera=camera, lidar=lidar, T_true=T)
    out["before"] = _listing(d)

    assert find_matches.main([d]) == 0
    out["plain"] = _listing(d)
    lines = []
    out["written"] = find_matches.run(find_matches.build_parser().parse_args([d, "--picture"]), log=lines.append)
    out["picture_lines"] = lines
    out["picture"] = _listing(d)
    os.remove(os.path.join(d, "bag0_matches.png"))
    lines = []
    out["written_only"] = find_matches.run(find_matches.build_parser().parse_args([d, "--picture_only"]), log=lines.append)
    out["only_lines"] = lines
    out["only"] = _listing(d)

    # initial_guess_auto from ground-truth matches (keypoint = truncated projection of the pixel's point), 10 of 120 moved 25 px away
    bag = dataset.VisualLiDARData(d, "bag0")
    proj = nid.create_camera("plumb_bob", INTR, [0.0] * 5)
    pix = rng.choice(LW * LH, size=120, replace=False)
    k1 = np.stack([pix % LW, pix // LW], axis=1)
    uv = proj.project(bag.points[index[k1[:, 1], k1[:, 0]], :3] @ T[:3, :3].T + T[:3, 3], device=-1)
    k0 = np.trunc(uv).astype(int)
    k0[:10, 0] = np.where(k0[:10, 0] < W // 2, k0[:10, 0] + 25, k0[:10, 0] - 25)
    with open(os.path.join(d, "bag0_matches.json"), "w") as f:
        json.dump({"kpts0": k0.reshape(-1).tolist(), "kpts1": k1.reshape(-1).tolist(), "matches": list(range(120)), "confidence": [1.0] * 120}, f)
    argv = [d, "--ransac_iterations", "256", "--seed", "4"]
    assert initial_guess_auto.main(argv) == 0
    out["guess_plain"] = _listing(d)
    lines = []
    _, out["T"], _ = initial_guess_auto.run(initial_guess_auto.build_parser().parse_args(argv + ["--picture"]), log=lines.append)
    out["guess_lines"] = lines
    out["guess_picture"] = _listing(d)
    out["proj"], out["corr"] = proj, pose.read_correspondences(d, "bag0", bag.points)
    return out


def _png(data, tmp_path):
    path = str(tmp_path / "picture.png")
    with open(path, "wb") as f:
        f.write(data)
    img, depth = dataset.read_png(path)
    assert depth == 8
    return img


def test_without_the_flag_the_directory_gains_the_json_only(run):
    assert sorted(run["plain"]) == sorted(list(run["before"]) + ["bag0_matches.json"])
    assert all(run["plain"][name] == data for name, data in run["before"].items())


def test_find_matches_picture_equals_the_oracle_on_the_json_of_the_same_run(run, tmp_path):
    d = run["d"]
    assert run["written"] == [os.path.join(d, "bag0_matches.json")]  # the JSON paths only
    assert sorted(run["picture"]) == sorted(list(run["plain"]) + ["bag0_matches.png"])
    assert all(run["picture"][name] == data for name, data in run["plain"].items())  # the same JSON, everything else untouched
    assert run["picture_lines"][0].endswith(f"-> {os.path.join(d, 'bag0_matches.json')}, {os.path.join(d, 'bag0_matches.png')}")
    result = json.loads(run["picture"]["bag0_matches.json"])
    matched = sum(1 for m in result["matches"] if m >= 0)
    print(f"{len(result['kpts0']) // 2} camera keypoints, {len(result['kpts1']) // 2} LiDAR keypoints, {matched} matches")
    assert len(result["kpts0"]) >= 20 and len(result["kpts1"]) >= 20 and matched >= 1, "void: nothing to draw"
    prims = draw.match_primitives(result, (H, W), (LH, LW))
    assert sum(1 for p in prims if p[0] == draw.LINE) == matched
    want = do.draw(run["camera"], run["lidar"], prims)
    got = _png(run["picture"]["bag0_matches.png"], tmp_path)
    assert got.shape == (H, 2 * W, 3) and np.array_equal(got, want)
    assert not np.array_equal(want, do.canvas(run["camera"], run["lidar"]))


def test_picture_only_reproduces_the_png_byte_for_byte(run):
    assert run["written_only"] == []
    assert run["only"] == run["picture"]  # names and bytes: the PNG again, the JSON as it was
    assert "bag0_matches.png" in run["only_lines"][0]


def test_initial_guess_auto_picture_equals_the_oracle_and_leaves_calib_json_alone(run, tmp_path):
    assert sorted(run["guess_picture"]) == sorted(list(run["guess_plain"]) + ["bag0_init_auto.png"])
    assert all(run["guess_picture"][name] == data for name, data in run["guess_plain"].items())  # calib.json among them: byte-identical
    assert b"init_T_lidar_camera_auto" in run["guess_plain"]["calib.json"]
    kp, pts = run["corr"]
    prims, green, red = draw.residual_primitives(run["proj"], kp, pts, run["T"], 10.0)
    print(f"{green} green, {red} red")
    assert green >= 100 and red >= 10 and green + red == 120  # the 10 moved keypoints are 25 px off
    assert any(f"{green} correspondences within 10.0 px (green), {red} beyond (red)" in line and "bag0_init_auto.png" in line for line in run["guess_lines"])
    want = do.draw(run["camera"], None, prims)
    got = _png(run["guess_picture"]["bag0_init_auto.png"], tmp_path)
    assert got.shape == (H, W, 3) and np.array_equal(got, want)
    assert (want == (0, 255, 0)).all(axis=2).any() and (want == (255, 0, 0)).all(axis=2).any()
