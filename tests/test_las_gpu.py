"""GPU tests of the LAS map route (nidreg_integrator_insert_las, k_vox_decode_las of csrc/nid_las_kernels.hpp) and of the map options
of preprocess_map.  The bar is BIT FOR BIT: the integrator fed the raw records must hold the records, in the order, that a second
integrator holds after ``nidreg_integrator_insert`` of the doubles of ``las_oracle.decode`` with the filtered points left out; the
winners' sequence numbers are the RAW indices of the points (a filtered point takes a number).  Shapes are the smallest at which the
kernel can go wrong: counts around one and two tiles of 256 records, record lengths that are no multiple of anything, one record
length past the LDS staging limit of 128 bytes."""
import json
import os

import numpy as np
import pytest

import las_oracle as lo
from direct_visual_lidar_calibration_amd import dataset, preprocess, preprocess_map, synth

pytestmark = pytest.mark.gpu

RES = 0.5  # with coordinates within +-3 m: about 1700 voxels, so 515 points share voxels and "the last one wins" is exercised
SCALE, OFFSET, ORIGIN = (0.001, 1e-4, 0.01), (0.25, -0.5, 0.125), (0.0, 0.0, 0.0)
COUNTS = (0, 1, 255, 256, 257, 2 * 256 + 3)


def make_records(point_format, n, extra=0, seed=0, classes=(0, 1, 2), withheld_rate=0.0):
    rng = np.random.default_rng(1000 * point_format + 10 * extra + seed)
    X, Y, Z = rng.integers(-3000, 3000, n), rng.integers(-30000, 30000, n), rng.integers(-300, 300, n)
    rgb = rng.integers(0, 65536, (n, 3)) if point_format in lo.RGB_OFFSET else None
    return lo.pack_records(point_format, X, Y, Z, rng.integers(0, 65536, n), rng.choice(np.asarray(classes), n), rng.random(n) < withheld_rate, rgb, extra, rng)


def check(rec, point_format, scale=SCALE, offset=OFFSET, origin=ORIGIN, res=RES, **options):
    """the records through the kernel == the oracle's doubles through nidreg_integrator_insert; returns (records, raw winners, keep)"""
    n, step = rec.shape
    xyz, inten, keep = lo.decode(rec, point_format, scale, offset, origin, **options)
    a, b = preprocess.StaticPointCloudIntegrator(res, 0.0), preprocess.StaticPointCloudIntegrator(res, 0.0)
    try:
        skipped = a.insert_las(rec.reshape(-1), step, point_format, scale, offset, origin, **options)
        b.insert_points(xyz[keep], inten[keep])
        got, want = a.get_records(), b.get_records()
        assert skipped == int((~keep).sum()), (skipped, int((~keep).sum()))
        assert a.info()["offered"] == n and b.info()["offered"] == int(keep.sum())
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        raw = np.flatnonzero(keep)[b.last_seq]  # the winners' raw indices: the same order, numbers that differ only where points were skipped
        assert np.array_equal(a.last_seq, raw)
        return got, raw, keep
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("point_format,extra", [(0, 0), (2, 0), (3, 0), (10, 0), (10, 3)])
def test_every_count_at_every_record_length(point_format, extra):
    for n in COUNTS:
        rec = make_records(point_format, n, extra, seed=n, withheld_rate=0.1 if n > 1 else 0.0)
        assert rec.shape == (n, {(0, 0): 20, (2, 0): 26, (3, 0): 34, (10, 0): 67, (10, 3): 70}[(point_format, extra)])
        got, raw, keep = check(rec, point_format)
        if n == 515:
            assert 100 < len(got) < keep.sum()  # voxels shared by several points


def test_records_longer_than_the_staging_limit_are_read_from_global_memory():
    for n in (1, 257, 515):
        rec = make_records(6, n, extra=120, seed=n, classes=(1, 7), withheld_rate=0.2)
        assert rec.shape[1] == 150
        check(rec, 6, exclude_classes=(7,))
    check(make_records(6, 300, extra=98), 6)  # 128 bytes: the last staged length


def test_extreme_coordinates_keep_their_sign():
    ints = np.array([-(2**31), -1, 0, 2**31 - 1, -(2**31) + 1, 1, 255, 256, -256, 65536, -65537, 2**24, -(2**24) - 1], dtype=np.int64)
    X, Y, Z = ints, np.roll(ints, 1), np.roll(ints, 2)
    for point_format in (0, 6):
        rec = lo.pack_records(point_format, X, Y, Z, np.arange(len(ints)) * 5000)
        # at 4 m voxels the key holds +-4194 km: +-2147483.648 m fits
        got, raw, _ = check(rec, point_format, scale=(0.001,) * 3, offset=(0.0,) * 3, res=4.0)
        assert np.array_equal(raw, np.arange(len(ints)))  # all in voxels of their own
        assert got[0, 0] == np.float32(-2147483.648) and got[3, 0] == np.float32(2147483.647) and got[1, 0] == np.float32(-0.001) and got[2, 0] == 0.0
        check(rec, point_format, scale=(0.001, 1e-4, 0.002), offset=(1000.5, -2000.25, 0.0), origin=(1000.0, -2000.0, 3.0), res=8.0)


def test_a_georeferenced_map_is_recentred_in_fp64_and_refused_without_its_origin():
    n = 515
    rng = np.random.default_rng(8)
    X, Y, Z = rng.integers(-90000, 90000, n), rng.integers(-900000, 900000, n), rng.integers(-2000, 2000, n)
    rec = lo.pack_records(3, X, Y, Z, rng.integers(0, 65536, n), rgb=rng.integers(0, 65536, (n, 3)), rng=rng)
    scale, offset, origin = (0.001, 1e-4, 0.01), (500000.37, 4000000.91, 123.456), (500000.0, 4000000.0, 100.0)
    got, raw, keep = check(rec, 3, scale, offset, origin, res=0.002)  # inside the key limit of +-2097 m at 2 mm
    assert keep.all() and np.array_equal(raw, np.arange(n))  # 2 mm voxels: every point in its own
    xyz, _, _ = lo.decode(rec, 3, scale, offset, origin)
    assert np.array_equal(got[:, :3], xyz.astype(np.float32)) and np.abs(xyz).max() < 200.0
    # narrowing the georeferenced coordinate itself would have cost up to 25 cm: the recentred one is good to 8 um
    absolute, _, _ = lo.decode(rec, 3, scale, offset, (0.0, 0.0, 0.0))
    assert np.abs(absolute.astype(np.float32).astype(np.float64) - absolute).max() > 0.1 and np.abs(got[:, :3].astype(np.float64) - xyz).max() < 8e-6
    integ = preprocess.StaticPointCloudIntegrator(0.002, 0.0)
    try:
        with pytest.raises(ValueError, match="outside the packed-key limit"):
            integ.insert_las(rec.reshape(-1), 34, 3, scale, offset, (0.0, 0.0, 0.0))
        assert integ.info()["offered"] == 0 and integ.size() == 0  # refused as a whole
    finally:
        integ.close()


def test_class_masks_and_the_withheld_bit_in_both_layouts():
    n = 515
    for point_format, classes, excluded in ((1, (0, 7, 31, 2), (7, 31)), (1, (0, 7, 31, 2), (0,)), (3, (0, 7, 31), (0, 7, 31)), (6, (7, 18, 255, 1), (7, 18, 255)), (8, (7, 18, 255, 64, 128), (255, 64))):
        for keep_withheld in (False, True):
            rec = make_records(point_format, n, seed=3, classes=classes, withheld_rate=0.25)
            if point_format <= 5:
                assert (rec[:, 15] & 0x60).any() and (rec[:, 15] & 0x80).any()  # synthetic / key-point bits set (and ignored), withheld points present
            else:
                assert (rec[:, 15] & 0x04).any() and (rec[:, 15] & 0xFB).any()
            _, _, keep = check(rec, point_format, exclude_classes=excluded, keep_withheld=keep_withheld)
            assert 0 < keep.sum() < n or set(classes) == set(excluded)
            check(rec, point_format, keep_withheld=keep_withheld)  # no mask: only the flag filters
    # in formats 6 - 10 bit 7 of byte 15 is the edge-of-flight-line flag, in formats 0 - 5 bit 2 belongs to the class: neither is the withheld bit
    rec = lo.pack_records(6, [100, 900], [0, 0], [0, 0], [1, 2])
    rec[:, 15] = 0x80
    assert check(rec, 6)[2].all()
    rec = lo.pack_records(0, [100, 900], [0, 0], [0, 0], [1, 2], classification=[4, 4], flags=[0, 0])
    assert check(rec, 0)[2].all() and not check(rec, 0, exclude_classes=(4,))[2].any()


def test_a_filtered_point_that_would_have_won_its_voxel_leaves_the_previous_winner():
    # three points in one voxel; the last is class 7 / withheld: the second stays
    for point_format in (0, 7):
        rgb = [[1, 2, 3]] * 3 if point_format == 7 else None
        rec = lo.pack_records(point_format, [10, 20, 30], [0, 0, 0], [0, 0, 0], [111, 222, 333], classification=[1, 1, 7], rgb=rgb)
        got, raw, _ = check(rec, point_format, exclude_classes=(7,))
        assert raw.tolist() == [1] and got[0, 3] == 222.0
        got, raw, _ = check(rec, point_format)
        assert raw.tolist() == [2] and got[0, 3] == 333.0
        rec = lo.pack_records(point_format, [10, 20, 30], [0, 0, 0], [0, 0, 0], [111, 222, 333], withheld=[False, False, True], rgb=rgb)
        assert check(rec, point_format)[1].tolist() == [1] and check(rec, point_format, keep_withheld=True)[1].tolist() == [2]


@pytest.mark.parametrize("point_format", [2, 3, 5, 7, 8, 10])
def test_rgb_intensity_is_the_exact_integer_luma(point_format):
    values = np.array([0, 255, 256, 65535])
    rgb = np.stack(np.meshgrid(values, values, values, indexing="ij"), axis=-1).reshape(-1, 3)  # all 64 combinations
    n = len(rgb)
    rec = lo.pack_records(point_format, np.arange(n) * 1000, np.zeros(n), np.zeros(n), np.full(n, 9), rgb=rgb)
    got, raw, _ = check(rec, point_format, scale=(0.001,) * 3, offset=(0.0,) * 3, intensity="rgb")
    assert np.array_equal(raw, np.arange(n))
    assert np.array_equal(got[:, 3].astype(np.int64), 77 * rgb[:, 0] + 150 * rgb[:, 1] + 29 * rgb[:, 2]) and got[:, 3].max() == 256.0 * 65535.0
    assert (check(rec, point_format, scale=(0.001,) * 3, offset=(0.0,) * 3)[0][:, 3] == 9.0).all()  # the default reads the intensity field
    check(make_records(point_format, 515, seed=5), point_format, intensity="rgb")
    integ = preprocess.StaticPointCloudIntegrator(RES, 0.0)
    try:
        with pytest.raises(ValueError, match="rgb intensity asked of point format 1"):
            integ.insert_las(make_records(1, 3).reshape(-1), 28, 1, SCALE, OFFSET, intensity="rgb")
    finally:
        integ.close()


def test_chunked_reading_gives_the_same_records_and_offered(tmp_path):
    rec = make_records(3, 515, extra=1, seed=9, classes=(1, 7), withheld_rate=0.1)
    path = str(tmp_path / "m.las")
    lo.write_las(path, 3, rec, SCALE, OFFSET, minor=4, vlr_bytes=77)
    header = dataset.read_las_header(path)
    out = []
    for chunk_points in (100, 1 << 23):
        integ = preprocess.StaticPointCloudIntegrator(RES, 0.0)
        try:
            skipped = preprocess_map.integrate_las(integ, path, header, ORIGIN, "intensity", (7,), False, chunk_points)
            out.append((skipped, integ.get_records(), integ.last_seq, integ.info()))
        finally:
            integ.close()
    (s0, r0, q0, i0), (s1, r1, q1, i1) = out
    assert s0 == s1 > 0 and np.array_equal(r0.view(np.uint32), r1.view(np.uint32)) and np.array_equal(q0, q1) and i0 == i1 and i0["offered"] == 515
    lines = []
    a = preprocess_map.load_lidar_points(path, RES, log=lines.append, las_exclude_classes=(7,), chunk_points=100)
    b = preprocess_map.load_lidar_points(path, RES, log=lambda m: None, las_exclude_classes=(7,))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].shape == (r0.shape[0], 4)
    assert lines == ["map_origin=0,0,0", f"map_points=515 skipped={s0} filtered={r0.shape[0]}"]


def test_equal_intensities_are_reported_with_the_option_that_helps(tmp_path):
    rec = make_records(2, 40, seed=2)
    rec[:, 12:14] = 0
    path = str(tmp_path / "flat.las")
    lo.write_las(path, 2, rec, SCALE, OFFSET)
    lines = []
    preprocess_map.load_lidar_points(path, RES, log=lines.append)
    assert len(lines) == 3 and "--map_intensity rgb" in lines[2]
    lines = []
    preprocess_map.load_lidar_points(path, RES, log=lines.append, map_intensity="rgb")
    assert len(lines) == 2


# ---- end to end ------------------------------------------------------------------------------------------------------------------
E2E_RES = 0.05
FILES = ("000000.ply", "000000_lidar_intensities.png", "000000_lidar_indices.png", "000000.png")


@pytest.fixture(scope="module")
def scene_files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("las_e2e")
    scene = synth.make_scene("pinhole_vga", num_points=20000, seed=30)
    image = str(tmp / "image.png")
    dataset.write_png_gray(image, (scene.image_u8 // 2 + 40).astype(np.uint8))
    intr = ",".join(repr(float(v)) for v in scene.intrinsics)
    dist = ",".join(repr(float(v)) for v in scene.distortion)
    argv = ["--image_path", image, "--camera_model", scene.model, "--camera_intrinsics", intr, "--camera_distortion_coeffs", dist, "--voxel_resolution", str(E2E_RES)]
    return tmp, scene, argv


def read_dir(path):
    files = {name: open(os.path.join(path, name), "rb").read() for name in FILES}
    with open(os.path.join(path, "calib.json")) as f:
        calib = json.load(f)
    return files, calib


def test_preprocess_map_of_a_georeferenced_las_equals_the_recentred_float64_ply(scene_files, capsys):
    tmp, scene, argv = scene_files
    pts = np.asarray(scene.points)[:, :3]
    scale, shift = (0.001, 0.001, 0.001), (500000.25, 4000000.5, 310.125)  # a UTM-like datum: the photograph was taken at `shift`
    ints = np.rint(pts / np.asarray(scale)).astype(np.int64)
    inten = np.rint(np.asarray(scene.intensities) / max(float(np.max(scene.intensities)), 1e-9) * 65535.0).astype(np.int64)
    rec = lo.pack_records(1, ints[:, 0], ints[:, 1], ints[:, 2], inten)
    rec[:, 15] &= 0x7F  # nothing withheld
    las, ply = str(tmp / "map.las"), str(tmp / "map64.ply")
    lo.write_las(las, 1, rec, scale, shift, minor=2)
    xyz, w, keep = lo.decode(rec, 1, scale, shift, shift)
    assert keep.all() and np.abs(xyz - pts).max() < 1e-3
    body = np.empty(len(xyz), dtype=[("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("intensity", "<u2")])
    body["x"], body["y"], body["z"], body["intensity"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], w
    with open(ply, "wb") as f:
        f.write(f"ply\nformat binary_little_endian 1.0\nelement vertex {len(xyz)}\nproperty double x\nproperty double y\nproperty double z\nproperty ushort intensity\nend_header\n".encode())
        f.write(body.tobytes())
    origin = ",".join(repr(v) for v in shift)
    dst_las, dst_ply, dst_auto = str(tmp / "d_las"), str(tmp / "d_ply"), str(tmp / "d_auto")
    assert preprocess_map.main(argv + ["--map_path", las, "--dst_path", dst_las, "--map_origin", origin]) == 0
    out = capsys.readouterr().out
    assert "map_origin=500000.25,4000000.5,310.125" in out and f"map_points={len(xyz)} skipped=0 filtered=" in out
    assert preprocess_map.main(argv + ["--map_path", ply, "--dst_path", dst_ply]) == 0
    files_las, calib_las = read_dir(dst_las)
    files_ply, calib_ply = read_dir(dst_ply)
    for name in FILES:
        assert files_las[name] == files_ply[name], name
    assert calib_las["meta"].pop("map_origin") == list(shift) and "map_origin" not in calib_ply["meta"]
    assert calib_las["meta"].pop("data_path") == las and calib_ply["meta"].pop("data_path") == ply
    assert calib_las == calib_ply
    # auto: the header bounds leave +-1024 m, so the origin is the floor of their middle -- a whole number of metres
    assert preprocess_map.main(argv + ["--map_path", las, "--dst_path", dst_auto]) == 0
    _, calib_auto = read_dir(dst_auto)
    mid = [float(np.floor((lo_ + hi_) / 2.0)) for lo_, hi_ in zip(*(dataset.read_las_header(las)[k] for k in ("min", "max")))]
    assert calib_auto["meta"]["map_origin"] == mid and abs(mid[0] - 500000.0) < 200.0
    # an explicit origin with a PLY map: the float64 route, the origin recorded
    dst_shift = str(tmp / "d_shift")
    assert preprocess_map.main(argv + ["--map_path", ply, "--dst_path", dst_shift, "--map_origin", "-0.5,0.25,0"]) == 0
    _, calib_shift = read_dir(dst_shift)
    assert calib_shift["meta"]["map_origin"] == [-0.5, 0.25, 0.0]
    got, _ = dataset.read_ply(os.path.join(dst_shift, "000000.ply"))
    integ = preprocess.StaticPointCloudIntegrator(E2E_RES, 0.0)
    try:
        integ.insert_points(xyz - np.array([-0.5, 0.25, 0.0]), w)  # subtracted in float64, before the narrowing
        want = integ.get_records()
    finally:
        integ.close()
    assert np.array_equal(got[:, :3].astype(np.float32).view(np.uint32), want[:, :3].view(np.uint32))


def test_preprocess_map_of_a_compressed_pcd_equals_the_binary_pcd(scene_files):
    tmp, scene, argv = scene_files
    n = len(scene.points)
    rec = np.zeros(n, dtype=[("x", "<f4"), ("normal", "<f4", (3,)), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")])
    rec["x"], rec["y"], rec["z"], rec["intensity"] = scene.points[:, 0], scene.points[:, 1], scene.points[:, 2], scene.intensities
    rec["normal"] = np.random.default_rng(1).normal(size=(n, 3))
    head = f"VERSION 0.7\nFIELDS x normal y z intensity\nSIZE 4 4 4 4 4\nTYPE F F F F F\nCOUNT 1 3 1 1 1\nWIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA "
    binary, compressed = str(tmp / "b.pcd"), str(tmp / "c.pcd")
    with open(binary, "wb") as f:
        f.write((head + "binary\n").encode() + rec.tobytes())
    planes = b"".join(np.ascontiguousarray(rec[k]).tobytes() for k in rec.dtype.names)
    stream = lo.lzf_pack_literals(planes)
    with open(compressed, "wb") as f:
        f.write((head + "binary_compressed\n").encode() + np.array([len(stream), len(planes)], dtype="<u4").tobytes() + stream)
    dst_b, dst_c = str(tmp / "d_b"), str(tmp / "d_c")
    assert preprocess_map.main(argv + ["--map_path", binary, "--dst_path", dst_b]) == 0
    assert preprocess_map.main(argv + ["--map_path", compressed, "--dst_path", dst_c]) == 0
    files_b, calib_b = read_dir(dst_b)
    files_c, calib_c = read_dir(dst_c)
    for name in FILES:
        assert files_b[name] == files_c[name], name
    assert calib_b["meta"].pop("data_path") == binary and calib_c["meta"].pop("data_path") == compressed
    assert calib_b == calib_c and "map_origin" not in calib_b["meta"]


def test_the_phase_clock_is_read_cleared_by_a_refused_call_and_refused():
    import ctypes
    import math

    from direct_visual_lidar_calibration_amd import _lib

    lib = _lib.load()
    rec = make_records(0, 1)
    assert rec.shape == (1, 20)
    a = preprocess.StaticPointCloudIntegrator(RES, 0.0)
    try:
        assert a.insert_las(rec.reshape(-1), 20, 0, SCALE, OFFSET, ORIGIN) == 0
        ms = (ctypes.c_double * 3)(-1.0, -1.0, -1.0)
        assert lib.nidreg_integrator_las_timing(ms) == 0 and all(math.isfinite(v) and v >= 0.0 for v in ms)  # upload, decode kernel, the integrator's passes
        with pytest.raises(ValueError, match="point formats 0..10 are read, got 11"):
            a.insert_las(rec.reshape(-1), 20, 11, SCALE, OFFSET, ORIGIN)
        assert lib.nidreg_integrator_las_timing(ms) == 0 and list(ms) == [0.0, 0.0, 0.0]  # the call clears its clock before it checks anything
        assert lib.nidreg_integrator_las_timing(None) == _lib.NIDREG_ERR_INVALID
    finally:
        a.close()
