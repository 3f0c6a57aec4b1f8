"""float32 cloud ingest: ``nidreg_cloud_create_f32`` / ``nid.Cloud.from_float32`` / ``dataset.read_ply_float32`` and the
``calibrate`` path that uses them.  The reference stores every cloud as four floats per vertex (preprocess.cpp:161-169) and
widens them to doubles after loading (visual_lidar_data.cpp:19-26); here the floats are uploaded as stored and widened on the
GPU.  float -> double is exact, so every handle built from such a cloud must have the bits of one built from the host-widened
doubles: same info, same cost and gradient (==), same fixed-point histograms."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from direct_visual_lidar_calibration_amd import _lib, calibrate, calibration, dataset, nid, se3, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "direct_visual_lidar_calibration_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "cxx", "test_dropin_f32.bin")

CAMERAS = {
    "plumb_bob": ("plumb_bob", [210.0, 205.0, 160.0, 120.0], [-0.04, 0.08, 1e-4, -3e-4, -0.04], 320, 240),
    "fisheye": ("fisheye", [140.0, 140.0, 160.0, 120.0], [-0.01, 0.002, -1e-4, 1e-5], 320, 240),
    "omnidir": ("omnidir", [110.0, 110.0, 160.0, 160.0, 1.0], [-0.02, 0.003, 1e-4, -2e-4], 320, 320),
    "equirectangular": ("equirectangular", [384.0, 256.0], [], 384, 256),
    "atan": ("atan", [210.0, 205.0, 160.0, 120.0], [0.6], 320, 240),
    "rational_polynomial": ("rational_polynomial", [210.0, 205.0, 160.0, 120.0], [0.05, -0.02, 1e-4, -2e-4, 0.01, 0.03, -0.01, 0.002], 320, 240),
}

# record layouts: float fields in file order ("e*" = extra properties around the intensity)
LAYOUTS = {
    16: ["x", "y", "z", "intensity"],
    20: ["x", "y", "z", "e0", "intensity"],
    28: ["e0", "x", "y", "z", "intensity", "e1", "e2"],
}


def records(xyz, inten, fields, seed=0):
    """(xyz view (n, 3), intensity view (n,)) over ONE buffer of float32 records laid out as `fields`."""
    n = xyz.shape[0]
    dt = np.dtype([(f, "<f4") for f in fields])
    rec = np.zeros(n, dtype=dt)
    rng = np.random.default_rng(seed)
    for f in fields:
        rec[f] = rng.standard_normal(n)
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    rec["intensity"] = inten
    if n == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.float32)
    xv = np.ndarray((n, 3), dtype="<f4", buffer=rec, offset=dt.fields["x"][1], strides=(dt.itemsize, 4))
    iv = np.ndarray((n,), dtype="<f4", buffer=rec, offset=dt.fields["intensity"][1], strides=(dt.itemsize,))
    return xv, iv


def widen(xyz, inten):
    pts = np.ones((xyz.shape[0], 4))
    pts[:, :3] = xyz
    return pts, np.asarray(inten, dtype=np.float64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# --------------------------------------------------------------------------------------------- CPU
def test_header_declares_and_library_exports_the_f32_entry_point():
    import re

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nidreg.h")).read(), flags=re.S)
    assert re.search(r"int\s+nidreg_cloud_create_f32\s*\(\s*int device_id,\s*const float\* points,\s*int64_t point_stride,\s*const float\* intensities,"
                     r"\s*int64_t intensity_stride,\s*int64_t num_points,\s*nidreg_cloud\*\* out\s*\)", src)
    assert "nidreg_cloud_create_f32" in _lib.EXPORTS
    assert hasattr(_lib.load(), "nidreg_cloud_create_f32")


def test_f32_argument_validation_before_any_device_call():
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    c = ctypes.c_void_p()
    cases = [
        (0, p, 16, p + 12, 16, -1),            # num_points < 0
        (0, p, 16, p + 12, 16, 2**31),         # num_points > INT_MAX
        (0, None, 16, p + 12, 16, 2),          # null points
        (0, p, 16, None, 16, 2),               # null intensities
        (0, p, 8, p + 12, 16, 2),              # point_stride < 12
        (0, p, 16, p + 12, 2, 2),              # intensity_stride < 4
        (0, p, 18, p + 12, 16, 2),             # point_stride not a multiple of 4
        (0, p, 16, p + 12, 6, 2),              # intensity_stride not a multiple of 4
        (0, p + 2, 16, p + 12, 16, 2),         # points not 4-byte aligned
        (0, p, 16, p + 13, 16, 2),             # intensities not 4-byte aligned
        (-1, p, 16, p + 12, 16, 2),            # device id out of range
    ]
    for dev, pp, ps, ip, istr, n in cases:
        c.value = None
        rc = lib.nidreg_cloud_create_f32(dev, pp, ps, ip, istr, n, ctypes.byref(c))
        msg = _lib.last_error()
        assert rc == -1, (dev, ps, istr, n, rc, msg)  # NIDREG_ERR_INVALID
        assert msg.startswith("nidreg_cloud_create_f32: ") and len(msg) > len("nidreg_cloud_create_f32: ")
        assert c.value is None
    assert lib.nidreg_cloud_create_f32(0, p, 16, p + 12, 16, 1, None) == -1


def test_from_float32_refuses_what_the_abi_cannot_take():
    good = np.zeros((4, 3), np.float32)
    ints = np.zeros(4, np.float32)
    with pytest.raises(ValueError, match="byte order"):
        nid.Cloud.from_float32(good.astype(">f4"), ints)
    with pytest.raises(ValueError, match="byte order"):
        nid.Cloud.from_float32(good, ints.astype(">f4"))
    with pytest.raises(ValueError, match="consecutive"):
        nid.Cloud.from_float32(np.zeros((3, 4), np.float32).T, ints)
    raw = np.zeros(4 * 7 + 12, dtype=np.uint8)
    with pytest.raises(ValueError, match="multiples of 4"):  # rows 6 bytes apart
        nid.Cloud.from_float32(np.ndarray((4, 3), dtype=np.float32, buffer=raw, offset=0, strides=(6, 4)), ints)
    with pytest.raises(ValueError):
        nid.Cloud.from_float32(np.zeros((4, 3)), ints)  # float64
    with pytest.raises(ValueError):
        nid.Cloud.from_float32(good, np.zeros(5, np.float32))


def _write_records(path, fields, xyz, inten, fmt="binary_little_endian", types=None, pre_element=None):
    n = xyz.shape[0]
    types = types or {}
    order = "<" if fmt != "binary_big_endian" else ">"
    codes = {f: types.get(f, "f4") for f in fields}
    names = {"f4": "float", "f8": "double", "u1": "uchar"}
    dt = np.dtype([(f, order + codes[f]) for f in fields])
    rec = np.zeros(n, dtype=dt)
    rng = np.random.default_rng(5)
    for f in fields:
        rec[f] = rng.standard_normal(n) * 3
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    key = next(f for f in fields if f in ("intensity", "scalar_intensity", "intensities"))
    rec[key] = inten
    head = f"ply\nformat {fmt} 1.0\ncomment test\n"
    body = b""
    if pre_element is not None:
        head += f"element camera {pre_element}\nproperty float a\nproperty uchar b\n"
        body += np.zeros(pre_element, dtype=[("a", order + "f4"), ("b", "u1")]).tobytes()
    head += f"element vertex {n}\n" + "".join(f"property {names[codes[f]]} {f}\n" for f in fields) + "end_header\n"
    if fmt == "ascii":
        body = "".join(" ".join(repr(float(r[f])) for f in fields) + "\n" for r in rec).encode()
    else:
        body += rec.tobytes()
    with open(path, "wb") as f:
        f.write(head.encode() + body)


def _cloud(n, seed=1):
    rng = np.random.default_rng(seed)
    xyz = (rng.standard_normal((n, 3)) * 10).astype(np.float32)
    inten = rng.random(n).astype(np.float32)
    return xyz, inten


def _check_f32_equals_read_ply(path):
    got = dataset.read_ply_float32(path)
    assert got is not None
    xyz, inten = got
    assert xyz.dtype == np.float32 and inten.dtype == np.float32 and xyz.shape[1] == 3
    assert np.may_share_memory(xyz, inten)  # one buffer: the vertex block as read
    pts, ints = dataset.read_ply(path)
    assert xyz.shape[0] == pts.shape[0]
    w_pts, w_int = widen(xyz, inten)
    assert np.array_equal(bits(w_pts), bits(pts)) and np.array_equal(bits(w_int), bits(ints))
    # the views alias one read of the file's vertex block (the last element of these files)
    raw = xyz.base
    assert raw is inten.base and raw.dtype == np.uint8 and raw.size == xyz.shape[0] * xyz.strides[0]
    data = open(path, "rb").read()
    assert raw.tobytes() == data[len(data) - raw.size:]
    return xyz, inten


def test_read_ply_float32_views_equal_read_ply_bit_for_bit(tmp_path):
    xyz, inten = _cloud(1000)
    xyz[:4] = [[0.0, -0.0, 1e-40], [np.inf, -np.inf, np.nan], [np.finfo(np.float32).max, -np.finfo(np.float32).max, 1.0], [1e-45, -1e-45, 0.0]]
    inten[:4] = [-0.0, 1e-40, np.nan, np.inf]
    # write_ply output
    p = str(tmp_path / "w.ply")
    dataset.write_ply(p, widen(xyz, inten)[0], inten)
    v, i = _check_f32_equals_read_ply(p)
    assert v.strides == (16, 4) and i.strides == (16,)
    raw = np.fromfile(p, dtype=np.uint8)[-1000 * 16:]
    assert np.array_equal(np.frombuffer(raw.tobytes(), dtype="<f4").reshape(1000, 4)[:, :3].view(np.uint32), v.view(np.uint32))
    # 20 / 28 B records with extra properties before and after the intensity, and an element before the vertices
    for size, fields in LAYOUTS.items():
        p = str(tmp_path / f"r{size}.ply")
        _write_records(p, fields, xyz, inten, pre_element=3 if size == 28 else None)
        v, i = _check_f32_equals_read_ply(p)
        assert v.strides == (size, 4) and i.strides == (size,)
    # every intensity property name, with read_ply's precedence
    for key in ("intensity", "scalar_intensity", "intensities"):
        p = str(tmp_path / f"{key}.ply")
        _write_records(p, ["x", "y", "z", key], xyz, inten)
        _check_f32_equals_read_ply(p)
    p = str(tmp_path / "both.ply")
    _write_records(p, ["x", "y", "z", "intensities", "intensity"], xyz, inten)
    v, i = _check_f32_equals_read_ply(p)  # "intensity" (offset 16) wins over "intensities" (offset 12), as in read_ply
    assert i.strides == (20,) and i.__array_interface__["data"][0] - v.__array_interface__["data"][0] == 16
    # an empty cloud
    p = str(tmp_path / "empty.ply")
    _write_records(p, LAYOUTS[16], xyz[:0], inten[:0])
    v, i = dataset.read_ply_float32(p)
    assert v.shape == (0, 3) and i.shape == (0,)


def test_read_ply_float32_declines_other_files(tmp_path):
    xyz, inten = _cloud(50)
    fields = LAYOUTS[16]
    p = str(tmp_path / "a.ply")
    _write_records(p, fields, xyz, inten, fmt="ascii")
    assert dataset.read_ply_float32(p) is None
    _write_records(p, fields, xyz, inten, fmt="binary_big_endian")
    assert dataset.read_ply_float32(p) is None
    for f in ("x", "intensity"):
        _write_records(p, fields, xyz, inten, types={f: "f8"})
        assert dataset.read_ply_float32(p) is None
    with open(p, "wb") as f:  # no intensity property
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nend_header\n" + np.zeros(6, "<f4").tobytes())
    assert dataset.read_ply_float32(p) is None
    # read_ply still reads all of them (its behaviour is unchanged: tests/test_dataset.py)
    _write_records(p, fields, xyz, inten, fmt="binary_big_endian")
    pts, ints = dataset.read_ply(p)
    assert np.array_equal(pts[:, :3], xyz.astype(np.float64)) and np.array_equal(ints, inten.astype(np.float64))


def _write_dir(path, n=3000, bags=2, seed=3, camera="plumb_bob"):
    scenes = [synth.make_scene(CAMERAS[camera], num_points=n, seed=seed + k) for k in range(bags)]
    s0 = scenes[0]
    dataset.write_preprocessed(path, (s0.model, s0.intrinsics, s0.distortion), [(f"bag{k}", s.image_u8, s.points, s.intensities) for k, s in enumerate(scenes)],
                               init_T_lidar_camera_tum=dataset.T_camera_lidar_to_tum(s0.T_camera_lidar_init))
    return scenes


def test_visual_lidar_data_float32_bags_widen_lazily_to_the_same_arrays(tmp_path, monkeypatch):
    d = str(tmp_path / "data")
    scenes = _write_dir(d, n=2000)
    _, bags = dataset.load_dataset(d)
    monkeypatch.setattr(dataset, "read_ply_float32", lambda path: None)
    _, eager = dataset.load_dataset(d)
    for b, e, s in zip(bags, eager, scenes):
        assert b.xyz_f32 is not None and e.xyz_f32 is None
        assert b.num_points == e.num_points == s.points.shape[0]
        assert "points" not in vars(b) and "intensities" not in vars(b)
        assert np.array_equal(bits(b.points), bits(e.points)) and np.array_equal(bits(b.intensities), bits(e.intensities))
        assert b.points.dtype == np.float64 and b.points.shape == (s.points.shape[0], 4) and b.points.flags.c_contiguous
        assert np.array_equal(b.points, s.points) and np.array_equal(b.intensities, s.intensities)
        assert b.points is b.points  # cached


def test_cli_dry_run_on_float32_directory_never_widens(tmp_path, monkeypatch):
    d = str(tmp_path / "data")
    _write_dir(d, n=2000)
    seen = []
    real = dataset.load_dataset

    def spy(*a, **k):
        cfg, bags = real(*a, **k)
        seen.extend(bags)
        return cfg, bags

    monkeypatch.setattr(dataset, "load_dataset", spy)
    lines = []
    calibrate.run(calibrate.build_parser().parse_args([d, "--dry_run"]), log=lines.append)
    assert len(seen) == 2
    for b in seen:
        assert b.xyz_f32 is not None
        assert "points" not in vars(b) and "intensities" not in vars(b)
    assert any("loaded bag1: image 320x240, 2000 points" == ln for ln in lines), lines


def _cxx_build():
    import __graft_entry__

    if not os.path.exists(os.path.join(CSRC, "libnidreg.so")):
        __graft_entry__.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "test_dropin_f32.cpp"), "-L", CSRC, "-lnidreg",
                           f"-Wl,-rpath,{CSRC}", "-o", EXE])
    return EXE


def test_dropin_device_cloud_f32_constructor_compiles():
    assert os.path.exists(_cxx_build())


# --------------------------------------------------------------------------------------------- GPU
def _same_bits(a, b):
    assert np.float64(a).tobytes() == np.float64(b).tobytes(), (a, b)


def _compare_spline(proj, image_f64, c32, c64, bins, poses, cull=None, **kw):
    a = nid.NIDCost.from_cloud(proj, image_f64, c32, bins, cull=cull, **kw)
    b = nid.NIDCost.from_cloud(proj, image_f64, c64, bins, cull=cull, **kw)
    try:
        assert a.info() == b.info()
        for x in poses:
            ok1, v1, g1 = a(x)
            ok2, v2, g2 = b(x)
            assert ok1 == ok2
            _same_bits(v1, v2)
            assert np.array_equal(bits(g1), bits(g2))
            ha, hb = a.histogram_fixed(), b.histogram_fixed()
            assert np.array_equal(ha[0], hb[0]) and ha[1:] == hb[1:]
        return a.info()
    finally:
        a.close()
        b.close()


def _compare_nearest(proj, image_u8, c32, c64, bins, Ts, max_fov, cull=None):
    a = nid.CostCalculatorNID.from_cloud(proj, image_u8, c32, nid.NIDCostParams(bins), max_fov=max_fov, cull=cull)
    b = nid.CostCalculatorNID.from_cloud(proj, image_u8, c64, nid.NIDCostParams(bins), max_fov=max_fov, cull=cull)
    try:
        assert a.info() == b.info()
        total = 0
        for T in Ts:
            _same_bits(a.calculate(T), b.calculate(T))
            ha, hb = a.histogram_fixed(), b.histogram_fixed()
            assert np.array_equal(ha[0], hb[0]) and ha[1:] == hb[1:]
            total += int(ha[0].sum())
        return total
    finally:
        a.close()
        b.close()


def _both(xyz, inten, layout=16):
    """(cloud from the float32 records, cloud from the host-widened doubles)"""
    if layout == "soa":
        xv, iv = np.ascontiguousarray(xyz, dtype=np.float32), np.ascontiguousarray(inten, dtype=np.float32)
        assert xv.shape[0] <= 1 or (xv.strides == (12, 4) and iv.strides == (4,))
    else:
        xv, iv = records(np.asarray(xyz, np.float32), np.asarray(inten, np.float32), LAYOUTS[layout])
    pts, ints = widen(xv, iv)
    return nid.Cloud.from_float32(xv, iv), nid.Cloud(pts, ints)


def _scene(name, n=20000, seed=11):
    return synth.make_scene(CAMERAS[name], num_points=n, seed=seed)


@pytest.mark.gpu
def test_device_id_out_of_range_is_refused():
    lib = _lib.load()
    buf = np.zeros(8, np.float32)
    c = ctypes.c_void_p()
    assert lib.nidreg_cloud_create_f32(10000, buf.ctypes.data, 16, buf.ctypes.data + 12, 16, 2, ctypes.byref(c)) == -1
    assert "device_id" in _lib.last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("model", sorted(CAMERAS))
def test_every_camera_model_spline_and_nearest_with_and_without_culling(model):
    s = _scene(model)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    c32, c64 = _both(s.points[:, :3], s.intensities)
    assert c32.num_points == c64.num_points == s.points.shape[0]
    T = se3.to_matrix(s.T_camera_lidar_init)
    max_fov = nid.estimate_camera_fov(proj, (s.width, s.height))
    rng = np.random.default_rng(3)
    poses = [s.T_camera_lidar_init, synth.random_pose_near(s.T_camera_lidar_true, rng)]
    for cull in (None, (T, np.cos(max_fov), True)):
        _compare_spline(proj, s.image_f64, c32, c64, 16, poses, cull=cull)
        assert _compare_nearest(proj, s.image_u8, c32, c64, 16, [se3.to_matrix(x) for x in poses], max_fov, cull=cull) > 0
    c32.close()
    c64.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [16, 20, 28, "soa"])
def test_record_layouts_and_sizes_around_the_wave(layout):
    s = _scene("plumb_bob", n=5000, seed=4)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    x = s.T_camera_lidar_init
    for n in (0, 1, 63, 64, 65, 4097):
        c32, c64 = _both(s.points[:n, :3], s.intensities[:n], layout)
        assert c32.num_points == n
        if n == 0:
            errs = []
            for c in (c32, c64):  # an empty cloud: whatever the double route does, the float route does too
                try:
                    h = nid.NIDCost.from_cloud(proj, s.image_f64, c, 16)
                    errs.append(("ok", h.num_points, h(x, want_grad=False)[1]))
                    h.close()
                except RuntimeError as e:
                    errs.append(("error", str(e)))
            assert len(errs) == 2 and str(errs[0]) == str(errs[1]), errs
        else:
            _compare_spline(proj, s.image_f64, c32, c64, 16, [x])
        c32.close()
        c64.close()


@pytest.mark.gpu
def test_two_million_points_and_wide_bins():
    s = _scene("plumb_bob", n=30011, seed=12)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    x = s.T_camera_lidar_init
    c32, c64 = _both(s.points[:, :3], s.intensities)
    for bins in (16, 256, 300):  # bins > 256 reads d_int on the device (occupied bins)
        _compare_spline(proj, s.image_f64, c32, c64, bins, [x])
    max_fov = nid.estimate_camera_fov(proj, (s.width, s.height))
    _compare_nearest(proj, s.image_u8, c32, c64, 300, [se3.to_matrix(x)], max_fov)
    c32.close()
    c64.close()
    # ~2M points: the scene's cloud 67 times, jittered, narrowed to float
    rng = np.random.default_rng(2)
    reps = 67
    xyz = (np.tile(s.points[:, :3], (reps, 1)) + rng.normal(0.0, 0.01, (reps * s.points.shape[0], 3))).astype(np.float32)
    inten = np.tile(s.intensities, reps).astype(np.float32)
    c32, c64 = _both(xyz, inten)
    assert c32.num_points == xyz.shape[0] > 2_000_000
    T = se3.to_matrix(x)
    _compare_spline(proj, s.image_f64, c32, c64, 16, [x], cull=(T, np.cos(max_fov), True))
    _compare_nearest(proj, s.image_u8, c32, c64, 16, [T], max_fov)
    c32.close()
    c64.close()


@pytest.mark.gpu
def test_sharded_handle_from_a_float32_cloud():
    s = _scene("fisheye", n=20000, seed=5)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    c32, c64 = _both(s.points[:, :3], s.intensities, 28)
    T = se3.to_matrix(s.T_camera_lidar_init)
    min_z = np.cos(nid.estimate_camera_fov(proj, (s.width, s.height)))
    info = _compare_spline(proj, s.image_f64, c32, c64, 16, [s.T_camera_lidar_init], cull=(T, min_z, True), devices=[0, 0])
    assert info["num_points"] > 0
    c32.close()
    c64.close()


@pytest.mark.gpu
def test_special_values_pass_through_exactly():
    """Denormal, +-0, +-inf, NaN and FLT_MAX coordinates and intensities mixed into a scene, and a group of points whose
    coordinates are ALL float denormals: at the identity pose they project to real pixels (x / z, y / z are ordinary ratios),
    so a widening that flushed denormals to zero would drop them (0 / 0)."""
    s = _scene("plumb_bob", n=6000, seed=9)
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    f32 = np.finfo(np.float32)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, f32.max, -f32.max, 1e-45, -1e-45, 1e-40, f32.tiny, 1.0], dtype=np.float32)
    rng = np.random.default_rng(1)
    sp = rng.choice(specials, size=(600, 3)).astype(np.float32)
    sp_i = rng.choice(specials, size=600).astype(np.float32)
    xyz = np.concatenate([s.points[:, :3].astype(np.float32), sp])
    inten = np.concatenate([s.intensities.astype(np.float32), sp_i])
    c32, c64 = _both(xyz, inten)
    rng2 = np.random.default_rng(4)
    poses = [s.T_camera_lidar_init, synth.random_pose_near(s.T_camera_lidar_true, rng2)]
    max_fov = nid.estimate_camera_fov(proj, (s.width, s.height))
    T = se3.to_matrix(s.T_camera_lidar_init)
    for bins in (16, 256):
        _compare_spline(proj, s.image_f64, c32, c64, bins, poses)
        _compare_spline(proj, s.image_f64, c32, c64, bins, poses[:1], cull=(T, np.cos(max_fov), True))
    _compare_nearest(proj, s.image_u8, c32, c64, 16, [se3.to_matrix(x) for x in poses], max_fov)
    c32.close()
    c64.close()
    # all-denormal coordinates: z = 2^-140, x, y = k * 2^-149 (|k| < 300)
    k = rng.integers(-300, 300, size=(4000, 2))
    den = np.empty((4000, 3), dtype=np.float32)
    den[:, :2] = k.astype(np.float32) * np.float32(2.0**-149)
    den[:, 2] = np.float32(2.0**-140)
    assert np.all(np.abs(den) < f32.tiny) and np.all(den[:, 2] > 0)
    c32, c64 = _both(den, rng.random(4000).astype(np.float32))
    assert _compare_nearest(proj, s.image_u8, c32, c64, 16, [np.eye(4)], max_fov) > 0
    c32.close()
    c64.close()


@pytest.mark.gpu
@pytest.mark.parametrize("reg", ["nid_bfgs", "nid_nelder_mead"])
def test_calibrate_pairs_float32_pair_gives_the_bits_of_the_widened_pair(reg):
    s = synth.make_scene("pinhole_vga", num_points=100_000, seed=20250523)  # configs[0]
    proj = nid.create_camera(s.model, s.intrinsics, s.distortion)
    xv, iv = records(s.points[:, :3].astype(np.float32), s.intensities.astype(np.float32), LAYOUTS[16])
    pts, ints = widen(xv, iv)
    params = calibration.VisualCameraCalibrationParams(nid_bins=16, registration_type=reg)
    x32, _ = calibrate.calibrate_pairs(proj, [(s.image_u8, xv, iv)], s.T_camera_lidar_init, params)
    x64, _ = calibrate.calibrate_pairs(proj, [(s.image_u8, pts, ints)], s.T_camera_lidar_init, params)
    assert np.array_equal(bits(x32), bits(x64))


@pytest.mark.gpu
def test_cli_calib_json_byte_identical_to_the_double_route(tmp_path, monkeypatch):
    d32 = str(tmp_path / "data")
    _write_dir(d32, n=12000, bags=2, seed=21)
    d64 = str(tmp_path / "data64")
    shutil.copytree(d32, d64)
    l32, l64 = [], []
    calibrate.run(calibrate.build_parser().parse_args([d32]), log=l32.append)
    with monkeypatch.context() as m:
        m.setattr(dataset, "read_ply_float32", lambda path: None)
        calibrate.run(calibrate.build_parser().parse_args([d64]), log=l64.append)
    a = open(os.path.join(d32, "calib.json"), "rb").read()
    b = open(os.path.join(d64, "calib.json"), "rb").read()
    assert a == b and b"T_lidar_camera" in a
    assert "T_lidar_camera" in json.loads(a)["results"]
    assert [ln for ln in l32 if not ln.startswith("saved to")] == [ln for ln in l64 if not ln.startswith("saved to")]


@pytest.mark.gpu
def test_dropin_device_cloud_float_constructor_gives_the_same_costs(tmp_path):
    exe = _cxx_build()
    s = _scene("plumb_bob", n=20000, seed=31)
    T = se3.to_matrix(s.T_camera_lidar_init)
    min_z = float(np.cos(nid.estimate_camera_fov(nid.create_camera(s.model, s.intrinsics, s.distortion), (s.width, s.height))))
    intr = np.zeros(5)
    intr[: len(s.intrinsics)] = s.intrinsics
    dist = np.zeros(8)
    dist[: len(s.distortion)] = s.distortion
    path = tmp_path / "scene.bin"
    n = s.points.shape[0]
    xyz = s.points[:, :3].astype(np.float32)
    inten = s.intensities.astype(np.float32)
    with open(path, "wb") as f:
        f.write(s.model.encode().ljust(64, b"\0"))
        f.write(np.array([s.width, s.height, n, 16, len(s.intrinsics), len(s.distortion)], dtype="<i4").tobytes())
        f.write(intr.tobytes() + dist.tobytes() + np.asarray(s.T_camera_lidar_init, dtype=np.float64).tobytes() + np.float64(min_z).tobytes() + T.astype(np.float64).tobytes())
        f.write(np.ascontiguousarray(s.image_u8).tobytes())
        f.write(np.ascontiguousarray(xyz).tobytes() + np.ascontiguousarray(inten).tobytes())
    out = subprocess.check_output([exe, str(path)]).decode().split()
    vals = [float(v) for v in out]
    assert len(vals) == 6, out
    # (Frame doubles, 16 B records, SoA) x (no cull, cull)
    assert vals[0] == vals[1] == vals[2] and np.isfinite(vals[0])
    assert vals[3] == vals[4] == vals[5] and np.isfinite(vals[3])
