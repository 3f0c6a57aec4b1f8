"""INTEGRATION.md executed: integration/reference_camera.patch is applied to a scratch copy of the reference's
two camera headers, and tests/cxx/test_integration.cpp is compiled in -DNIDREG_WITH_REFERENCE_DEPS mode together
with the reference's own src/camera/create_camera.cpp -- i.e. the reference's camera factory and classes feeding
this repository's vlcal::NIDCost.  CPU: the patch applies, everything compiles and links, the patched cameras
report the right model ids / padded parameters and still project on the CPU.  GPU: the binary (built here, it
travels with the snapshot) evaluates cost + Jacobian and matches the oracle.  Needs the reference tree to build."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
CSRC = os.path.join(ROOT, "direct_visual_lidar_calibration_amd", "csrc")
# programs compiled from reference sources are build products of oracle/_ref/ (never committed; they travel with the built tree)
REF_BIN = os.path.join(ROOT, "oracle", "_ref")
EXE = os.path.join(REF_BIN, "test_integration.bin")
EXE_CAL = os.path.join(REF_BIN, "test_integration_calibrate.bin")
RPATH_REL = "-Wl,-rpath,$ORIGIN/../../direct_visual_lidar_calibration_amd/csrc"  # libnidreg.so wherever the tree lies


def build(scratch):
    inc = os.path.join(scratch, "include", "camera")
    os.makedirs(inc, exist_ok=True)
    for name in ("generic_camera_base.hpp", "generic_camera.hpp"):
        shutil.copy(os.path.join(REF, "include", "camera", name), inc)
    subprocess.check_call(["patch", "-p1", "-s", "-d", scratch, "-i", os.path.join(ROOT, "integration", "reference_camera.patch")])
    os.makedirs(REF_BIN, exist_ok=True)
    if not os.path.exists(os.path.join(CSRC, "libnidreg.so")):
        import __graft_entry__

        __graft_entry__.build()
    cmd = ["g++", "-std=c++17", "-O1", "-DNIDREG_WITH_REFERENCE_DEPS", "-Wno-sign-compare",
           "-I", os.path.join(scratch, "include"),          # the two patched headers shadow the originals
           "-I", os.path.join(ROOT, "oracle", "shim"),      # Eigen / ceres / OpenCV as this image knows them
           "-I", os.path.join(REF, "include"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cxx", "test_integration.cpp"), os.path.join(REF, "src", "camera", "create_camera.cpp"),
           "-L", CSRC, "-lnidreg", f"-Wl,-rpath,{CSRC}", RPATH_REL, "-o", EXE]
    subprocess.check_call(cmd)
    return EXE


def build_calibrate(scratch):
    """The reference's unmodified visual_camera_calibration.cpp against the drop-in headers (integration/include first)."""
    build(scratch)  # patched camera headers + libnidreg.so
    cmd = ["g++", "-std=c++17", "-O1", "-DNIDREG_WITH_REFERENCE_DEPS", "-Wno-sign-compare", "-Wl,--allow-multiple-definition",
           "-I", os.path.join(scratch, "include"), "-I", os.path.join(ROOT, "integration", "include"), "-I", os.path.join(ROOT, "oracle", "shim"),
           "-I", os.path.join(REF, "include"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cxx", "test_integration_calibrate.cpp"), os.path.join(REF, "src", "vlcal", "calib", "visual_camera_calibration.cpp"),
           os.path.join(REF, "src", "camera", "create_camera.cpp"), os.path.join(REF, "src", "vlcal", "common", "estimate_fov.cpp"),
           "-L", CSRC, "-lnidreg", f"-Wl,-rpath,{CSRC}", RPATH_REL, "-o", EXE_CAL]
    subprocess.check_call(cmd)
    return EXE_CAL


EXE_CAL_NP = os.path.join(REF_BIN, "test_integration_calibrate_nopatch.bin")


def build_calibrate_nopatch():
    """The second integration route: NO reference header is patched; integration/src/create_camera.cpp is compiled instead
    of the reference's src/camera/create_camera.cpp (its cameras are the reference's GenericCamera<P> objects that also
    implement camera::NidregCameraInfo), everything else as in build_calibrate."""
    if not os.path.exists(os.path.join(CSRC, "libnidreg.so")):
        import __graft_entry__

        __graft_entry__.build()
    os.makedirs(REF_BIN, exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-DNIDREG_WITH_REFERENCE_DEPS", "-Wno-sign-compare", "-Wl,--allow-multiple-definition",
           "-I", os.path.join(ROOT, "integration", "include"), "-I", os.path.join(ROOT, "oracle", "shim"),
           "-I", os.path.join(REF, "include"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cxx", "test_integration_calibrate.cpp"), os.path.join(REF, "src", "vlcal", "calib", "visual_camera_calibration.cpp"),
           os.path.join(ROOT, "integration", "src", "create_camera.cpp"), os.path.join(REF, "src", "vlcal", "common", "estimate_fov.cpp"),
           "-L", CSRC, "-lnidreg", f"-Wl,-rpath,{CSRC}", RPATH_REL, "-o", EXE_CAL_NP]
    subprocess.check_call(cmd)
    return EXE_CAL_NP


def test_unpatched_reference_headers_with_the_replacement_camera_factory():
    """visual_camera_calibration.cpp, estimate_fov.cpp and EVERY reference header unmodified; only create_camera.cpp is
    swapped for integration/src/create_camera.cpp: compiles, links, starts."""
    if not os.path.isdir(os.path.join(REF, "include", "camera")):
        pytest.skip("reference tree not present")
    exe = build_calibrate_nopatch()
    assert subprocess.run([exe]).returncode == 2


def test_reference_calibration_driver_compiles_against_the_dropin_headers(tmp_path):
    """visual_camera_calibration.cpp, unmodified, with <vlcal/costs/nid_cost.hpp>, <vlcal/calib/cost_calculator_nid.hpp>
    and <vlcal/calib/view_culling.hpp> forwarded to include/vlcal_amd/: the reference's constructor calls and functor
    uses (:73-85, :147-173, :193-216) are source compatible with the drop-in classes, and the program links."""
    if not os.path.isdir(os.path.join(REF, "include", "camera")):
        pytest.skip("reference tree not present")
    exe = build_calibrate(str(tmp_path))
    assert os.path.exists(exe)
    assert subprocess.run([exe]).returncode == 2  # usage error path: starts and exits without touching the GPU
    from direct_visual_lidar_calibration_amd import _lib

    if _lib.load().nidreg_device_count() == 0:
        # without a GPU the reference's calibrate() runs up to its first engine call -- estimate_camera_fov through the
        # reference's own Nelder-Mead and CPU projection, then ViewCulling through the drop-in -- and fails loudly there
        r = subprocess.run([exe, _scene_file(tmp_path), "16"], capture_output=True, text=True)
        assert r.returncode != 0 and "no HIP device" in r.stderr, (r.returncode, r.stderr[-300:])


def _scene_file(tmp_path):
    from test_reference_golden import CASES

    c = CASES[0]
    intr = np.zeros(5)
    intr[: len(c["intrinsics"])] = c["intrinsics"]
    dist = np.zeros(8)
    dist[: len(c["distortion"])] = c["distortion"]
    path = tmp_path / "scene_cal.bin"
    with open(path, "wb") as f:
        f.write(c["model"].encode().ljust(64, b"\0"))
        f.write(struct.pack("<6i", c["W"], c["H"], c["points"].shape[0], int(c["nm_bins"]), len(c["intrinsics"]), len(c["distortion"])))
        f.write(intr.tobytes() + dist.tobytes() + np.asarray(c["se3"], dtype=np.float64).tobytes() + struct.pack("<d", 0.0) + c["T"].astype(np.float64).tobytes())
        f.write(np.ascontiguousarray(c["image_u8"]).tobytes())
        f.write(np.ascontiguousarray(c["points"], dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(c["intensities"], dtype=np.float64).tobytes())
    return str(path)


def test_patch_applies_builds_and_cameras_expose_parameters(tmp_path):
    if not os.path.isdir(os.path.join(REF, "include", "camera")):
        pytest.skip("reference tree not present")
    import oracle_lib

    exe = build(str(tmp_path))
    out = subprocess.check_output([exe, "--describe"]).decode().strip().splitlines()
    ids = {"plumb_bob": 0, "fisheye": 1, "equidistant": 1, "omnidir": 2, "equirectangular": 3, "atan": 4, "rational_polynomial": 5}
    assert len(out) == len(ids)
    given = {"plumb_bob": ([210, 205, 160, 120], [-0.04, 0.08, 1e-4, -3e-4, -0.04]), "fisheye": ([140, 140, 160, 120], [-0.01, 0.002]), "equidistant": ([140, 140, 160, 120], []),
             "omnidir": ([110, 110, 160, 160, 1.0], [-0.02, 0.003, 1e-4, -2e-4]), "equirectangular": ([384, 256], []), "atan": ([210, 205, 160, 120], [0.6]),
             "rational_polynomial": ([210, 205, 160, 120], [0.05, -0.02, 1e-4, -2e-4, 0.01, 0.03, -0.01, 0.002])}
    for line in out:
        tok = line.split()
        name, mid, vals = tok[0], int(tok[1]), np.array([float(v) for v in tok[2:]])
        assert mid == ids[name]
        intr, dist = given[name]
        assert np.array_equal(vals[:5], np.pad(np.array(intr, dtype=float), (0, 5 - len(intr))))
        assert np.array_equal(vals[5:13], np.pad(np.array(dist, dtype=float), (0, 8 - len(dist))))  # zero padded, surplus dropped
        uv = oracle_lib.project("fisheye" if name == "equidistant" else name, intr, dist, np.array([[0.3, -0.2, 2.0]]))
        assert np.array_equal(vals[13:15], uv[0])  # the reference's CPU projection is untouched by the patch


@pytest.mark.gpu
def test_reference_cameras_feed_the_gpu_cost(tmp_path):
    if not os.path.exists(EXE):
        pytest.skip("oracle/_ref/test_integration.bin was not built (needs the reference tree; built by the CPU test)")
    import oracle_lib
    from direct_visual_lidar_calibration_amd import se3, synth
    from test_gpu_parity import CAMERAS

    for name, bins in (("plumb_bob", 256), ("equirectangular", 16)):
        s = synth.make_scene(CAMERAS[name], num_points=15000, seed=33)
        x = s.T_camera_lidar_init
        intr = np.zeros(5)
        intr[: len(s.intrinsics)] = s.intrinsics
        dist = np.zeros(8)
        dist[: len(s.distortion)] = s.distortion
        path = tmp_path / f"{name}.bin"
        with open(path, "wb") as f:
            f.write(s.model.encode().ljust(64, b"\0"))
            f.write(struct.pack("<6i", s.width, s.height, s.points.shape[0], bins, len(s.intrinsics), len(s.distortion)))
            f.write(intr.tobytes() + dist.tobytes() + np.asarray(x, dtype=np.float64).tobytes() + struct.pack("<d", 0.0) + se3.to_matrix(x).astype(np.float64).tobytes())
            f.write(np.ascontiguousarray(s.image_u8).tobytes())
            f.write(np.ascontiguousarray(s.points, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(s.intensities, dtype=np.float64).tobytes())
        vals = np.array([float(v) for v in subprocess.check_output([EXE, str(path)]).decode().split()])
        ref = oracle_lib.nid_cost(s.model, s.intrinsics, s.distortion, s.image_f64, s.points, s.intensities, bins, x)
        parity.check_cost(vals[0], ref["cost"])
        parity.check_cost(vals[8], ref["cost"])
        parity.check_grad(vals[1:8], ref["grad"])


@pytest.mark.gpu
def test_reference_calibrate_drives_the_gpu_engine_without_any_header_patch(tmp_path):
    """Same as below through the patch-free route (replacement create_camera.cpp, all reference headers untouched)."""
    if not os.path.exists(EXE_CAL_NP):
        pytest.skip("oracle/_ref/test_integration_calibrate_nopatch.bin was not built (needs the reference tree)")
    from direct_visual_lidar_calibration_amd import se3
    from test_reference_golden import CASES

    c = CASES[0]
    path = _scene_file(tmp_path)
    out = subprocess.check_output([EXE_CAL_NP, str(path), str(int(c["nm_bins"]))]).decode().strip().splitlines()
    vals = [float(v) for v in out[-1].split()]
    T = np.array(vals[:16]).reshape(4, 4)
    dt, dr = se3.delta_trans_rot(se3.from_matrix(c["ref_nm_T_camera_lidar"]), se3.from_matrix(T))
    assert dt <= 1e-3 and dr <= 1e-3, (dt, dr)


@pytest.mark.gpu
def test_reference_calibrate_drives_the_gpu_engine(tmp_path):
    """The reference's own VisualCameraCalibration::calibrate (Nelder-Mead route) running on the GPU engine through the
    drop-in headers ends where the reference's CPU build ends (fixture).  The binary is built where the reference tree
    is mounted and travels with the snapshot."""
    if not os.path.exists(EXE_CAL):
        pytest.skip("oracle/_ref/test_integration_calibrate.bin was not built (needs the reference tree)")
    from direct_visual_lidar_calibration_amd import se3
    from test_reference_golden import CASES

    c = CASES[0]
    path = _scene_file(tmp_path)
    # the reference prints "cost:<value>" on every improvement (visual_camera_calibration.cpp:115); the result is the last line
    out = subprocess.check_output([EXE_CAL, str(path), str(int(c["nm_bins"]))]).decode().strip().splitlines()
    vals = [float(v) for v in out[-1].split()]
    assert len(vals) == 17 and vals[16] >= 1, out[-1]  # 16 matrix entries + the number of callback invocations
    T = np.array(vals[:16]).reshape(4, 4)
    dt, dr = se3.delta_trans_rot(se3.from_matrix(c["ref_nm_T_camera_lidar"]), se3.from_matrix(T))
    assert dt <= 1e-3 and dr <= 1e-3, (dt, dr)
