"""Host tests of the LAS map route: ``dataset.read_las_header`` against the struct parser of tests/las_oracle.py, its refusals, the
``--map_origin auto`` rule, the option handling of ``preprocess_map`` and the argument checks of ``nidreg_integrator_insert_las``,
which all run before a device is touched (no GPU here)."""
import ctypes
import struct

import numpy as np
import pytest

import las_oracle as lo
from direct_visual_lidar_calibration_amd import _lib, dataset, preprocess_map

SCALE, OFFSET = (0.001, 1e-4, 0.01), (500000.0, 4000000.0, 120.0)


def records(point_format, n, extra=0, seed=1):
    rng = np.random.default_rng(seed)
    X, Y, Z = rng.integers(-(2**31), 2**31, (3, n))
    rgb = rng.integers(0, 65536, (n, 3)) if point_format in lo.RGB_OFFSET else None
    return lo.pack_records(point_format, X, Y, Z, rng.integers(0, 65536, n), rng.integers(0, 32, n), rng.integers(0, 2, n), rgb, extra, rng)


@pytest.mark.parametrize("point_format", range(11))
def test_header_fields_of_every_format_and_version(tmp_path, point_format):
    for minor in range(5):
        extra = (0, 3)[(minor + point_format) % 2]
        rec = records(point_format, 7, extra)
        path = str(tmp_path / f"f{point_format}_v{minor}.LAS")
        lo.write_las(path, point_format, rec, SCALE, OFFSET, minor=minor, vlr_bytes=54 * (minor % 2))
        with open(path, "rb") as f:
            want = lo.parse_header(f.read())
        got = dataset.read_las_header(path)
        assert got == want
        assert got["version"] == (1, minor) and got["point_format"] == point_format and got["record_length"] == lo.BASE_LENGTH[point_format] + extra
        assert got["num_points"] == 7 and got["header_size"] == lo.HEADER_SIZE[minor] and got["point_offset"] == got["header_size"] + 54 * (minor % 2)
        assert got["scale"] == SCALE and got["offset"] == OFFSET and all(a <= b for a, b in zip(got["min"], got["max"]))
        chunks = list(dataset.read_las_chunks(path, got, chunk_points=3))
        assert [c.size for c in chunks] == [3 * rec.shape[1]] * 2 + [rec.shape[1]] and np.array_equal(np.concatenate(chunks), rec.reshape(-1))


def test_the_64_bit_count_is_used_when_it_is_not_zero(tmp_path):
    rec = records(6, 5)
    path = str(tmp_path / "a.las")
    lo.write_las(path, 6, rec, SCALE, OFFSET, minor=4, legacy_count=0)  # a 1.4 file with formats 6+ leaves the legacy count zero
    assert dataset.read_las_header(path)["num_points"] == 5
    lo.write_las(path, 1, records(1, 5), SCALE, OFFSET, minor=4, legacy_count=5, count64=0)
    assert dataset.read_las_header(path)["num_points"] == 5
    lo.write_las(path, 1, records(1, 5), SCALE, OFFSET, minor=4, legacy_count=2, count64=4)
    assert dataset.read_las_header(path)["num_points"] == 4
    # in a 1.3 file those bytes are not a count, whatever they hold
    lo.write_las(path, 1, records(1, 5), SCALE, OFFSET, minor=3, legacy_count=5, vlr_bytes=200)
    assert dataset.read_las_header(path)["num_points"] == 5


def _file(tmp_path, name="r.las", point_format=3, n=4, patch=None, cut=None, **kw):
    path = str(tmp_path / name)
    lo.write_las(path, point_format, records(point_format, n), kw.pop("scale", SCALE), kw.pop("offset", OFFSET), **kw)
    data = bytearray(open(path, "rb").read())
    for at, fmt, value in patch or ():
        struct.pack_into(fmt, data, at, value)
    with open(path, "wb") as f:
        f.write(data[:cut] if cut is not None else data)
    return path


def test_header_refusals_name_what_was_found(tmp_path):
    with pytest.raises(ValueError, match=r"not a LAS file \(signature b'LASX'"):
        dataset.read_las_header(_file(tmp_path, signature=b"LASX"))
    with pytest.raises(ValueError, match="LAS version 2.0"):
        dataset.read_las_header(_file(tmp_path, major=2, patch=[(25, "<B", 0)]))
    with pytest.raises(ValueError, match="LAS version 1.5"):
        dataset.read_las_header(_file(tmp_path, patch=[(25, "<B", 5)]))
    for byte in (0x80 | 3, 0x40 | 3, 0xC0 | 1):
        with pytest.raises(ValueError, match=r"compressed LAS \(LAZ\) is not read"):
            dataset.read_las_header(_file(tmp_path, format_byte=byte))
    with pytest.raises(ValueError, match="point format 11"):
        dataset.read_las_header(_file(tmp_path, format_byte=11))
    with pytest.raises(ValueError, match="record length 33 is below the 34 bytes of point format 3"):
        dataset.read_las_header(_file(tmp_path, patch=[(105, "<H", 33)]))
    for bad in (0.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="zero or non-finite"):
            dataset.read_las_header(_file(tmp_path, scale=(0.001, bad, 0.001)))
    with pytest.raises(ValueError, match="offset .* is not finite"):
        dataset.read_las_header(_file(tmp_path, offset=(0.0, 0.0, float("-inf"))))
    with pytest.raises(ValueError, match="header size 60000 lies outside the file"):
        dataset.read_las_header(_file(tmp_path, patch=[(94, "<H", 60000)]))
    with pytest.raises(ValueError, match="offset to point data 100000 lies outside the file"):
        dataset.read_las_header(_file(tmp_path, patch=[(96, "<I", 100000)]))
    with pytest.raises(ValueError, match="truncated"):
        dataset.read_las_header(_file(tmp_path, cut=-1))
    with pytest.raises(ValueError, match="truncated"):
        dataset.read_las_header(_file(tmp_path, patch=[(107, "<I", 5)]))
    with pytest.raises(ValueError, match="truncated LAS header"):
        dataset.read_las_header(_file(tmp_path, cut=100))
    assert dataset.read_las_header(_file(tmp_path))["num_points"] == 4  # the unpatched file is read


def test_auto_origin_on_both_sides_of_1024_m_and_for_negative_bounds():
    auto = preprocess_map.las_auto_origin
    assert auto({"min": (-1024.0, -3.0, -1.0), "max": (1024.0, 1024.0, 20.0)}) == (0.0, 0.0, 0.0)
    assert auto({"min": (-10.0, -3.0, -1.0), "max": (np.nextafter(1024.0, 2000.0), 7.0, 20.0)}) == (507.0, 2.0, 9.0)
    assert auto({"min": (499900.25, 3999950.5, 95.0), "max": (500101.0, 4000050.0, 140.0)}) == (500000.0, 4000000.0, 117.0)
    # floor, not truncation: a negative middle goes down
    assert auto({"min": (-2000.5, -1.0, -0.75), "max": (-1000.0, 0.0, 0.25)}) == (-1501.0, -1.0, -1.0)
    assert auto({"min": (0.0, -1025.0, 0.0), "max": (1.0, -1024.5, 1.0)}) == (0.0, -1025.0, 0.0)
    with pytest.raises(ValueError, match="--map_origin x,y,z"):
        auto({"min": (0.0, 0.0, float("nan")), "max": (1.0, 1.0, 1.0)})


def test_resolve_map_origin(tmp_path):
    path = _file(tmp_path, "utm.las", mins=(499900.0, 3999900.0, 90.0), maxs=(500100.5, 4000100.0, 131.0))
    assert preprocess_map.resolve_map_origin(path) == (500000.0, 4000000.0, 110.0)
    assert preprocess_map.resolve_map_origin(path, (1.5, -2.0, 3.0)) == (1.5, -2.0, 3.0)
    assert preprocess_map.resolve_map_origin(_file(tmp_path, "near.LAS", mins=(-5.0, -5.0, -1.0), maxs=(60.0, 5.0, 9.0))) == (0.0, 0.0, 0.0)
    assert preprocess_map.resolve_map_origin(str(tmp_path / "none.ply")) == (0.0, 0.0, 0.0)  # PLY / PCD: nothing is read for auto


def test_option_parsing_and_refusals(tmp_path):
    assert preprocess_map.parse_map_origin("auto") is None and preprocess_map.parse_map_origin(" AUTO ") is None
    assert preprocess_map.parse_map_origin("-500000.5,4e6,12") == (-500000.5, 4000000.0, 12.0)
    for bad in ("1,2", "1,2,3,4", "a,b,c", "1,2,nan", "1,,3", ""):
        with pytest.raises(ValueError, match="--map_origin must be"):
            preprocess_map.parse_map_origin(bad)
    assert preprocess_map.parse_classes(None) == () and preprocess_map.parse_classes("7,18") == (7, 18)
    for bad in ("7,256", "-1", "x", "7,,18"):
        with pytest.raises(ValueError, match="--las_exclude_classes must be"):
            preprocess_map.parse_classes(bad)
    # the value of --map_origin may start with a minus sign: it is attached with '=' like the two list options
    argv = preprocess_map._attach_values(["--map_origin", "-12.5,3,4", "--camera_intrinsics", "-1,2", "--las_keep_withheld"])
    assert argv == ["--map_origin=-12.5,3,4", "--camera_intrinsics=-1,2", "--las_keep_withheld"]
    args = preprocess_map.build_parser().parse_args(argv + ["--las_exclude_classes", "7,18", "--map_intensity", "rgb"])
    assert (args.map_origin, args.las_exclude_classes, args.map_intensity, args.las_keep_withheld) == ("-12.5,3,4", "7,18", "rgb", True)
    defaults = preprocess_map.build_parser().parse_args([])
    assert (defaults.map_origin, defaults.las_exclude_classes, defaults.map_intensity, defaults.las_keep_withheld) == ("auto", None, None, False)
    with pytest.raises(SystemExit):
        preprocess_map.build_parser().parse_args(["--map_intensity", "nir"])
    # a LAS-only option with another map format is refused by its name, before the map is read
    for kw, name in (({"map_intensity": "intensity"}, "--map_intensity"), ({"las_exclude_classes": (7,)}, "--las_exclude_classes"), ({"las_keep_withheld": True}, "--las_keep_withheld")):
        for ext in ("ply", "pcd"):
            with pytest.raises(ValueError, match=f"{name} is an option for LAS maps"):
                preprocess_map.load_lidar_points(str(tmp_path / f"absent.{ext}"), 0.002, **kw)


def test_main_reports_a_bad_map_origin_and_a_las_option_on_a_ply(tmp_path, capsys):
    image = str(tmp_path / "i.png")
    dataset.write_png_gray(image, np.arange(64, dtype=np.uint8).reshape(8, 8))
    base = ["--image_path", image, "--dst_path", str(tmp_path / "d"), "--camera_model", "plumb_bob", "--camera_intrinsics", "10,10,4,4", "--camera_distortion_coeffs", ""]
    assert preprocess_map.main(base + ["--map_path", str(tmp_path / "m.ply"), "--map_origin", "1,2"]) == 1
    assert "--map_origin must be" in capsys.readouterr().err
    assert preprocess_map.main(base + ["--map_path", str(tmp_path / "m.ply"), "--las_exclude_classes", "7"]) == 1
    assert "--las_exclude_classes is an option for LAS maps" in capsys.readouterr().err
    path = _file(tmp_path, "one.las", point_format=1)
    assert preprocess_map.main(base + ["--map_path", path, "--map_intensity", "rgb"]) == 1
    assert "point format 1, which carries no colour" in capsys.readouterr().err


def _insert_las(h=None, records=b"\0" * 40, n=1, step=34, fmt=3, scale=(0.001,) * 3, offset=(0.0,) * 3, origin=(0.0,) * 3, source=0, mask=None, keep=0):
    lib = _lib.load()
    tri = [None if t is None else (ctypes.c_double * 3)(*t) for t in (scale, offset, origin)]
    skipped = ctypes.c_int64(-5)
    rc = lib.nidreg_integrator_insert_las(h, records, n, step, fmt, tri[0], tri[1], tri[2], source, mask, keep, ctypes.byref(skipped))
    return rc, _lib.last_error(), skipped.value


def test_abi_argument_checks_run_on_the_host_before_the_handle_is_looked_at():
    """every call passes a NULL integrator: a check of the arguments that ran after the handle's would report the handle"""
    cases = [
        ({"fmt": 11}, "point formats 0..10 are read, got 11"),
        ({"fmt": -1}, "point formats 0..10 are read, got -1"),
        ({"step": 33}, "record_length 33 is outside 34..65535"),
        ({"fmt": 10, "step": 66}, "record_length 66 is outside 67..65535"),
        ({"step": 65536}, "record_length 65536 is outside"),
        ({"scale": (0.001, 0.0, 0.001)}, "a scale must be finite and not zero"),
        ({"scale": (float("nan"), 1.0, 1.0)}, "a scale must be finite and not zero"),
        ({"offset": (0.0, float("inf"), 0.0)}, "non-finite offset or origin"),
        ({"origin": (0.0, 0.0, float("nan"))}, "non-finite offset or origin"),
        ({"fmt": 1, "step": 28, "source": 1}, "rgb intensity asked of point format 1"),
        ({"fmt": 6, "step": 30, "source": 1}, "rgb intensity asked of point format 6"),
        ({"source": 2}, "intensity_source must be 0"),
        ({"scale": None}, "null scale3, offset3 or origin3"),
        ({"origin": None}, "null scale3, offset3 or origin3"),
        ({"records": None}, "negative num_points or null records"),
        ({"n": -1}, "negative num_points or null records"),
        ({}, "null integrator"),
        ({"fmt": 3, "source": 1, "n": 0, "records": None}, "null integrator"),
    ]
    for kw, text in cases:
        rc, msg, skipped = _insert_las(**kw)
        assert rc == _lib.NIDREG_ERR_INVALID and "nidreg_integrator_insert_las" in msg and text in msg, (kw, msg)
        assert skipped == 0
