"""The drop-in boundary without a GPU: libraries load, every declared C symbol is exported,
argument validation fails loudly, and host-only entry points work."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

import orbslam_jpminipc_amd as orb
from orbslam_jpminipc_amd import _native

ROOT = pathlib.Path(__file__).resolve().parent.parent


def declared_functions(header: pathlib.Path):
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    return sorted(set(re.findall(r"^[A-Za-z_][\w \*]*?\b(orb_\w+|oracle_\w+)\s*\(", text, flags=re.M)))


def exported(so: pathlib.Path):
    lib = ctypes.CDLL(str(so))
    return lib


def test_hip_library_exports_every_abi_symbol():
    names = declared_functions(ROOT / "include" / "orb_abi.h")
    assert "orb_extract" in names and "orb_search_for_initialization_batch_device" in names
    # the test / diagnostic hooks live in their own header, outside the reference-facing ABI
    debug = declared_functions(ROOT / "include" / "orb_debug.h")
    assert debug and all(n.startswith("orb_debug_") for n in debug)
    assert not [n for n in names if n.startswith("orb_debug_")]
    names = names + debug
    lib = orb.hip_lib()
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    # the Python binding table covers the whole header
    assert set(names) <= set(_native.HIP_SIGNATURES)


def test_oracle_library_exports_every_symbol():
    names = declared_functions(ROOT / "oracle" / "orb_oracle.h")
    lib = exported(ROOT / "oracle" / "liborb_oracle.so")
    assert [n for n in names if not hasattr(lib, n)] == []


def test_version_string():
    assert orb.hip_lib().orb_version().decode().startswith("orb_hip gfx950")


def test_bad_parameters_fail_loudly():
    with pytest.raises(orb.OrbError) as e:
        orb.ORBextractor(0, 1.2, 8)
    assert e.value.code == _native.ORB_EINVAL
    with pytest.raises(orb.OrbError):
        orb.ORBextractor(1000, 1.0, 8)  # scaleFactor must be > 1
    with pytest.raises(orb.OrbError):
        orb.ORBextractor(1000, 1.2, 99)


def test_product_does_not_reference_the_oracle():
    # the product library and package never load or link the checker
    so = (ROOT / "orbslam_jpminipc_amd" / "liborb_hip.so").read_bytes()
    assert b"liborb_oracle" not in so and b"oracle_extract" not in so
    for py in (ROOT / "orbslam_jpminipc_amd").glob("*.py"):
        assert "oracle" not in py.read_text().replace("oracle/", ""), py


def test_keypoint_record_layout():
    assert _native.KEYPOINT_DTYPE.itemsize == 28
    assert [f for f in _native.KEYPOINT_DTYPE.names] == ["x", "y", "size", "angle", "response", "octave", "class_id"]


def test_synth_is_deterministic_and_consecutive_frames_overlap():
    a = orb.synth_stream(320, 240, stream=3, first=0, count=3)
    b = orb.synth_stream(320, 240, stream=3, first=1, count=2)
    assert np.array_equal(a[1:], b)
    c = orb.synth_stream(320, 240, stream=4, first=0, count=1)
    assert not np.array_equal(a[0], c[0])
    # frame t+1 is frame t shifted by (dx, dy) in [-6, 6]^2 up to the +-8 noise
    f0, f1 = a[0].astype(int), a[1].astype(int)
    best = min(
        (np.abs(f0[16:-16, 16:-16] - f1[16 + dy:224 + dy, 16 + dx:304 + dx]).mean(), dx, dy)
        for dx in range(-6, 7) for dy in range(-6, 7))
    assert best[0] < 6.0
    assert orb.synth_special(orb.SYN_FLAT, 64, 48).max() == 128


def test_cpp_facade_compiles_and_fails_loudly(tmp_path):
    """include/orb_slam_gpu.hpp (the reference-class facade) builds against liborb_hip.so."""
    import subprocess

    pkg = ROOT / "orbslam_jpminipc_amd"
    exe = tmp_path / "orb_facade_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), str(ROOT / "tests/native/facade_check.cpp"),
                    f"-L{pkg}", "-lorb_hip", f"-Wl,-rpath,{pkg}", "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_matcher_family_validates_before_device_work():
    """Bad views, flag arrays and FeatureVectors fail with ORB_EINVAL/ENOTSUP on any host."""
    from orbslam_jpminipc_amd.views import FeatureVector, View

    k = np.zeros(3, orb.KEYPOINT_DTYPE)
    k["octave"] = [0, 1, 9]  # octave 9 >= nlevels
    V = View(k, np.zeros((3, 32), np.uint8))
    m = orb.ORBmatcher(0.9, True)
    with pytest.raises(orb.OrbError) as e:
        m.WindowSearch(V, None, V, 100)
    assert e.value.code == _native.ORB_EINVAL
    k["octave"] = 0
    V = View(k, np.zeros((3, 32), np.uint8), bounds=(0, 0, 0, 480))  # empty bounds
    with pytest.raises(orb.OrbError):
        m.WindowSearch(V, None, V, 100)
    V = View(k, np.zeros((3, 32), np.uint8))
    bad = FeatureVector([5, 3], [0, 1, 2], [0, 1])  # node ids not ascending
    good = FeatureVector([3, 5], [0, 1, 3], [0, 1, 2])
    with pytest.raises(orb.OrbError) as e:
        m.SearchByBoW_KF_KF(V, None, bad, V, None, good)
    assert e.value.code == _native.ORB_EINVAL
    oob = FeatureVector([3], [0, 1], [7])  # feature index out of range
    with pytest.raises(orb.OrbError):
        m.SearchByBoW_KF_F(V, None, oob, V, good)
