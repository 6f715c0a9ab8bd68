"""gpu::KeyFrameDatabase of include/orb_slam_gpu.hpp on the GPU: build/kfdb_facade
(tests/native/kfdb_facade.cpp, built by __graft_entry__.build()) drives the C++ facade on
scenarios with answers known by construction and reports through its exit status."""
import pathlib
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.mark.gpu
def test_cpp_kfdb_facade_on_gpu():
    exe = ROOT / "build" / "kfdb_facade"
    if not exe.exists():  # build() makes it; a tree that skipped build() compiles it here (g++, seconds)
        import __graft_entry__ as ge

        exe.parent.mkdir(exist_ok=True)
        subprocess.run(ge.KFDB_FACADE_CMD(exe), check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "kfdb facade OK" in r.stdout, r.stdout + r.stderr
