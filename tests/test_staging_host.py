"""csrc/orb_staging.h, the layout of the host calls' arenas and of the batch forms' scratch blocks, and
csrc/orb_initializer_scratch.h, compiled for the host (tests/native/staging_host.cpp ->
build/libstaging_host.so).

The expectations are in the C++ source, one function per subject, each returning the line of the
first one that fails; this file runs them, repeats the four-region sweep with an alignment chain
written here, and runs the same source as a program under AddressSanitizer and UBSan.  That a
pointer cannot be had before the arena is reserved is a static_assert there: it does not compile."""
import ctypes
import itertools
import pathlib
import subprocess
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CHECKS = ["staging_check_chain4", "staging_check_cases", "staging_check_chain_subsets", "staging_check_rec_subsets",
          "staging_check_stage"]


@pytest.fixture(scope="module")
def L():
    return ctypes.CDLL(str(ROOT / "build" / "libstaging_host.so"))


@pytest.mark.parametrize("name", CHECKS)
def test_check(L, name):
    fn = getattr(L, name)
    fn.restype = ctypes.c_int
    assert fn() == 0, f"{name}: the expectation at tests/native/staging_host.cpp:{fn()} does not hold"


def test_four_regions_against_the_alignment_chain(L):
    """Byte counts {0, 1, 255, 256, 257} in every position: the offsets are those of al(prev + bytes)."""
    al = lambda x: -(-x // 256) * 256  # noqa: E731
    A4, A5 = ctypes.c_size_t * 4, ctypes.c_size_t * 5
    for b in itertools.product([0, 1, 255, 256, 257], repeat=4):
        off = A5()
        L.staging_offsets4(A4(*b), off)
        want = [0]
        for x in b:
            want.append(al(want[-1] + x))
        assert list(off) == want, b
        assert all(want[k + 1] == want[k] for k in range(4) if b[k] == 0)  # no bytes, no room


def test_sanitized_program(tmp_path):
    """The same source as a stand-alone program under AddressSanitizer and UBSan, on buffers of exactly
    the planned sizes."""
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge

    exe = tmp_path / "staging_host_san"
    subprocess.run(ge.STAGING_HOST_CMD(exe, ("-DSTAGING_HOST_MAIN", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=all")), check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "status 0" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr
