"""csrc/orb_extract_plan.h, the extractor's frame-size planner, compiled for the host
(tests/native/extract_plan_host.cpp -> build/libextract_plan_host.so).

The table of tests/pyramid_cases.py (plan / no plan / K0, recorded on an MI355X) and
tests/golden/extract_plan_digests.json (a digest of every table and of the scalar fields per geometry,
recorded from the planner's statements as they stood inside orb_hip.hip, with only the HIP allocation,
copy and free calls stubbed out) are what the planner must reproduce.  The refusals, the assertions of
test_gpu_pyramid_geometry.py::test_plans_match_the_table and the invariants are stated in the C++
source, each check returning the line of the first expectation that fails; the same source runs as a
program under AddressSanitizer and UBSan."""
import ctypes
import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import pyramid_cases as pc

ROOT = pathlib.Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "extract_plan_digests.json"
HARRIS_SCORE, FAST_SCORE, FT_CL = 0, 1, 256


class PlanCase(ctypes.Structure):
    _fields_ = [("w", ctypes.c_int), ("h", ctypes.c_int), ("nf", ctypes.c_int), ("sf", ctypes.c_float),
                ("nl", ctypes.c_int), ("score", ctypes.c_int), ("fast_th", ctypes.c_int),
                ("max_batch", ctypes.c_int), ("fast_cl", ctypes.c_int)]


def plan_case(W, H, nf, sf=1.2, nl=8, score=FAST_SCORE, max_batch=1, fast_cl=FT_CL):
    return PlanCase(W, H, nf, sf, nl, score, 20, max_batch, fast_cl)


# the three geometries of test_gpu_pyramid_stream.py::OTHER_GEOMETRIES_PLAN, all with a stream plan
OTHER_GEOMETRIES = {"1920x1080": plan_case(1920, 1080, 3000), "1024x768_sf1.5_L5": plan_case(1024, 768, 1500, 1.5, 5),
                    "800x600_sf1.25_L7": plan_case(800, 600, 1200, 1.25, 7)}


def golden_cases():
    """name -> PlanCase of every geometry of the golden file."""
    out = {c.name: plan_case(c.W, c.H, c.nf, c.sf, c.nl) for c in pc.ALL_CASES}
    out.update(OTHER_GEOMETRIES)
    out.update({"640x480": plan_case(640, 480, 1000), "1241x376": plan_case(1241, 376, 2000),
                "1280x720": plan_case(1280, 720, 2000), "320x240": plan_case(320, 240, 500),
                "640x480_harris": plan_case(640, 480, 1000, score=HARRIS_SCORE),
                "640x480_batch512": plan_case(640, 480, 1000, max_batch=512),
                "640x480_fastcl8": plan_case(640, 480, 1000, fast_cl=8)})
    return out


@pytest.fixture(scope="module")
def L():
    return ctypes.CDLL(str(ROOT / "build" / "libextract_plan_host.so"))


@pytest.fixture(scope="module")
def golden():
    return {g["name"]: g for g in json.loads(GOLDEN.read_text())}


def query(L, case):
    """The planner's answer to what the handle's getters report: a dict."""
    msg, why = ctypes.create_string_buffer(256), ctypes.create_string_buffer(256)
    fpl, nq, nw, ring = (np.zeros(16, np.int32) for _ in range(4))
    scale = np.zeros(16, np.float32)
    ints = [ctypes.c_int() for _ in range(5)]  # max keypoints, stream, k0, rounds, lds
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    code = L.extract_plan_query(ctypes.byref(case), msg, p(fpl), p(scale), ctypes.byref(ints[0]),
                                *(ctypes.byref(i) for i in ints[1:]), p(nq), p(nw), p(ring), why)
    n = case.nl if ints[1].value else 0
    return dict(code=code, msg=msg.value.decode(), why=why.value.decode(), features_per_level=fpl[:case.nl].tolist(),
                scale=scale[:case.nl].tolist(), max_keypoints=ints[0].value, stream=ints[1].value, k0=ints[2].value,
                rounds=ints[3].value, lds=ints[4].value,
                levels=[(int(nq[l]), int(nw[l]), int(ring[l])) for l in range(n)])


def test_the_recorded_table(L, golden):
    """Every case of pyramid_cases.ALL_CASES: the recorded expect and K0, the assertions of
    test_plans_match_the_table (level sizes from the oracle's pyramid), the recorded reason of the two
    level-count cases; and the three OTHER_GEOMETRIES_PLAN entries."""
    k0s, hoisted, per_round = set(), [], []
    assert len(pc.ALL_CASES) == 118 and all(c.expect != pc.REFUSED for c in pc.ALL_CASES)
    for case in pc.ALL_CASES:
        c = plan_case(case.W, case.H, case.nf, case.sf, case.nl)
        q = query(L, c)
        assert q["code"] == 0, f"{case.name}: {q['msg']}"
        assert q["stream"] == (case.expect == pc.PLAN), f"{case.name}: stream plan {q['stream']}, expected '{case.expect}'"
        g = golden[case.name]  # the parent's own answer agrees with the table recorded on the GPU
        assert (g["code"], g["stream"], g["k0"] or None) == (0, q["stream"], case.k0), case.name
        line = L.extract_plan_check_table_row(ctypes.byref(c), q["stream"], case.k0 or 0)
        assert line == 0, f"{case.name}: the expectation at tests/native/extract_plan_host.cpp:{line} does not hold"
        if not q["stream"]:
            assert q["levels"] == [] and q["why"] == case.why, f"{case.name}: '{q['why']}'"
            continue
        k0, nr, lds, lv = q["k0"], q["rounds"], q["lds"], q["levels"]
        assert k0 == case.k0 and q["why"] == "", f"{case.name}: K0 {k0}, recorded {case.k0}"
        assert nr >= (case.H + k0 - 1) // k0 and 0 < lds <= 76 * 1024
        assert len(lv) == case.nl and sum(nw for _, nw, _ in lv) <= 14 and all(nw >= 1 for _, nw, _ in lv)
        if case.nl >= 13:
            assert [nw for _, nw, _ in lv][1:] == [1] * (case.nl - 1)
        sizes = pc.level_sizes(case)
        for l, (nq, nw, ring) in enumerate(lv):
            pitch = (sizes[l][0] + 32 + 15) & ~15
            assert nq == (pitch // 16 if l == 0 else pitch // 4), f"{case.name} level {l}"
            assert (1 <= ring <= min(255, sizes[l][1])) if l + 1 < case.nl else ring == 0, f"{case.name} level {l}"
            if l >= 1:
                (hoisted if nq <= 64 * nw else per_round).append((case.name, l))
        k0s.add(k0)
    assert len(k0s) >= 5 and hoisted and per_round
    assert {c.name for c in pc.ALL_CASES if c.expect == pc.NO_PLAN} == {"140x134_nf700_sf1.1_L15", "160x150_nf800_sf1.1_L16"}
    for name, c in OTHER_GEOMETRIES.items():
        assert query(L, c)["stream"] == 1 and golden[name]["stream"] == 1, name


def test_refusals(L):
    line = L.extract_plan_check_refusals()
    assert line == 0, f"the expectation at tests/native/extract_plan_host.cpp:{line} does not hold"


def test_every_table_against_the_recorded_digests(L, golden):
    cases = golden_cases()
    assert set(cases) == set(golden) and len(cases) == 118 + 10
    buf = ctypes.create_string_buffer(1 << 14)
    for name, c in cases.items():
        assert L.extract_plan_describe(name.encode(), ctypes.byref(c), buf, len(buf)) > 0
        got, want = json.loads(buf.value), golden[name]
        assert set(got["digests"]) == set(want["digests"]), name
        bad = [k for k in want["digests"] if got["digests"][k] != want["digests"][k]]
        assert not bad and got == want, f"{name}: {bad or 'parameters or scalars'} differ from the recorded plan"
        assert len(want["digests"]) == (12 if want["stream"] else 7), name


def test_invariants(L):
    for name, c in golden_cases().items():
        line = L.extract_plan_check_invariants(ctypes.byref(c))
        assert line == 0, f"{name}: the expectation at tests/native/extract_plan_host.cpp:{line} does not hold"


def test_sanitized_program(tmp_path):
    """The same source as a stand-alone program under AddressSanitizer and UBSan with libstdc++'s
    assertions: the refusals, every golden line, the table rows and the invariants."""
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge

    exe = tmp_path / "extract_plan_host_san"
    subprocess.run(ge.EXTRACT_PLAN_HOST_CMD(exe, ("-DEXTRACT_PLAN_HOST_MAIN", "-g", "-fsanitize=address,undefined",
                                                  "-fno-sanitize-recover=all", "-D_GLIBCXX_ASSERTIONS")), check=True)
    r = subprocess.run([str(exe), str(GOLDEN)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "128 geometries, status 0" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr
