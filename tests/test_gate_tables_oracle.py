"""The gate tables (tests/gate_tables.py) against the CPU oracle and, where
tests/test_matcher_family_oracle.py has one, against the pure-Python restatement (CPU only).

Each row dictates the decision its reference line makes on that side of the threshold; the
oracle has to make the same one.  This separates a wrong oracle (or a wrong table) from a wrong
kernel: tests/test_gpu_matcher_gates.py then holds the GPU to both.  Every row is asserted;
a failure lists all rows that disagree.
"""
import numpy as np
import pytest

import gate_tables as GT
from oracle_lib import OracleMatcher
from test_matcher_family_oracle import PyView, py_epipolar, py_fuse, py_is_in_frustum, py_sbp_local

NNRATIO = 0.9


def oracle():
    return OracleMatcher(NNRATIO, False)


def report(bad):
    assert not bad, "%d row(s) differ:\n%s" % (len(bad), "\n".join(bad))


def test_frustum_rows():
    groups = GT.frustum_table()
    assert sum(len(G.rows) for G in groups) >= 60
    bad = [f"{r}: oracle {got}, dictated {r.expect}" for r, got in GT.run_frustum(oracle(), groups)
           if not GT.same_frustum(got, r.expect)]
    with np.errstate(all="ignore"):
        for G in groups:
            ref = py_is_in_frustum(G.V, G.points(), G.limit)
            bad += [f"{r}: python {p}, dictated {r.expect}" for r, p in zip(G.rows, ref)
                    if not GT.same_frustum((p[0], p[3], p[1], p[2], p[4]), r.expect)]
    report(bad)


def test_area_rows():
    groups = GT.area_table()
    assert sum(len(G.rows) for G in groups) >= 120
    bad = [f"{r}: oracle {got}, dictated {r.expect}" for r, got in GT.run_area(oracle(), groups) if got != r.expect]
    with np.errstate(all="ignore"):
        for G in groups:
            P = PyView(G.V) if np.isfinite(G.V.kps["x"]).all() and np.isfinite(G.V.kps["y"]).all() else None
            for r in G.rows:
                i = r.inp
                if P is None or not all(np.isfinite(i[k]) and abs(i[k]) < 1e9 for k in "xyr"):
                    continue  # (int) of a NaN / inf / huge float: Python raises where x86 yields INT_MIN
                got = P.kf_area(i["x"], i["y"], i["r"]) if i["keyframe"] else P.area(i["x"], i["y"], i["r"], i["lo"], i["hi"])
                if got != r.expect:
                    bad.append(f"{r}: python {got}, dictated {r.expect}")
    report(bad)


CALLS = GT.matcher_calls()


@pytest.mark.parametrize("mode,S", [c[1:] for c in CALLS], ids=[c[0] for c in CALLS])
def test_matcher_rows(mode, S):
    n, out, exp = GT.run_scene(oracle(), mode, S)
    bad = []
    for i, r in enumerate(S.rows):
        got = out[i] == i  # target i <-> query i, whichever side the matcher reports by
        if got != r.expect:
            bad.append(f"{r}: oracle {'matched' if got else 'no match'}")
    report(bad)
    np.testing.assert_array_equal(out, exp)
    assert n == sum(r.expect for r in S.rows)
    # the pure-Python restatements of the same two families
    b = S.build()
    with np.errstate(all="ignore"):
        if mode == "local":
            ref = py_sbp_local(b["T"], np.zeros(b["T"].n, np.uint8), np.ones(b["n"], np.uint8), b["u"], b["v"], b["level"],
                               b["vc"], b["qd"], S.th, NNRATIO)
            np.testing.assert_array_equal(ref[1], exp)
        if mode in ("fuse", "fuse_scw"):
            ref = py_fuse(b["T"], b["pts"], np.ones(b["n"], np.uint8), S.th, mode == "fuse_scw")
            np.testing.assert_array_equal(ref[1], exp)


def test_triangulation_rows():
    groups = GT.triangulation_table()
    bad = []
    for G in groups:
        n, out, exp = GT.run_triangulation(oracle(), G)
        for i, r in enumerate(G.rows):
            if (out[i] == i) != r.expect:
                bad.append(f"{r}: oracle {out[i]}")
            k1, k2 = (GT.kps_at([k[0]], [k[1]], [k[2]])[0] for k in (r.inp["k1"], r.inp["k2"]))
            with np.errstate(all="ignore"):
                if bool(py_epipolar(k1, k2, G.F12, GT.SIGMA2)) != r.expect:
                    bad.append(f"{r}: python disagrees")
        np.testing.assert_array_equal(out, exp)
        assert n == sum(r.expect for r in G.rows)
    report(bad)


def test_embedded_tables_keep_their_rows():
    """The embedded form (LEAD fillers in front) shifts every expectation by LEAD and matches
    nothing more: the oracle gives the same verdicts."""
    o = oracle()
    for _, mode, S in CALLS[:: max(1, len(CALLS) // 6)]:
        n, out, exp = GT.run_scene(o, mode, S, GT.LEAD)
        np.testing.assert_array_equal(out, exp)
    for G in GT.triangulation_table():
        n, out, exp = GT.run_triangulation(o, G, GT.LEAD)
        np.testing.assert_array_equal(out, exp)
    for (r, a), (_, b) in zip(GT.run_frustum(o, GT.frustum_table(), GT.LEAD), GT.run_frustum(o, GT.frustum_table())):
        assert GT.same_frustum(a, b), str(r)
