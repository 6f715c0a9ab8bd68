"""The oracle and the pure-Python restatement on the SearchForInitialization gate tables
(tests/sfi_gate_tables.py): every row's dictated vnMatches12 entry, on the first call; the two
restatements against each other on the second call, which reads the vbPrevMatched the first
wrote.  Plus the tables' own guards: a row for every gate, side and direction the tables promise,
the exact-rescan precondition from the scene alone, and the ComputeThreeMaxima populations.

No row is skipped or filtered: a row that cannot be constructed is taken out of the builder, with
a sentence there saying why.
"""
import numpy as np
import pytest

import sfi_gate_tables as S
from oracle_lib import lib, search_for_initialization
from test_matcher_oracle import PyFrame, hamming, py_search_for_initialization

NNRATIO = 0.9
TABLES = S.all_tables()
IDS = [repr(t) for t in TABLES]


def run_oracle(T, b, prev):
    return search_for_initialization(b["k1"], b["d1"], b["k2"], b["d2"], 0, 0, prev, NNRATIO, T.ori, T.window,
                                     bounds=T.bounds)


def run_python(T, b, prev):
    F1 = PyFrame(b["k1"], b["d1"], 0, 0, T.bounds)
    F2 = PyFrame(b["k2"], b["d2"], 0, 0, T.bounds)
    return py_search_for_initialization(F1, F2, prev, NNRATIO, T.ori, T.window)


def report(T, b, got, who):
    l1, l2 = b["lead1"], b["lead2"]
    bad = [f"{r}: {who} {got[l1 + i] - l2 if got[l1 + i] >= 0 else -1}, dictated {r.expect}"
           for i, r in enumerate(T.rows) if got[l1 + i] != b["m12"][l1 + i]]
    assert not bad, "%d row(s) differ:\n%s" % (len(bad), "\n".join(bad))
    np.testing.assert_array_equal(got, b["m12"])


@pytest.mark.parametrize("lead1,lead2", [(0, 0), (7, 5)])
@pytest.mark.parametrize("T", TABLES, ids=IDS)
def test_rows_oracle_and_python(T, lead1, lead2):
    b = T.build(lead1, lead2)
    po, pp = b["prev"].copy(), b["prev"].copy()
    no, mo = run_oracle(T, b, po)
    npy, mp = run_python(T, b, pp)
    report(T, b, mo, "oracle")
    report(T, b, mp, "python")
    assert no == npy == b["n"]
    assert po.tobytes() == pp.tobytes()
    # vbPrevMatched: the matched keypoint's position, untouched elsewhere (NaN rows keep their bits)
    exp = b["prev"].copy()
    hit = b["m12"] >= 0
    exp[hit, 0], exp[hit, 1] = b["k2"]["x"][b["m12"][hit]], b["k2"]["y"][b["m12"][hit]]
    assert po.tobytes() == exp.tobytes()
    # the second call reads the updated vbPrevMatched
    no2, mo2 = run_oracle(T, b, po)
    np2, mp2 = run_python(T, b, pp)
    assert no2 == np2
    np.testing.assert_array_equal(mo2, mp2)
    assert po.tobytes() == pp.tobytes()


def test_guards_every_gate_side_and_direction():
    keys = {(t.rect, t.window) + r.inp["key"] for t in TABLES for r in t.rows}
    want = set()
    for rect in "AB":
        for w in (100, 40):
            for d in S.DIRS:
                for side in ("below", "on", "above"):
                    want |= {(rect, w, "box", side, d), (rect, w, "box second", side, d)}
        for d in S.DIRS:
            want.add((rect, 0, "box", "above", d))
            for side in ("below", "on", "above"):
                want.add((rect, 100, "rescan box", side, d))
            want |= {(rect, 40, "cells clamped", "in", d), (rect, 40, "cells outside the grid", "out", d)}
        want |= {(rect, 0, "box", "on", "0"), (rect, 10000, "cells whole grid", "in", "0")}
        for g, d in (("column", "-x"), ("column", "+x"), ("row", "-y"), ("row", "+y")):
            f = "first" if d[0] == "-" else "last"
            want |= {(rect, 40, f"cells {f} {g}", "in", d), (rect, 40, f"rescan cells {f} {g}", "in", d)}
        want |= {(rect, 8, "cells sparse first column", "in", "-x"), (rect, 8, "cells sparse last column", "in", "+x")}
        want |= {(rect, 40, "level F2 octave 1", "out", "0"), (rect, 40, "level F1 octave 1", "out", "0"),
                 (rect, 40, "level F1 octave 1 on an octave-1 keypoint", "out", "0"),
                 (rect, 40, "steal at equal distance", "on", "0")}
        for side in ("nan", "inf", "1e12"):
            for g in ("x", "y", "x and y"):
                want.add((rect, 40, "nonfinite prev " + g, side, "-" + g[0]))
                if side != "nan":
                    want.add((rect, 40, "nonfinite prev " + g, side, "+" + g[0]))
        want |= {(rect, 40, "nonfinite F2 keypoint", "nan", "-x"), (rect, 40, "nonfinite F2 keypoint", "inf", "-x")}
    want.add(("A", 0, "cells one cell", "on", "0"))
    missing = want - keys
    assert not missing, sorted(missing)
    # PosInGrid: on each rectangle and edge one keypoint outside the grid and the adjacent float inside
    for t in TABLES:
        if t.name != "window":
            continue
        for d in ("-x", "+x", "-y", "+y"):
            rows = [r for r in t.rows if r.inp["key"][0].startswith("posingrid") and "interior" not in r.inp["key"][0]
                    and r.inp["key"][2] == d]
            assert sorted(r.inp["in"] for r in rows) == [False, True], (t, d)
        if t.rect == "A":  # exact: the outside rows sit on -0.5 / last + 0.5
            sides = {r.inp["key"][1:] for r in t.rows if r.inp["key"][0].startswith("posingrid") and not r.inp.get("in", True)}
            assert sides == {("on", d) for d in ("-x", "+x", "-y", "+y")}
    # rotation bins: every boundary 15 .. 345 with its three sides, and the three special inputs
    rot = {r.inp["key"][1:] for t in TABLES for r in t.rows if r.inp["key"][0] == "rotbin"}
    for k in range(12):
        assert {(s, str(15 + 30 * k)) for s in ("below", "on", "above")} <= rot
    assert {("on", "-0"), ("denormal", "360"), ("on", "-15")} <= rot
    # both kinds of rectangle carry orientation tables
    assert {t.rect for t in TABLES if t.ori} == {"A", "B"}


def test_rescan_precondition():
    """From the scene alone: at the row's turn the eight best of its in-window candidates by
    (distance, traversal order) are each held at a distance no larger than the row's own, and more
    than eight candidates are in the window: the truncated top-8 has no live entry."""
    n = 0
    for T in TABLES:
        if not T.rescans:
            continue
        b = T.build()
        F2 = PyFrame(b["k2"], b["d2"], 0, 0, T.bounds)
        for qi in T.rescans:
            cand = F2.area(b["prev"][qi, 0], b["prev"][qi, 1], T.window, 0, 0)
            assert len(cand) >= 10, (T, qi, len(cand))
            ranked = sorted(range(len(cand)), key=lambda o: (hamming(b["d1"][qi], b["d2"][cand[o]]), o))[:8]
            for o in ranked:
                i2 = cand[o]
                d = hamming(b["d1"][qi], b["d2"][i2])
                holders = [i1 for i1 in range(qi) if b["k1"]["octave"][i1] == 0 and hamming(b["d1"][i1], b["d2"][i2]) == 0
                           and b["prev"][i1, 0] == b["k2"]["x"][i2] and b["prev"][i1, 1] == b["k2"]["y"][i2]]
                # a holder at distance 0 on the keypoint accepts it (0 < 0.9 * second for any second > 0:
                # no two F2 descriptors of the window are equal) and nothing can take it back
                assert holders and 0 <= d, (T, qi, i2)
            D = [hamming(b["d2"][a], b["d2"][c]) for a in cand for c in cand if a != c]
            assert min(D) > 0
            n += 1
    assert n >= 2 * (12 + 4)


def test_three_maxima_populations():
    """The orientation tables' bins hold what they claim, counted with the oracle's own rot_bin
    over every accepting query (robbed ones included)."""
    L = lib()
    seen = 0
    for T in TABLES:
        if T.maxima is None:
            continue
        b = T.build()
        hist = {}
        for i, e in enumerate(T.q):
            if e.accepts is None:
                continue
            i2 = b["off"][e.accepts]
            bn = L.oracle_rot_bin(float(b["k1"]["angle"][i]), float(b["k2"]["angle"][i2]))
            hist[bn] = hist.get(bn, 0) + 1
        assert hist == T.maxima[0], (T, hist)
        kept = {L.oracle_rot_bin(float(b["k1"]["angle"][i]), float(b["k2"]["angle"][b["m12"][i]]))
                for i in range(len(T.q)) if b["m12"][i] >= 0}
        assert tuple(sorted(kept)) == T.maxima[1], (T, kept)
        seen += 1
    assert seen == 16
