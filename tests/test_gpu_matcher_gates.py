"""GPU parity of the projection matchers' geometric gates (k_query_prep, enum_candidates /
k_area_fill, k_grid_build's cell_of, k_is_in_frustum, kf_in_image, predict_level, epipolar_ok
in csrc/orb_match.hip) exactly on their thresholds: the tables of tests/gate_tables.py, one
query per row on / next to a float comparison of the reference, or on a NaN / inf / denormal
input.

Every row is held to two things: the decision its reference line dictates (stated by the
table, confirmed for the oracle by tests/test_gate_tables_oracle.py) and the oracle's result.
Match arrays, counts, in_view and level are identical; float outputs are bit-identical where
the oracle's are finite and NaN where the oracle's are NaN.  Each table runs as built and
embedded after 250 fillers that match nothing, so that its rows straddle the 256-thread block
boundary of k_query_prep and k_is_in_frustum.  A failure lists every row that differs.
"""
import numpy as np
import pytest

import gate_tables as GT
import orbslam_jpminipc_amd as orb
from oracle_lib import OracleMatcher

pytestmark = pytest.mark.gpu

NNRATIO = 0.9
LEADS = [0, GT.LEAD]


def both():
    return orb.ORBmatcher(NNRATIO, False), OracleMatcher(NNRATIO, False)


def report(bad):
    assert not bad, "%d row(s) differ:\n%s" % (len(bad), "\n".join(bad))


def check_rows(rows, out, ref, exp):
    """Per-row verdicts of a match array (row i's entry: target i when the matcher reports by
    target, query lead + i when by query), then the whole arrays: nothing else may be matched."""
    off = len(exp) - len(rows)
    bad = [f"{r}: GPU {out[off + i]}, oracle {ref[off + i]}, dictated {exp[off + i]}" for i, r in enumerate(rows)
           if not out[off + i] == ref[off + i] == exp[off + i]]
    report(bad)
    np.testing.assert_array_equal(out, ref)
    np.testing.assert_array_equal(out, exp)


@pytest.mark.parametrize("lead", LEADS)
def test_is_in_frustum_rows(lead):
    g, o = both()
    groups = GT.frustum_table()
    bad = []
    for (r, a), (_, b) in zip(GT.run_frustum(g, groups, lead), GT.run_frustum(o, groups, lead)):
        if not (GT.same_frustum(a, b) and GT.same_frustum(a, r.expect)):
            bad.append(f"{r}: GPU {a}, oracle {b}, dictated {r.expect}")
    report(bad)


@pytest.mark.parametrize("lead", LEADS)
def test_features_in_area_rows(lead):
    g, o = both()
    groups = GT.area_table()
    bad = []
    for (r, a), (_, b) in zip(GT.run_area(g, groups, lead), GT.run_area(o, groups)):
        if a != b or a != r.expect:
            bad.append(f"{r}: GPU {a}, oracle {b}, dictated {r.expect}")
    report(bad)


CALLS = GT.matcher_calls()


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("mode,S", [c[1:] for c in CALLS], ids=[c[0] for c in CALLS])
def test_matcher_rows(mode, S, lead):
    g, o = both()
    n, out, exp = GT.run_scene(g, mode, S, lead)
    nr, ref, _ = GT.run_scene(o, mode, S, lead)
    check_rows(S.rows, out, ref, exp)
    assert n == nr == sum(r.expect for r in S.rows)


@pytest.mark.parametrize("lead", LEADS)
def test_triangulation_rows(lead):
    g, o = both()
    for G in GT.triangulation_table():
        n, out, exp = GT.run_triangulation(g, G, lead)
        nr, ref, _ = GT.run_triangulation(o, G, lead)
        check_rows(G.rows, out, ref, exp)
        assert n == nr == sum(r.expect for r in G.rows)
