"""The adversarial matcher scenes (tests/adversarial_scenes.py) against the CPU oracle and, where
tests/test_matcher_family_oracle.py has one, the Python reading of the matcher: every builder's
analytic expectation (the chain mappings, the float32 evaluation of each acceptance rule, the
plain loop over a vocabulary node) must be what the reference's sequential loops compute.  This
pins the scenes themselves: were one of them to stop being a chain, the GPU tests built on them
(tests/test_gpu_matcher_adversarial.py) would lose their point silently."""
import numpy as np
import pytest

import adversarial_scenes as A
from oracle_lib import OracleMatcher, search_for_initialization
from test_matcher_family_oracle import py_fuse, py_sbp_local, py_triangulation, py_window_search

W, H = A.W, A.H
RATIOS = (0.6, 0.75, 0.8, 0.9)


def rng_of(*key):
    return np.random.default_rng([7, *[int(k) if k is not None else 99991 for k in key]])


def test_exact_distances():
    rng = rng_of(0)
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    for k in (0, 1, 49, 50, 51, 100, 256):
        assert A.hamming_matrix(d[None], A.at_distance(rng, d, k)[None])[0, 0] == k
    assert A.hamming_matrix(d[None], A.flip_bits(d, [0, 9, 255])[None])[0, 0] == 3
    for kind in "AB":
        A.chain_descriptors(rng, 2100, kind)  # asserts own / prev / far itself


@pytest.mark.parametrize("n,layout", [(2100, "short"), (200, "long")])
def test_list_lengths(n, layout):
    """GetFeaturesInArea of the oracle around every query: at most 8 targets in the short
    layout (no GPU candidate list is truncated), the whole chain in the long one."""
    C = A.chain_scene(rng_of(1, n), n, "A", layout)
    o = OracleMatcher()
    lens = np.array([len(o.GetFeaturesInArea(C.T, C.Q.kps["x"][q], C.Q.kps["y"][q], C.window, 0, 0))
                     for q in range(C.Q.n)])
    qx, qy = C.Q.kps["x"], C.Q.kps["y"]
    np.testing.assert_array_equal(lens, A.box_counts(qx, qy, C.T.kps["x"], C.T.kps["y"], C.window))
    assert (lens.max() <= 8 and lens.min() >= 1) if layout == "short" else (lens == n).all()


VARIANTS = [(0, None), (3, None), (7, None), (0, 0), (3, 0), (0, 137), (7, 137)]


def _expect(C, mode, ori):
    return C.by_target_ori if ori and mode in A.ORI_MODES else C.by_target


@pytest.mark.parametrize("lead,broken", VARIANTS)
@pytest.mark.parametrize("mode,kind", [("window", "A"), ("window", "B"), ("local", "A"), ("f2f", "A"), ("motion", "B"),
                                       ("reloc", "B"), ("sim3", "B")])
def test_grid_chain(mode, kind, lead, broken):
    for n, layout in ((300, "short"), (200, "long")):
        C = A.chain_scene(rng_of(2, n, lead, broken), n, kind, layout, lead, broken)
        full = n if broken is None else (broken if kind == "A" else n - 1)
        assert C.count == full
        for ori in (False, True):
            cnt, out = A.run_grid(OracleMatcher(0.9, ori), mode, C)
            e = _expect(C, mode, ori)
            np.testing.assert_array_equal(out, e)
            assert cnt == (e >= 0).sum()
            if ori and mode in A.ORI_MODES and full >= 100:
                assert 0 < cnt < full  # the 10 % bin is dropped, the three maxima stay


def test_orientation_bins():
    """40/30/20/10 % of an unbroken chain's pairs fall into rotation bins 1..4:
    ComputeThreeMaxima keeps 1, 2, 3 (max3 = 20 % is not below 0.1 * max1) and drops the fourth."""
    C = A.chain_scene(rng_of(3), 1100, "A")
    assert C.count == 1100 and C.count_ori == 990
    dropped = np.flatnonzero((C.by_target >= 0) & (C.by_target_ori < 0))
    assert (dropped % 10 == 9).all() and len(dropped) == 110


def test_grid_chain_long_strides():
    """The GPU tests' sizes: more than one and more than two 1024-thread strides."""
    for n in (1100, 2100):
        for mode, kind in (("window", "A"), ("motion", "B")):
            for broken in (None, 1029):
                C = A.chain_scene(rng_of(4, n, broken), n, kind, "short", 3, broken)
                cnt, out = A.run_grid(OracleMatcher(0.9, False), mode, C)
                np.testing.assert_array_equal(out, C.by_target)


@pytest.mark.parametrize("mode", ["local", "f2f"])
def test_taken_head(mode):
    """T[0] taken before the call: query 0 has no candidate left and query 1 finds T[0] taken,
    exactly as if query 0 had matched it, so links 1 .. n-1 match.  (Removing the head *query*
    is what empties the result: broken = 0 above.)"""
    C = A.chain_scene(rng_of(5), 300, "A", take_first=True)
    cnt, out = A.run_grid(OracleMatcher(0.9, False), mode, C, C.taken0)
    assert cnt == 299 and out[0] == -1
    np.testing.assert_array_equal(out, C.by_target)


def test_single_queries():
    """Each query alone: kind A is rejected by the ratio test, kind B takes its predecessor's
    target: the chained result comes from the cross-query state, not from the descriptors."""
    for kind in "AB":
        C = A.chain_scene(rng_of(6), 300, kind)
        o = OracleMatcher(0.9, False)
        for q in range(1, 300, 8):
            u = np.zeros(300, np.uint8)
            u[q] = 1
            cnt, out = o.WindowSearch(C.Q, u, C.T, C.window)
            if kind == "A":
                assert cnt == 0
            else:
                assert cnt == 1 and out[q - 1] == q


def test_python_readings_on_chains():
    for broken in (None, 41):
        C = A.chain_scene(rng_of(7, broken), 150, "A", "short", 3, broken)
        for ori in (False, True):
            cnt, out = py_window_search(C.Q, C.usable, C.T, C.window, 0, 2**31 - 1, 0.9, ori)
            np.testing.assert_array_equal(out, _expect(C, "window", ori))
        z, one = np.zeros(C.Q.n, np.int32), np.ones(C.Q.n, np.float32)
        cnt, out = py_sbp_local(C.T, np.zeros(C.T.n, np.uint8), C.usable, C.Q.kps["x"], C.Q.kps["y"], z, one,
                                C.Q.desc, C.window / 2.5, 0.9)
        np.testing.assert_array_equal(out, C.by_target)
        assert cnt == C.count


def sfi(C, nnratio=0.9, ori=False, window=None):
    k1, k2 = C.Q.kps, C.T.kps
    prev = np.ascontiguousarray(np.stack([k1["x"], k1["y"]], 1).astype(np.float32))
    return search_for_initialization(k1, C.Q.desc, k2, C.T.desc, W, H, prev, nnratio, ori, window or C.window)


@pytest.mark.parametrize("n,layout,window", [(200, "long", 100), (1000, "short", None), (1500, "short", None)])
def test_sfi_chain(n, layout, window):
    for lead, broken in ((0, None), (3, None), (0, 0), (7, 137)):
        C = A.chain_scene(rng_of(8, n, lead, broken), n, "A", layout, lead, broken, disabled_octave=1)
        for ori in (False, True):
            cnt, m12 = sfi(C, 0.9, ori, window)
            np.testing.assert_array_equal(m12, C.by_query(ori))
            assert cnt == (n if broken is None else broken) - (0 if not ori else C.count - C.count_ori)


@pytest.mark.parametrize("n", [16, 64, 400])
@pytest.mark.parametrize("nnratio", [0.9, 0.75])
def test_bow_chain(n, nnratio):
    for lead, broken in ((0, None), (3, None), (0, 0), (7, n // 2 + 3)):
        C = A.chain_scene(rng_of(9, n, lead, broken), n, "A", "short", lead, broken)
        for dup in (False, True):
            fv1, fv2 = A.chain_bow(C, duplicate=dup)
            for ori in (False, True):
                o = OracleMatcher(nnratio, ori)
                cnt, out = o.SearchByBoW_KF_F(C.Q, C.usable, fv1, C.T, fv2)
                np.testing.assert_array_equal(out, C.by_target_ori if ori else C.by_target)
                cnt2, out2 = o.SearchByBoW_KF_KF(C.Q, C.usable, fv1, C.T, None, fv2)
                np.testing.assert_array_equal(out2, C.by_query(ori))
                assert cnt == cnt2 == (C.count_ori if ori else C.count)
        assert C.count == (n if broken is None else broken)


@pytest.mark.parametrize("lead,broken", [(0, None), (3, None), (7, None), (0, 0), (3, 77)])
def test_triangulation_chain(lead, broken):
    V1, h1, fv1, V2, fv2, F12, exp, exp_o = A.triangulation_scene(rng_of(10, lead, broken), 200, lead, broken)
    h2 = np.zeros(V2.n, np.uint8)
    assert (exp >= 0).sum() == (200 if broken is None else 199)
    if broken is not None:
        assert (exp[lead + broken + 1:] == np.arange(broken, 199)).all()  # shifted by one after the break
    for ori, e in ((False, exp), (True, exp_o)):
        cnt, out = OracleMatcher(0.6, ori).SearchForTriangulation(V1, h1, fv1, V2, h2, fv2, F12)
        np.testing.assert_array_equal(out, e)
        assert cnt == (e >= 0).sum()
    cnt, out = py_triangulation(V1, h1, fv1, V2, h2, fv2, F12, True)
    np.testing.assert_array_equal(out, exp_o)


# accepted rows of the two-candidate table per nnratio: (KF-KF, KF-F); they differ in the d1 == 50 rows
TABLE_COUNTS = {0.6: (151, 151), 0.75: (115, 118), 0.8: (111, 113), 0.9: (104, 106)}


@pytest.mark.parametrize("nnratio", RATIOS)
def test_ratio_table(nnratio):
    Tb = A.ratio_table(rng_of(11, int(100 * nnratio)), nnratio)
    pairs = [r for r in Tb.rows if r[1] is not None]
    assert 226 <= len(pairs) <= 238
    assert 8 <= Tb.exact_ties(nnratio) <= 20  # rows that tell `<` from `<=`
    for k, name in enumerate(("bow_kf_kf", "bow_kf_f")):
        acc = sum(A.rule(name, nnratio)(d1, d2) for d1, d2 in pairs)
        assert acc == TABLE_COUNTS[nnratio][k]
    o = OracleMatcher(nnratio, False)
    cnt, by_t, by_q = Tb.expect("bow_kf_f", nnratio)
    n, out = o.SearchByBoW_KF_F(Tb.Q, None, Tb.fvq, Tb.T, Tb.fvt)
    assert n == cnt
    np.testing.assert_array_equal(out, by_t)
    cnt, by_t, by_q = Tb.expect("bow_kf_kf", nnratio)
    n, out = o.SearchByBoW_KF_KF(Tb.Q, None, Tb.fvq, Tb.T, None, Tb.fvt)
    assert n == cnt
    np.testing.assert_array_equal(out, by_q)
    for mode in A.GRID_MODES:
        C = A.table_chain(Tb)
        cnt, by_t, _ = Tb.expect(mode, nnratio, 64 if mode == "reloc" else 100)
        n, out = A.run_grid(o, mode, C, orbdist=64)
        assert n == cnt and cnt > 0, (mode, n, cnt)
        np.testing.assert_array_equal(out, by_t)
    cnt, _, by_q = Tb.expect("sfi", nnratio)
    n, m12 = sfi(A.table_chain(Tb), nnratio, False)
    assert n == cnt
    np.testing.assert_array_equal(m12, by_q)
    for name in ("fuse", "triang", "sim3_pair"):
        cnt, _, by_q = Tb.expect(name, nnratio)
        n, out = A.run_table_by_query(o, name, Tb)
        assert n == cnt > 50
        np.testing.assert_array_equal(out, by_q)
    # the Python readings of the matchers
    ones, z = np.ones(Tb.Q.n, np.uint8), np.zeros(Tb.Q.n, np.int32)
    cnt, out = py_window_search(Tb.Q, ones, Tb.T, Tb.window, 0, 2**31 - 1, nnratio, False)
    np.testing.assert_array_equal(out, Tb.expect("window", nnratio)[1])
    cnt, out = py_sbp_local(Tb.T, np.zeros(Tb.T.n, np.uint8), ones, Tb.Q.kps["x"], Tb.Q.kps["y"], z,
                            np.ones(Tb.Q.n, np.float32), Tb.Q.desc, Tb.window / 2.5, nnratio)
    np.testing.assert_array_equal(out, Tb.expect("local", nnratio)[1])
    cnt, out = py_fuse(Tb.T, A.chain_map_points(C, kind="sim3"), ones, Tb.window / 1.2, False)
    np.testing.assert_array_equal(out, Tb.expect("fuse", nnratio)[2])
    cnt, out = py_triangulation(Tb.Q, np.zeros(Tb.Q.n, np.uint8), Tb.fvq, Tb.T, np.zeros(Tb.T.n, np.uint8), Tb.fvt,
                                A.F12_ROWS, False)
    np.testing.assert_array_equal(out, Tb.expect("triang", nnratio)[2])


SWEEPS = {"unstaged": ((1, 2, 15, 16, 17, 63, 64, 65, 130), (1, 3, 4, 5, 63, 64, 65, 67, 130)),
          "staged": ((1, 15, 16, 17, 64, 65), (1, 4, 5, 64, 65, 67))}


@pytest.mark.parametrize("which", list(SWEEPS))
@pytest.mark.parametrize("nnratio", [0.75, 0.9, 1.25])
def test_node_sweep(which, nnratio):
    """The oracle against the plain loop over each node; every node big enough shows all three
    dependency outcomes (an acceptance takes a later query's best, its second, neither).
    nnratio 1.25 accepts equal best and second distances, so the duplicated candidates of the
    tie nodes show that the first minimum in candidate order wins."""
    Sw = A.node_sweep(rng_of(12, len(SWEEPS[which][0])), *SWEEPS[which])
    assert (Sw.Q.n <= 1800 and Sw.T.n <= 1800) == (which == "staged")
    assert len(Sw.tie_nodes) >= 1
    for usable in (True, False):
        uq, ut = (Sw.uq, Sw.ut) if usable else (None, None)
        for kf_kf in (False, True):
            stats = {}
            cnt, by_t, by_q = A.bow_loop(kf_kf, nnratio, Sw.Q, uq, Sw.fvq, Sw.T, ut, Sw.fvt, stats)
            o = OracleMatcher(nnratio, False)
            if kf_kf:
                n, out = o.SearchByBoW_KF_KF(Sw.Q, uq, Sw.fvq, Sw.T, ut, Sw.fvt)
                np.testing.assert_array_equal(out, by_q)
            else:
                n, out = o.SearchByBoW_KF_F(Sw.Q, uq, Sw.fvq, Sw.T, Sw.fvt)
                np.testing.assert_array_equal(out, by_t)
            assert n == cnt and cnt > Sw.Q.n // 10
            if nnratio == 0.75:
                for node, (nc, nq) in Sw.shapes.items():
                    if nc >= 15 and nq >= 63:
                        assert stats[node] == {"best", "second", "neither"}, (node, nc, nq, stats[node])
    if nnratio == 1.25:  # a tie node's duplicate pair: only the earlier candidate may be matched first
        cnt, by_t, _ = A.bow_loop(False, nnratio, Sw.Q, None, Sw.fvq, Sw.T, None, Sw.fvt)
        tn = {int(x): k for k, x in enumerate(Sw.fvt.nodes)}
        hit = 0
        for node in Sw.tie_nodes:
            c = Sw.fvt.features[Sw.fvt.offsets[tn[node]]:Sw.fvt.offsets[tn[node] + 1]]
            assert not (by_t[c[-1]] >= 0 and by_t[c[-2]] < 0)
            hit += by_t[c[-2]] >= 0
        assert hit >= 1


def test_big_bow_pair_is_fast_and_matches():
    import time

    t0 = time.perf_counter()
    V1, fv1, V2, fv2 = A.big_bow_pair(rng_of(13), 11800, 11800)
    assert time.perf_counter() - t0 < 1.0
    n, out = OracleMatcher(0.75, True).SearchByBoW_KF_F(V1, None, fv1, V2, fv2)
    assert n > 1000
