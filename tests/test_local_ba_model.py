"""The CPU model of Optimizer::LocalBundleAdjustment (tests/native/local_ba_model.cpp)
on cases small enough to work by hand: both Jacobians against central differences, one damped step
through the Schur complement against numpy's solve of the full system, the vertices that drop out,
the erase walk on a hand-made table, a refused solve and an edge with z = 0."""
import numpy as np
import pytest

import local_ba_model as lbm
import local_ba_scenes as sc

K4 = np.array(sc.K_DEFAULT, np.float64)
DELTA = float(np.float32(np.sqrt(5.991)))


def _pose(seed):
    rng = np.random.default_rng(seed)
    R = sc.rot(rng.normal(0, 0.4, 3))
    return lbm.pose7(np.concatenate([R.reshape(9), rng.normal(0, 0.5, 3)]))


def test_jacobians_match_central_differences():
    rng = np.random.default_rng(5)
    for k in range(20):
        T = _pose(k)
        M = lbm.pose_matrix(T)
        Xc = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(3, 9)])
        X = M[:9].reshape(3, 3).T @ (Xc - M[9:])
        obs = rng.uniform(0, 240, 2)
        e0, chi2, A, B = lbm.edge(T, K4, X, obs, 0.7)
        assert chi2 == pytest.approx(0.7 * e0 @ e0, rel=1e-14)
        h = 1e-6
        for d in range(3):  # X + delta
            dx = np.zeros(3)
            dx[d] = h
            num = (lbm.edge(T, K4, X + dx, obs, 1.0)[0] - lbm.edge(T, K4, X - dx, obs, 1.0)[0]) / (2 * h)
            np.testing.assert_allclose(A[:, d], num, rtol=1e-6, atol=1e-6)
        for d in range(6):  # exp(delta) * T
            dx = np.zeros(6)
            dx[d] = h
            num = (lbm.edge(lbm.exp_update(dx, T), K4, X, obs, 1.0)[0] -
                   lbm.edge(lbm.exp_update(-dx, T), K4, X, obs, 1.0)[0]) / (2 * h)
            np.testing.assert_allclose(B[:, d], num, rtol=1e-6, atol=1e-6)


def _small(seed=7, **kw):
    """2 free keyframes + 1 fixed, 6 points, every point seen by all three."""
    args = dict(n_free=2, n_fixed=1, n_pt=6, obs_per_pt=3, outliers=0.0)
    args.update(kw)
    return sc.build_scene(seed, args.pop("n_free"), args.pop("n_fixed"), args.pop("n_pt"), args.pop("obs_per_pt"), **args)


def _full_system(g, st):
    """[[Hpp, Hpl], [Hpl', Hll]] and b over the free keyframes, then the points."""
    free = [i for i in range(len(g["kf_fixed"])) if not g["kf_fixed"][i]]
    npt = len(g["pt_pos"])
    n = 6 * len(free) + 3 * npt
    H, b = np.zeros((n, n)), np.zeros(n)
    for a, i in enumerate(free):
        H[6 * a:6 * a + 6, 6 * a:6 * a + 6] = st["Hpp"][i]
        b[6 * a:6 * a + 6] = st["bp"][i]
    o = 6 * len(free)
    for p in range(npt):
        H[o + 3 * p:o + 3 * p + 3, o + 3 * p:o + 3 * p + 3] = st["Hll"][p]
        b[o + 3 * p:o + 3 * p + 3] = st["bl"][p]
    for e, (p, i) in enumerate(zip(g["edge_pt"], g["edge_kf"])):
        if g["kf_fixed"][i]:
            continue
        a = free.index(i)
        H[6 * a:6 * a + 6, o + 3 * p:o + 3 * p + 3] = st["Hpl"][e]
        H[o + 3 * p:o + 3 * p + 3, 6 * a:6 * a + 6] = st["Hpl"][e].T
    return H, b, free


def test_quadratic_form_matches_the_edges():
    g = _small()
    st = lbm.step(g, 1.0)
    assert st["status"] == 0
    Hpp, Hll = np.zeros_like(st["Hpp"]), np.zeros_like(st["Hll"])
    bp, bl = np.zeros_like(st["bp"]), np.zeros_like(st["bl"])
    for e, (p, i) in enumerate(zip(g["edge_pt"], g["edge_kf"])):
        T = lbm.pose7(g["kf_pose"][i])
        s = float(g["edge_inv_sigma2"][e])
        err, chi2, A, B = lbm.edge(T, g["kf_K"][i].astype(np.float64), g["pt_pos"][p].astype(np.float64),
                                   g["edge_obs"][e].astype(np.float64), s)
        w = 1.0 if chi2 <= DELTA * DELTA else DELTA / np.sqrt(chi2)  # rho[1] of the Huber kernel
        Hll[p] += A.T @ A * s * w
        bl[p] += -A.T @ err * s * w
        if not g["kf_fixed"][i]:
            Hpp[i] += B.T @ B * s * w
            bp[i] += -B.T @ err * s * w
            np.testing.assert_allclose(st["Hpl"][e], B.T @ A * s * w, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(st["Hpp"], Hpp, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(st["Hll"], Hll, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(st["bp"], bp, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(st["bl"], bl, rtol=1e-12, atol=1e-9)
    assert not st["Hpp"][2].any() and not st["bp"][2].any()  # the fixed keyframe gets no block and no b


@pytest.mark.parametrize("order", [0, 1, 2])
def test_damped_step_through_schur_equals_the_full_30x30_solve(order):
    g = _small()
    assert len(g["edge_pt"]) == 18
    lam = 3.5
    st = lbm.step(g, lam, order)
    assert st["status"] == 0
    H, b, free = _full_system(g, st)
    assert H.shape == (30, 30)
    x = np.linalg.solve(H + lam * np.eye(30), b)
    got = np.concatenate([st["xp"][free].reshape(-1), st["xl"].reshape(-1)])
    assert np.max(np.abs(got - x)) <= 1e-9 * np.max(np.abs(x))
    assert not st["xp"][2].any()  # the fixed keyframe has no unknowns


def test_point_seen_only_by_fixed_keyframes():
    g = sc.build_scene(11, 2, 3, 12, 3, outliers=0.0)
    # point 0: its three edges go to the three fixed keyframes (2, 3, 4)
    own = np.flatnonzero(g["edge_pt"] == 0)
    g["edge_kf"][own] = [2, 3, 4]
    for e in own:
        R, t = g["kf_pose"][g["edge_kf"][e]][:9].reshape(3, 3).astype(np.float64), g["kf_pose"][g["edge_kf"][e]][9:]
        g["edge_obs"][e] = sc.project(R, t.astype(np.float64), K4, g["pt_pos"][0:1].astype(np.float64) + 0.01)[0][0]
    lam = 0.25
    st = lbm.step(g, lam)
    assert st["status"] == 0 and not st["Hpl"][own].any()
    want = np.linalg.solve(st["Hll"][0] + lam * np.eye(3), st["bl"][0])  # no Hpl block: x_l = Dinv b_l
    np.testing.assert_allclose(st["xl"][0], want, rtol=1e-9)
    res = lbm.local_bundle_adjustment(g)
    assert res["status"] == 0 and np.isfinite(res["pt_pos_f64"]).all()
    assert np.abs(res["pt_pos_f64"][0] - g["pt_pos"][0]).max() > 1e-6  # it is optimised all the same


def test_free_keyframe_that_loses_every_edge_keeps_its_pose_in_round_2():
    g = sc.build_scene(13, 3, 2, 40, 3, outliers=0.0)
    kf = 1
    own = np.flatnonzero(g["edge_kf"] == kf)
    assert len(own) >= 10
    # every observation of this keyframe is a gross outlier, each in its own direction: no pose fits them
    rng = np.random.default_rng(13)
    g["edge_obs"][own] += (rng.choice([-1, 1], (len(own), 2)) * rng.uniform(80, 200, (len(own), 2))).astype(np.float32)
    g["pt_nobs"][:] = 5  # no point goes bad: only the keyframe drops out
    res = lbm.local_bundle_adjustment(g)
    assert res["status"] == 0
    assert (res["edge_erased"][own] == 1).all()
    r1, r2 = res["info"]["round"]
    assert r1["active_keyframes"] == 3 and r2["active_keyframes"] == 2
    assert res["kf_pose_f64"][kf].tobytes() == res["kf_pose_round1_f64"][kf].tobytes()
    for other in (0, 2):  # the others went on
        assert res["kf_pose_f64"][other].tobytes() != res["kf_pose_round1_f64"][other].tobytes()
    for fx in (3, 4):  # fixed: the input after the quaternion round trip
        np.testing.assert_array_equal(res["kf_pose_f64"][fx], lbm.pose_matrix(lbm.pose7(g["kf_pose"][fx])))


def test_erase_walk_on_a_hand_made_table():
    # point 0: three edges, chi2 8 / 9 / 1; point 1: two edges that pass; point 2: a depth of -1 and a
    # chi2 of 7; point 3: three edges, one failing
    ept = [0, 0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 3]
    chi2 = [8.0, 9.0, 1.0, 1.0, 5.991, 1.0, 1.0, 7.0, 1.0, 1.0, 9.0, 1.0]
    depth = [4.0, 4.0, 4.0, 4.0, 4.0, 4.0, -1.0, 4.0, 4.0, 4.0, 4.0, 4.0]
    zero_e, zero_p = np.zeros(12, np.uint8), np.zeros(4, np.uint8)
    # nobs 3: the first failing edge takes the count to 2, the point goes bad, its later failing edge is
    # skipped and keeps erased = 0
    er, bad, nobs = lbm.erase_walk(ept, [3, 2, 5, 3], chi2, depth, zero_e, zero_p, 1)
    assert er.tolist() == [1, 0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0]  # chi2 == 5.991 is not > 5.991
    assert bad.tolist() == [1, 0, 0, 1] and nobs.tolist() == [2, 2, 3, 2]
    # nobs 4 (one observation in a bad keyframe that has no edge): losing one edge leaves 3, point 3 stays;
    # point 0 loses both failing edges and goes bad at the second
    er4, bad4, nobs4 = lbm.erase_walk(ept, [4, 2, 5, 4], chi2, depth, zero_e, zero_p, 1)
    assert er4.tolist() == [1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0]
    assert bad4.tolist() == [1, 0, 0, 0] and nobs4.tolist() == [2, 2, 3, 3]
    # round 2 on the first table: a bad point's edges are skipped whatever their chi2, erased edges too
    chi2b = [0.0, 100.0, 100.0, 9.0, 1.0, 6.0, 100.0, 100.0, 1.0, 100.0, 100.0, 100.0]
    er2, bad2, nobs2 = lbm.erase_walk(ept, nobs, chi2b, [4.0] * 12, er, bad, 2)
    assert er2.tolist() == [1, 0, 0, 2, 0, 2, 1, 1, 0, 0, 1, 0]
    assert bad2.tolist() == [1, 2, 2, 1] and nobs2.tolist() == [2, 1, 2, 2]


def test_edges_of_a_point_gone_bad_in_round_1_stay_active_in_round_2():
    g = sc.host_case("outliers_points_go_bad")
    m = g["model"]
    bad1 = np.flatnonzero(m["pt_bad"] == 1)
    left = [e for e in range(len(g["edge_pt"])) if g["edge_pt"][e] in set(bad1) and m["edge_erased"][e] == 0]
    assert len(bad1) >= 4 and len(left) >= 4
    assert np.isfinite(m["chi2"][1][left]).all()  # they were in round 2's optimisation
    assert m["info"]["round"][1]["active_edges"] == int((m["edge_erased"] != 1).sum())
    assert any(m["chi2"][1][e] > lbm.CHI2_TH for e in left)  # and none of them was classified
    mutant = lbm.local_bundle_adjustment(g, variant=2)
    assert mutant["info"]["round"][1]["active_edges"] < m["info"]["round"][1]["active_edges"]


def test_chi2_exactly_at_the_threshold_is_kept():
    g = sc.threshold_case()
    m = lbm.local_bundle_adjustment(g)
    assert m["status"] == 0
    assert np.array_equal(m["chi2"], np.full((2, 4), 5.991)), "the case is built on exact equality"
    assert not m["edge_erased"].any() and not m["pt_bad"].any()
    assert [(r["iterations"], r["trials"]) for r in m["info"]["round"]] == [(1, 1), (1, 1)]
    assert np.array_equal(m["kf_pose"], g["kf_pose"]) and np.array_equal(m["pt_pos"], g["pt_pos"])
    assert lbm.local_bundle_adjustment(g, variant=5)["edge_erased"].tolist() == [1, 0, 1, 0]  # >= for >
    up = lbm.local_bundle_adjustment(sc.threshold_case(above=True))
    # one float above: each point loses its first edge, goes bad at a count of 1, and keeps its second
    assert up["edge_erased"].tolist() == [1, 0, 1, 0] and up["pt_bad"].tolist() == [1, 1]
    assert (up["chi2"][0] > 5.991).all() and up["info"]["round"][1]["active_keyframes"] == 0


def test_refused_solve():
    rng = np.random.default_rng(3)
    M = rng.normal(0, 1, (12, 12))
    S = M @ M.T + 12 * np.eye(12)
    b = rng.normal(0, 1, 12)
    ok, x = lbm.cholesky_solve(S, b)
    assert ok
    np.testing.assert_allclose(x, np.linalg.solve(S, b), rtol=1e-10)
    S[5, 5] = -1.0
    ok, x = lbm.cholesky_solve(S, b)
    assert not ok and not x.any()
    S[5, 5] = np.nan
    assert not lbm.cholesky_solve(S, b)[0]
    assert not lbm.cholesky_solve(np.zeros((3, 3)), np.ones(3))[0]  # a zero pivot is not positive


def test_one_edge_with_z_zero():
    g = sc.build_scene(17, 2, 2, 20, 3, outliers=0.0)
    # keyframe 3 (fixed): the identity pose; point 0 lies in its image plane, so z = 0 exactly
    g["kf_pose"][3] = np.concatenate([np.eye(3).reshape(9), np.zeros(3)]).astype(np.float32)
    keep = g["edge_kf"] != 3
    keep[np.flatnonzero(g["edge_pt"] == 0)[0]] = True
    for k in ("edge_pt", "edge_kf", "edge_obs", "edge_inv_sigma2"):
        g[k] = g[k][keep]
    e0 = int(np.flatnonzero(g["edge_pt"] == 0)[0])
    g["edge_kf"][e0] = 3
    g["edge_kf"][e0 + 1:e0 + 3] = [0, 1]
    g["pt_pos"][0] = [0.5, -0.25, 0.0]
    g["pt_nobs"][:] = 6
    res = lbm.local_bundle_adjustment(g)
    assert res["status"] == 0
    r1, r2 = res["info"]["round"]
    # every trial of round 1 meets a system that is not finite: refused, rejected, the state kept
    assert r1["refused"] == r1["trials"] == r1["iterations"] >= 1 and not np.isfinite(r1["chi2_before"])
    assert res["depth"][0][e0] == 0.0 and res["edge_erased"][e0] == 1  # !(0 > 0): isDepthPositive fails
    assert r2["refused"] == 0 and np.isfinite(r2["chi2_after"]) and r2["chi2_after"] < r2["chi2_before"]
    assert np.isfinite(res["kf_pose_f64"]).all() and np.isfinite(res["pt_pos_f64"]).all()


def test_refusals_and_empty_problems():
    g = _small()
    a = {k: g[k].copy() for k in sc.GRAPH_KEYS}
    assert lbm.local_bundle_adjustment(a)["status"] == 0
    bad = dict(a, kf_fixed=np.ones(3, np.uint8))
    assert lbm.local_bundle_adjustment(bad)["status"] == -95  # no free keyframe
    bad = dict(a, edge_pt=a["edge_pt"][::-1].copy())
    assert lbm.local_bundle_adjustment(bad)["status"] == -22  # points descend
    bad = dict(a, edge_kf=np.where(np.arange(18) == 1, a["edge_kf"][0], a["edge_kf"]).astype(np.int32))
    assert lbm.local_bundle_adjustment(bad)["status"] == -22  # a pair twice
    bad = dict(a, edge_kf=np.where(np.arange(18) == 4, 3, a["edge_kf"]).astype(np.int32))
    assert lbm.local_bundle_adjustment(bad)["status"] == -22  # keyframe index out of range
    bad = dict(a, pt_nobs=np.full(6, 2, np.int32))
    assert lbm.local_bundle_adjustment(bad)["status"] == -22  # more edges than observations
    empty = dict(a, edge_pt=a["edge_pt"][:0], edge_kf=a["edge_kf"][:0], edge_obs=a["edge_obs"][:0],
                 edge_inv_sigma2=a["edge_inv_sigma2"][:0])
    res = lbm.local_bundle_adjustment(empty)
    assert res["status"] == 0 and res["info"]["round"][0]["iterations"] == 0
    np.testing.assert_array_equal(res["pt_pos"], a["pt_pos"])
    for i in range(3):
        np.testing.assert_array_equal(res["kf_pose_f64"][i], lbm.pose_matrix(lbm.pose7(a["kf_pose"][i])))


def test_every_listed_case_finds_a_decisive_seed():
    for name in list(sc.HOST_CASES) + [sc.GAUGE_FREE_CASE[0]]:
        g = sc.host_case(name)
        assert g["skipped"] <= sc.MAX_SEED_SKIPS and lbm.decisive(g["model"], g["scale"]), name
    assert lbm.decisive(sc.fixture_scene()["model"], sc.RADIUS)
