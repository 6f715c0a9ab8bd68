"""The CPU model of Optimizer::OptimizeEssentialGraph (tests/native/essential_graph_model.cpp, DESIGN.md
§22) proved by hand, and the Sim3 functions of csrc/orb_g2o_math.h pinned against it.  No GPU."""
from __future__ import annotations

import numpy as np
import pytest

import essential_graph_model as egm
import essential_graph_scenes as egs

EPS = 1e-5
# one v per branch of log(): |sigma| and the rotation (d = cos(theta) against 1 - eps: theta against
# 4.47e-3) sit a factor of ten or more on either side of the two eps tests; in the near branch log() takes
# omega = deltaR / 2, whose own error is theta^3 / 6, so theta is 7.5e-5 there.  Where |sigma| >= eps the
# small-angle B of both Sim3(update) and log() is ((sigma^2 / 2 - sigma + 1) s) / sigma^3 as sim3.h writes it
# (about 1 / sigma^3, not 1 / 6): the two are inverse to each other only where both take that branch, so
# case 1 keeps theta below exp's own eps as well.
BRANCH_CASES = {
    0: np.array([6e-5, -4e-5, 2e-5, 0.3, -0.2, 0.5, 1e-6]),    # |sigma| < eps, d > 1 - eps
    1: np.array([6e-6, -4e-6, 2e-6, 0.3, -0.2, 0.5, 0.05]),    # |sigma| >= eps, d > 1 - eps
    2: np.array([0.3, -0.2, 0.4, 0.3, -0.2, 0.5, -1e-6]),      # |sigma| < eps, d <= 1 - eps
    3: np.array([0.3, -0.2, 0.4, 0.3, -0.2, 0.5, -0.07]),      # |sigma| >= eps, d <= 1 - eps
}


@pytest.mark.parametrize("branch", sorted(BRANCH_CASES))
def test_log_of_exp_in_each_branch(branch):
    v = BRANCH_CASES[branch]
    out, br = egm.log(egm.exp(v))
    assert br == branch
    assert np.abs(out - v).max() <= 1e-12


def _rand_sim3(rng, rot=0.5, s=0.1):
    u = rng.normal(0, 1, 7) * np.array([rot, rot, rot, 1, 1, 1, s])
    return egm.exp(u)


def test_header_sim3_functions_match_the_model():
    """csrc/orb_g2o_math.h compiled for the host: the product, the inverse and the two conversions bit for
    bit, log() (its LU is written with selects, the model's with swaps) to 1e-13."""
    rng = np.random.default_rng(5)
    H = egm.host()
    for k in range(200):
        a, b = _rand_sim3(rng), _rand_sim3(rng, rot=1e-3 if k % 2 else 0.5, s=1e-7 if k % 3 == 0 else 0.1)
        o = np.zeros(8)
        H.s3h_mul(a.ctypes.data, b.ctypes.data, o.ctypes.data)
        assert o.tobytes() == egm.mul(a, b).tobytes()
        H.s3h_inverse(a.ctypes.data, o.ctypes.data)
        assert o.tobytes() == egm.inverse(a).tobytes()
        M = np.zeros(12)
        H.s3h_to_pose(b.ctypes.data, M.ctypes.data)
        assert M.tobytes() == egm.to_pose(b).tobytes()
        T = np.concatenate([egs._rodrigues(rng.normal(0, 1, 3)).reshape(9), rng.normal(0, 3, 3)]).astype(np.float32)
        H.s3h_from_pose(T.ctypes.data, o.ctypes.data)
        assert o.tobytes() == egm.from_pose(T).tobytes()
        r = np.zeros(7)
        br = H.s3h_log(b.ctypes.data, r.ctypes.data)
        ref, br_m = egm.log(b)
        assert br == br_m
        assert np.abs(r - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())


def test_lu3_solve_against_numpy():
    rng = np.random.default_rng(6)
    H = egm.host()
    for perm in ([0, 1, 2], [1, 0, 2], [2, 1, 0], [1, 2, 0], [2, 0, 1], [0, 2, 1]):
        W = (np.diag([5.0, 3.0, 2.0]) + rng.normal(0, 0.2, (3, 3)))[perm]  # the pivot of each column in every row
        t, x = rng.normal(size=3), np.zeros(3)
        W = np.ascontiguousarray(W)
        H.s3h_lu3_solve(W.ctypes.data, t.ctypes.data, x.ctypes.data)
        assert np.abs(x - np.linalg.solve(W, t)).max() <= 1e-13


def _err(C, vi, vj):
    return egm.log(egm.mul(egm.mul(C, vi), egm.inverse(vj)))[0]


def test_numeric_jacobian_against_central_difference():
    rng = np.random.default_rng(7)
    vi, vj = _rand_sim3(rng), _rand_sim3(rng)
    C = egm.mul(egm.mul(vj, egm.inverse(vi)), _rand_sim3(rng, 0.05, 0.02))
    err, Ji, Jj = egm.edge(C, vi, vj)
    assert err.tobytes() == _err(C, vi, vj).tobytes()
    h = 1e-6
    for d in range(7):
        u = np.zeros(7)
        u[d] = h
        ci = (_err(C, egm.mul(egm.exp(u), vi), vj) - _err(C, egm.mul(egm.exp(-u), vi), vj)) / (2 * h)
        cj = (_err(C, vi, egm.mul(egm.exp(u), vj)) - _err(C, vi, egm.mul(egm.exp(-u), vj))) / (2 * h)
        # the model differences at 1e-9, where the rounding of the errors is about 1e-16 / 1e-9
        assert np.abs(Ji[:, d] - ci).max() <= 1e-5
        assert np.abs(Jj[:, d] - cj).max() <= 1e-5


def _two_kf():
    return egs.constructed(2, [(1, 0, 1)], fixed=(0,), corrected=[1], seed=3, n_iterations=1)


def test_two_keyframes_one_damped_step():
    g, res = _two_kf()
    a = egm.graph_arrays(g)
    v0, v1 = egm.from_pose(a["kf_pose"][0]), a["kf_corrected"][1]
    C = egm.mul(v0, egm.inverse(a["kf_noncorrected"][1]))  # Sji = Sjw * Swi with i = 1, j = 0
    err, Ji, _ = egm.edge(C, v1, v0)
    H, b = Ji.T @ Ji, -Ji.T @ err
    x = np.linalg.solve(H + 1e-16 * np.eye(7), b)
    want = egm.mul(egm.exp(x), v1)
    assert res["info"]["trials"] == 1 and res["info"]["trial_accepted"] == [1]
    assert res["info"]["n_free"] == 1 and res["info"]["n_active"] == 2
    assert np.abs(res["kf_sim3"][1] - want).max() <= 1e-9 * np.abs(want).max()
    assert res["info"]["chi2_before"] == pytest.approx(float(err @ err), rel=1e-12)


def _ring5():
    return egs.ring(5, n_corrected=2, n_loop_to=1, fixed=0, seed=11, covis=(2,), pts_per_kf=4)


def test_five_keyframe_ring_converges():
    g, res = _ring5()
    I = res["info"]
    assert I["chi2_after"] < I["chi2_before"] and I["iterations"] >= 1
    assert res["kf_sim3"][0].tobytes() == egm.from_pose(g["kf_pose"][0]).tobytes()
    assert res["kf_pose_f64"][0].tobytes() == egm.to_pose(egm.from_pose(g["kf_pose"][0])).tobytes()
    assert res["kf_pose"].tobytes() == res["kf_pose_f64"].astype(np.float32).tobytes()
    br = res["margins"]["branch"]
    # the scene reaches both sides of both tests of log() (the fourth branch, a rotation without a scale,
    # is the unit-scale ring's)
    assert br[0] + br[2] > 0 and br[1] + br[3] > 0 and br[0] + br[1] > 0 and br[2] + br[3] > 0, br
    _, unit = egs.ring(5, n_corrected=2, n_loop_to=1, fixed=0, seed=11, covis=(2,), scale_per_lap=0.0)
    assert unit["margins"]["branch"][2] > 0, unit["margins"]["branch"]


def test_duplicate_pair_in_both_directions_adds_twice():
    g1, r1 = egs.constructed(2, [(1, 0, 1)], corrected=[1], seed=3, n_iterations=1)
    g2 = dict(g1)
    g2["edge_i"], g2["edge_j"], g2["edge_kind"] = np.int32([1, 1]), np.int32([0, 0]), np.uint8([1, 1])
    r2 = egm.run(g2, 1)
    assert r2["info"]["chi2_before"] == 2 * r1["info"]["chi2_before"]
    # twice H and twice b: the same step up to the damping of 1e-16
    assert np.abs(r2["kf_sim3"][1] - r1["kf_sim3"][1]).max() <= 1e-9
    g3, _ = egs.constructed(3, [(1, 0, 1), (2, 1, 1)], corrected=[1, 2], seed=4, n_iterations=3)
    g4 = dict(g3)
    g4["edge_i"], g4["edge_j"] = np.int32([1, 2, 1]), np.int32([0, 1, 2])
    g4["edge_kind"] = np.uint8([1, 1, 1])
    r3, r4 = egm.run(g3, 3), egm.run(g4, 3)
    assert r4["info"]["chi2_before"] > r3["info"]["chi2_before"]
    assert r4["info"]["n_edges"] == 3 and r4["info"]["profile_bytes"] == r3["info"]["profile_bytes"]


def test_isolated_vertex_and_unreferenced_point_come_back_bit_for_bit():
    g, _ = egs.constructed(4, [(1, 0, 1), (2, 1, 1)], corrected=[1, 2, 3], seed=5)
    g["pt_pos"] = np.float32([[1.25, -2.5, 3.0], [0.1, 0.2, 0.3], [4, 5, 6]])
    g["pt_ref"] = np.int32([-1, 3, 1])
    g["pt_skip"] = np.uint8([0, 0, 1])
    res = egm.run(g)
    assert res["info"]["n_active"] == 3 and res["info"]["n_free"] == 2
    assert res["kf_sim3"][3].tobytes() == np.ascontiguousarray(g["kf_corrected"][3]).tobytes()
    assert res["pt_pos"][0].tobytes() == g["pt_pos"][0].tobytes()
    assert res["pt_pos_f64"][0].tobytes() == g["pt_pos"][0].astype(np.float64).tobytes()
    assert res["pt_pos"][2].tobytes() == g["pt_pos"][2].tobytes()  # skipped: not written
    # vertex 3 did not move: its points go through S and back
    assert np.abs(res["pt_pos_f64"][1] - g["pt_pos"][1]).max() <= 1e-6


def test_refused_solve():
    """A keyframe whose corrected scale is 1e200 makes the Jacobian's entries overflow: the pivot is not
    finite, the trial's chi2 is DBL_MAX, the step is rejected and lambda grows."""
    g, _ = egs.constructed(3, [(1, 0, 1), (2, 1, 1)], corrected=[1, 2], seed=6)
    g["kf_corrected"] = g["kf_corrected"].copy()
    g["kf_corrected"][2, 4:7] = 1e160
    res = egm.run(g, 2)
    I = res["info"]
    assert I["refused"] >= 1 and I["trial_accepted"][0] == 0
    assert I["trial_chi2"][0] == np.finfo(np.float64).max
    assert res["kf_sim3"][1].tobytes() == np.ascontiguousarray(g["kf_corrected"][1]).tobytes()


def test_dense_and_profile_solves_agree_bit_for_bit():
    g, res = egs.ring(12, n_corrected=3, n_loop_to=2, fixed=1, seed=2)
    dense = egm.run(g, solver=egm.DENSE)
    assert res["info"]["profile_bytes"] < 11 * 11 * 49 * 8
    assert dense["kf_sim3"].tobytes() == res["kf_sim3"].tobytes()
    assert dense["info"]["trial_chi2"] == res["info"]["trial_chi2"]
    assert dense["info"]["lambda"] == res["info"]["lambda"]


def test_refusals():
    g, _ = _two_kf()
    for key, val in (("edge_j", np.int32([1])), ("edge_j", np.int32([2])), ("edge_i", np.int32([-1])),
                     ("edge_kind", np.uint8([2])), ("kf_fixed", np.uint8([0, 0]))):
        bad = dict(g)
        bad[key] = val
        assert egm.run(bad)["status"] == egm.EINVAL, key
    bad = dict(g)
    bad["kf_pose"] = g["kf_pose"].copy()
    bad["kf_pose"][1, 4] = np.nan
    assert egm.run(bad)["status"] == egm.EINVAL
    bad = dict(g)
    bad["kf_corrected"] = g["kf_corrected"].copy()
    bad["kf_corrected"][1, 7] = 0.0
    assert egm.run(bad)["status"] == egm.EINVAL


@pytest.mark.parametrize("variant", range(1, 8))
def test_every_mutant_moves_the_ring(variant):
    """The scenes can tell each mutant of DESIGN.md §22 from the model: what the GPU tests compare."""
    g, res = egs.ring(9, n_corrected=3, n_loop_to=2, fixed=0, seed=21, pts_per_kf=2)
    mut = egm.run(g, variant=variant)
    scale = g["scale"]
    moved = max(np.abs(mut["kf_pose_f64"] - res["kf_pose_f64"]).max(), np.abs(mut["kf_sim3"] - res["kf_sim3"]).max())
    assert moved > 1e-6 * scale, (variant, moved)


def test_sum_orders_agree_to_rounding():
    g, res = egs.ring(9, n_corrected=3, n_loop_to=2, fixed=0, seed=21)
    for order in (egm.PAIRWISE, egm.REVERSED):
        other = egm.run(g, sum_order=order)
        assert np.abs(other["kf_sim3"] - res["kf_sim3"]).max() <= 1e-6 * g["scale"]


def test_case_seeds():
    """Every listed case keeps the margins at the seed that essential_graph_scenes.CASE_SEEDS records."""
    assert set(egs.CASE_SEEDS) == set(egs.CASES)
    for name in egs.CASES:
        g, res, n_it, exact = egs.case(name)
        assert g["seed"] == egs.CASE_SEEDS[name], name
        assert egm.decisive_log(res) and (not exact or egm.decisive_trials(res)), name
        assert res["info"]["trials"] <= egm.MAX_TRIALS


def test_cases_cover_what_they_are_named_for():
    case = egs.case
    assert [case(n)[1]["info"]["n_free"] for n in ("free_1_edge_1", "free_2_chain", "chain_free_3", "chain_free_4",
                                                    "chain_free_5", "chain_free_11", "chain_free_12", "chain_free_13",
                                                    "ring_64", "ring_257")] == [1, 2, 3, 4, 5, 11, 12, 13, 64, 257]
    assert case("chain_free_13")[1]["info"]["profile_bytes"] == (1 + 12 * 2) * 49 * 8  # profile width 1
    g, res, _, _ = case("late_row_fixed_last")
    assert g["kf_fixed"][-1] == 1 and res["info"]["profile_bytes"] == (1 + 7 * 2 + 9) * 49 * 8  # row 8 reaches column 0
    g, res, _, _ = case("isolated_two_fixed")
    assert res["info"]["n_active"] == 7 and res["info"]["n_free"] == 5 and g["kf_fixed"].sum() == 2
    assert case("all_corrected")[0]["kf_has_corrected"].all() and not case("none_corrected")[0]["kf_has_corrected"].any()
    assert case("ring_20_fixed_2")[0]["kf_fixed"].tolist().index(1) == 2
    assert case("ring_20")[1]["margins"]["branch"][3] > 0 and case("ring_20_small_rotation")[1]["margins"]["branch"][3] == 0
    assert case("ring_20_unit_scale")[1]["margins"]["branch"][2] > 0
    assert case("ring_20_iterations_3")[1]["info"]["trial_accepted"] == [1, 1, 1]
    assert case("ring_20_iterations_1")[1]["info"]["trials"] == 1
