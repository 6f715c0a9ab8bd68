"""csrc/orb_epnp_math.h held stage by stage to tests/epnp_reference.py, a numpy float64 EPnP that shares
no statement with it.  The header is compiled for the host by
tests/native/pnp_solver_model.cpp, whose pnp_solver_model_stages exports what every step of
compute_pose left behind; the GPU tests hold the kernels to that build bit for bit.

Every stage is fed the header's own upstream value and compared with the reference's result for that
one step; `chain` then runs from the exported null-space basis and alphas to the three poses with
nothing else of the header's.  Inputs (epnp_stage_checks.general_cases): 600 four-point pm.scene sets
without noise, 200 with 1 px, 60 five-point sets, 80 sets of 6 to 45 points with 1 px; and the
degenerate sets of test_gpu_pnp_solver.py.

Bounds: 10 x the largest difference that scripts/measure_epnp_stage_bounds.py prints over those 940
inputs (the margin test_pnp_solver_model.py uses; it allows for another libm or LAPACK build).  Where
that is under 1e-15 (the centroid agreed to the bit) the bound is 1e-15, a few units in the last place
of values of order 1.  Measured -> bound:

    control points   centroid 0 -> 1e-15, radius 5.808e-13 -> 5.808e-12, direction 4.707e-14 -> 4.707e-13
    alphas           rows sum to 1: 1.332e-15 -> 1.332e-14, alphas @ cws - pw: 3.997e-15 -> 3.997e-14,
                     ci - inv(CC): 5.116e-13 -> 5.116e-12
    mtm_svd          ut ut^T - I: 2.248e-15 -> 2.248e-14; relative to w[0]: ut^T diag(w) ut - M^T M
                     1.777e-15 -> 1.777e-14, w - sv(M)^2 2.659e-15 -> 2.659e-14
    l_6x10           by its definition (relative) 6.141e-15 -> 6.141e-14, against the quadratic form's
                     columns 2.220e-16 -> 2.220e-15; rho 5.773e-15 -> 5.773e-14
    approximations   betas 5.322e-11 -> 5.322e-10
    gauss_newton     betas 6.035e-09 -> 6.035e-08
    compute_R_and_t  R 1.141e-14 -> 1.141e-13, t 8.493e-15 -> 8.493e-14, error (relative) 3.892e-08 ->
                     3.892e-07; the sign flip and the determinant branch equal
    the chain        R 3.527e-10 -> 3.527e-09, t 3.728e-09 -> 3.728e-08, error (relative) 5.742e-07 ->
                     5.742e-06, which is also the tie margin for the candidate N
    jacobi_svd       reconstruction 9.139e-16 -> 9.139e-15, orthonormal rows 2.220e-15 -> 2.220e-14,
                     singular values 1.474e-15 -> 1.474e-14 (first and last relative to the largest value)

The conditions (condition-number cap 1e6, branch guard 1e-6, eigenvalue floor 1e-12, singular-value
gap 1e-6; epnp_stage_checks.py states why) left out 1 case of 940 (a beta_1^2 within 1e-6 of 0)."""
import pathlib
import shutil
import subprocess
import sys

import numpy as np
import pytest

import epnp_reference as ref
import epnp_stage_checks as sc
import pnp_solver_model as pm

ROOT = pathlib.Path(__file__).resolve().parents[1]
K64 = sc.K64
BOUNDS = {"cws_centroid": 1e-15, "cws_radius": 5.808e-12, "cws_direction": 4.707e-13,
          "alphas_sum": 1.332e-14, "alphas_points": 3.997e-14, "ci": 5.116e-12,
          "svd_orth": 2.248e-14, "svd_mtm": 1.777e-14, "svd_w": 2.659e-14,
          "l_definition": 6.141e-14, "l_columns": 2.220e-15, "rho": 5.773e-14,
          "approx": 5.322e-10, "gn": 6.035e-08,
          "pose_R": 1.141e-13, "pose_t": 8.493e-14, "pose_rep": 3.892e-07, "pose_flags": 0.0,
          "chain_R": 3.527e-09, "chain_t": 3.728e-08, "chain_rep": 5.742e-06}
TIE_MARGIN = BOUNDS["chain_rep"]
SVD_BOUNDS = {"reconstruction": 9.139e-15, "orthonormal": 2.220e-14, "values": 1.474e-14}
# noise-free n-point scenes (n = 5 + seed % 41) whose first two errors are equal to the bit: both
# Gauss-Newton runs end on the same betas.  (30 000 noise-free four-point sets held no such tie.)
TIE_SEEDS = (8, 42, 44, 85)


def collect(cases):
    return [(name, *sc.differences(p3, p2, sel)) for name, p3, p2, sel in cases]


@pytest.fixture(scope="module")
def table():
    return collect(sc.general_cases())


def hold(table, keys):
    """Every difference under `keys` (a key ending in N stands for the three approximations) within its
    bound, over every case that has it; prints the largest."""
    for key in keys:
        names = [key.replace("N", str(N)) for N in (1, 2, 3)] if "N" in key else [key]
        bound = BOUNDS[key.replace("N", "")]
        got = [(d[k], name) for name, d, _, _ in table for k in names if k in d]
        assert got, key
        worst, where = max(got, key=lambda g: (np.isnan(g[0]), g[0]))
        print(f"{key}: {worst:.3e} (bound {bound:.3e}) at {where}, {len(got)} comparisons")
        assert worst <= bound, f"{key}: {worst:.3e} > {bound:.3e} at {where}"


# ---- the stages, each fed the header's own upstream value ------------------------------------------------
def check_control_points(table):
    hold(table, ["cws_centroid", "cws_radius", "cws_direction"])


def check_alphas(table):
    hold(table, ["alphas_sum", "alphas_points", "ci"])


def check_mtm_svd(table):
    hold(table, ["svd_orth", "svd_mtm", "svd_w"])


def check_l_and_rho(table):
    hold(table, ["l_definition", "l_columns", "rho"])


def check_approximations(table):
    hold(table, ["approxN"])


def check_gauss_newton(table):
    hold(table, ["gnN"])


def check_pose(table):
    hold(table, ["poseN_R", "poseN_t", "poseN_rep", "poseN_flags"])


def check_chain(table):
    hold(table, ["chainN_R", "chainN_t", "chainN_rep"])


def check_selection(table, cases):
    """The exported N is the strict rule on the header's own three errors (a tie keeps the lower N), and
    compute_pose returns that N's pose, error and branch bits."""
    for (name, _, h, _), (_, p3, p2, sel) in zip(table, cases):
        N = ref.strict_choice(h["rep_error"])
        assert h["N"] == N, name
        m = pm.compute_pose(p3, p2, K64, sel)
        assert m["R"].tobytes() == h["R"][N - 1].tobytes() and m["t"].tobytes() == h["t"][N - 1].tobytes(), name
        assert np.float64(m["rep_error"]).tobytes() == h["rep_error"][N - 1].tobytes(), name
        assert m["branches"] == h["branches"], name
        assert (bool(m["branches"] & pm.BR["N2"]), bool(m["branches"] & pm.BR["N3"])) == (N == 2, N == 3), name


def tie_cases():
    return [(f"tie/{s}", *pm.scene(5 + s % 41, s)[:2], None) for s in TIE_SEEDS]


def test_control_points(table):
    check_control_points(table)


def test_alphas(table):
    check_alphas(table)


def test_mtm_svd(table):
    check_mtm_svd(table)


def test_l_and_rho(table):
    check_l_and_rho(table)


def test_approximations(table):
    check_approximations(table)


def test_gauss_newton(table):
    check_gauss_newton(table)


def test_pose(table):
    check_pose(table)


def test_chain(table):
    check_chain(table)


def test_selection(table):
    check_selection(table, sc.general_cases())
    ties = tie_cases()
    tt = collect(ties)
    for name, _, h, _ in tt:
        assert h["rep_error"][0] == h["rep_error"][1] and h["N"] != 2, f"{name} no longer ties"
    check_selection(tt, ties)


def test_conditions_leave_few_cases_out(table):
    out = {}
    for _, d, _, _ in table:
        for k in d["outside"]:
            out[k] = out.get(k, 0) + 1
    print(f"left out of {len(table)}: {out}")
    assert all(v <= 0.05 * len(table) for v in out.values()), out


def test_coverage(table):
    """Enough cases choose each N clearly (the runner-up more than 0.1 % above), and enough take each
    branch of the approximations and of the pose."""
    clear = {1: 0, 2: 0, 3: 0}
    for _, _, h, _ in table:
        e = np.sort(h["rep_error"])
        if e[1] > e[0] * 1.001:
            clear[h["N"]] += 1
    taken = {b: sum(bool(h["branches"] & pm.BR[b]) for _, _, h, _ in table)
             for b in ("DET_NEG", "SIGN_FLIP", "B_NEG", "B1_NEG", "B_POS")}
    print(f"clear choices {clear}, branches {taken}")
    assert min(clear.values()) >= 20 and min(taken.values()) >= 20


def test_degenerate_sets():
    """The degenerate sets of test_gpu_pnp_solver.py.  What stays defined and is asserted: the centroid,
    the control-point offsets whose eigenvalue is not null, the alphas (rows sum to 1, alphas @ cws
    gives back the points: the pseudo-inverse of a singular CC still spans them), the decomposition of
    M^T M, L by its definition and rho, the selection rule.  Not asserted: ci (CC is singular) and, but
    for the point behind the camera, everything from the betas on (the solves are singular, the
    betas reach 1e96 or NaN).  Behind the camera the geometry is general: every stage is asserted."""
    import test_gpu_pnp_solver as tg

    deg = tg.degenerate_cases()
    cases = [(f"{name}/{k}", deg[name][0], deg[name][1], np.int32(s))
             for name in ("coplanar", "repeated", "identical", "behind") for k, s in enumerate(deg[name][2])]
    t = [(name, *sc.differences(p3, p2, sel, downstream=name.startswith("behind"))) for name, p3, p2, sel in cases]
    front = ["cws_centroid", "cws_radius", "alphas_sum", "alphas_points", "svd_orth", "svd_mtm", "svd_w",
             "l_definition", "l_columns", "rho"]
    hold(t, front)
    assert all("eig" in d["outside"] for name, d, _, _ in t if not name.startswith("behind"))
    behind = [r for r in t if r[0].startswith("behind")]
    assert behind and not behind[0][1]["outside"]
    for check in (check_control_points, check_alphas, check_approximations, check_gauss_newton, check_pose, check_chain):
        check(behind)
    check_selection(t, cases)


# ---- the Jacobi SVD on its own --------------------------------------------------------------------------
def test_jacobi_svd():
    worst = sc.jacobi_svd_differences()
    print({k: f"{v:.3e} (bound {SVD_BOUNDS[k]:.3e})" for k, v in worst.items()})
    assert all(worst[k] <= SVD_BOUNDS[k] for k in worst), worst


@pytest.mark.parametrize("m,n", sc.SVD_SHAPES)
def test_jacobi_svd_rank_deficient(m, n):
    """All-zero, rank 1 (one column; a general outer product) and two equal singular values (exactly,
    and rotated).  A row whose singular value came out null is refilled (BR_SVD_FILL): its W stays 0
    and it is a unit vector orthogonal to every earlier row.  Of two equal values the first stays first.

    The all-zero 6 x 5 is the case that found the header's second repair: the fifth
    vector of six signs that cv::RNG(0x12345678) yields is the exact negative of the fourth, its
    projections left rounding noise that the 1-norm renormalisation scaled back to order 1, and row 4
    came out with a dot product of 8.868e-01 with an earlier row.  The header now takes the next
    random vector when one collapses."""
    rng = np.random.default_rng(m * 13 + n)
    u, v = rng.normal(size=m), rng.normal(size=n)
    Q, _ = np.linalg.qr(rng.normal(size=(m, m)))
    P, _ = np.linalg.qr(rng.normal(size=(n, n)))
    col = np.zeros((m, n))
    col[:, 0] = u
    E = np.zeros((m, n))  # columns 0 and 1 are 3 e_0 and 3 e_1, column 2 is e_2
    E[0, 0] = E[1, 1] = 3.0
    E[2, 2] = 1.0
    s_eq = np.zeros(n)
    s_eq[:2] = 3.0
    tiny = np.finfo(np.float64).tiny
    not_orthogonal = []
    for name, A, rank, fills in (("zero", np.zeros((m, n)), 0, True), ("one column", col, 1, True),
                                 ("outer product", np.outer(u, v), 1, False), ("equal, exact", E, 3, n > 3),
                                 ("equal, rotated", Q[:, :n] @ np.diag(s_eq) @ P.T, 2, False)):
        Ut, W, Vt, br = pm.jacobi_svd(A)
        s = np.linalg.svd(A, compute_uv=False)
        scale = s[0] if s[0] > 0 else 1.0
        assert (np.diff(W) <= 0).all(), name
        assert np.abs(W - s).max() <= SVD_BOUNDS["values"] * scale, name
        assert np.abs(Ut[:n].T @ np.diag(W) @ Vt - A).max() <= SVD_BOUNDS["reconstruction"] * scale, name
        assert np.abs(Vt @ Vt.T - np.eye(n)).max() <= SVD_BOUNDS["orthonormal"], name
        assert not rank or np.abs(Ut[:rank] @ Ut[:rank].T - np.eye(rank)).max() <= SVD_BOUNDS["orthonormal"], name
        refilled = np.flatnonzero(W <= tiny)
        assert bool(br & pm.BR["SVD_FILL"]) == (refilled.size > 0), name
        if fills:
            assert refilled.tolist() == list(range(rank, n)), name
        for i in refilled:
            assert W[i] == 0, name
            assert abs(Ut[i] @ Ut[i] - 1) <= SVD_BOUNDS["orthonormal"], name
            if i and np.abs(Ut[:i] @ Ut[i]).max() > SVD_BOUNDS["orthonormal"]:
                not_orthogonal.append(f"{name}: row {i}, {np.abs(Ut[:i] @ Ut[i]).max():.3e}")
        if name == "equal, exact":  # column 0's vector before column 1's
            assert W[0] == W[1] == 3.0 and abs(Ut[0, 0]) == 1.0 and abs(Ut[1, 1]) == 1.0
            assert abs(Vt[0, 0]) == 1.0 and abs(Vt[1, 1]) == 1.0
    assert not not_orthogonal, not_orthogonal


# ---- mutants of the header ------------------------------------------------------------------------------
HEADER = pathlib.Path("orbslam_jpminipc_amd") / "csrc" / "orb_epnp_math.h"
MODEL = pathlib.Path("tests") / "native" / "pnp_solver_model.cpp"
FLIP = "        Rm[2][0] = -Rm[2][0];\n        Rm[2][1] = -Rm[2][1];\n        Rm[2][2] = -Rm[2][2];\n"
MUTANTS = {
    "approx_3 takes beta_2 from the wrong product": (
        "betas[2] = b5[3] / betas[0];", "betas[2] = b5[4] / betas[0];", "check_approximations"),
    "approx_2 takes beta_1 from beta_0*beta_1": (
        "betas[1] = (b3[2] > 0) ? sqrt(b3[2]) : 0.0;", "betas[1] = (b3[2] > 0) ? sqrt(b3[1]) : 0.0;",
        "check_approximations"),
    "a factor 2 missing in compute_L_6x10": (
        "row[4] = 2.0 * dot3(dv[1][i], dv[2][i]);", "row[4] = dot3(dv[1][i], dv[2][i]);", "check_l_and_rho"),
    "a factor 2 missing in the Gauss-Newton Jacobian": (
        "fma_(2 * rowL[5], b2,", "fma_(rowL[5], b2,", "check_gauss_newton"),
    "the determinant flip negates the second row": (FLIP, FLIP.replace("Rm[2]", "Rm[1]"), "check_pose"),
    "solve_for_sign removed": ("if (pc[2] < 0.0) {", "if (false && pc[2] < 0.0) {", "check_pose"),
    "a tie takes the later N": (
        "if (rep < best) {  // rep_errors[2] < rep_errors[1]", "if (rep <= best) {  // rep_errors[2] < rep_errors[1]",
        "check_selection"),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_fails_its_stage(name, tmp_path, monkeypatch):
    """The header with one statement changed, built with the model under the same relative layout: the
    check of the stage where the change sits must fail, and passes again on the unmodified build."""
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge

    old, new, check = MUTANTS[name]
    for rel in (HEADER, MODEL):
        (tmp_path / rel).parent.mkdir(parents=True)
        shutil.copy(ROOT / rel, tmp_path / rel)
    text = (tmp_path / HEADER).read_text()
    assert text.count(old) == 1, f"{old!r} matches {text.count(old)} times"
    (tmp_path / HEADER).write_text(text.replace(old, new))
    so = tmp_path / "libpnp_solver_model_mutant.so"
    cmd = ge.PNP_SOLVER_MODEL_CMD(so)
    assert cmd[-1] == str(ROOT / MODEL) and "-O3" in cmd
    cmd[-1] = str(tmp_path / MODEL)
    subprocess.run(["-O1" if c == "-O3" else c for c in cmd], check=True)

    cases = sc.general_cases()[::4] + tie_cases()
    run = (lambda t: check_selection(t, cases)) if check == "check_selection" else globals()[check]
    run(collect(cases))
    with monkeypatch.context() as mp:
        mp.setattr(pm, "_lib", pm.load(so))
        with pytest.raises(AssertionError):
            run(collect(cases))
