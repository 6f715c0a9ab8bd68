"""The inputs of the EPnP stage tests and, for one input, the difference between every stage the model
exports (pnp_solver_model.stages: csrc/orb_epnp_math.h on the host) and tests/epnp_reference.py.

Shared by tests/test_epnp_stages.py (which bounds the differences), scripts/measure_epnp_stage_bounds.py
(which prints the largest, the bounds being 10 x those) and tests/test_gpu_epnp_reference.py.

The conditions under which a comparison is made are stated here and are not measurements:

- COND_CAP: an approximation's betas are compared while its sub-matrix of L has a condition number
  under the cap; Gauss-Newton's while every Jacobian on the way has; the chain's while both have.
  A least-squares solution moves by (condition number) x (rounding), so past 1e6 two correct solvers
  agree to fewer than ten digits and five further steps multiply that.
- BRANCH_GUARD: the approximations decide a sign or a zero from the sign of a solved product
  (beta_0^2, beta_1^2, beta_0*beta_1).  Where such a product is within the guard of 0, relative to the
  largest product, two correct solvers may decide differently: such a case is not compared.
- EIG_FLOOR: a control-point direction is compared while its eigenvalue is at least the floor times the
  largest (under it the direction is that of rounding noise); CC's inverse while CC's condition
  number is under COND_CAP.
- GAP_FLOOR: the rotation of the absolute orientation is compared while the second singular value of
  the cross-covariance is at least the floor times the first.

Each may leave out at most 5 % of the cases (test_conditions_leave_few_cases_out)."""
import numpy as np

import epnp_reference as ref
import pnp_solver_model as pm

f32 = np.float32
K64 = np.float64(f32(pm.K_CAM))
COND_CAP = 1e6
BRANCH_GUARD = 1e-6
EIG_FLOOR = 1e-12
GAP_FLOOR = 1e-6


def general_cases():
    """(name, p3d, p2d, sel) over pm.scene: four points without noise (600) and with 1 px (200), five
    points (60, every other one with 1 px), 6 to 45 points with 1 px (80)."""
    out = []
    for seed in range(600):
        out.append((f"four/{seed}", *pm.scene(4, seed)[:2], None))
    for seed in range(1000, 1200):
        out.append((f"four-noisy/{seed}", *pm.scene(4, seed, noise=1.0)[:2], None))
    for seed in range(2000, 2060):
        out.append((f"five/{seed}", *pm.scene(5, seed, noise=float(seed % 2))[:2], None))
    for seed in range(3000, 3080):
        out.append((f"many/{seed}", *pm.scene(6 + seed % 40, seed, noise=1.0)[:2], None))
    return out


def rel(a, b):
    return abs(a - b) / max(abs(b), np.finfo(np.float64).tiny)


def near_branch(x):
    """Whether a product that decides a branch is within the guard of 0."""
    big = max(abs(v) for v in x.values())
    keys = [(0, 0)] + ([(1, 1), (0, 1)] if (1, 1) in x else [])
    return any(abs(x[k]) <= BRANCH_GUARD * big for k in keys)


def differences(p3d, p2d, sel=None, K=K64, rng=None, downstream=True):
    """{stage: difference} of one input, each stage fed the header's own upstream value, then the chain.
    A stage whose condition fails is absent and named in d["outside"].  downstream=False stops before
    the betas (a degenerate input, whose solves are singular)."""
    rng = rng or np.random.default_rng(0)
    h = pm.stages(p3d, p2d, K, sel)
    idx = np.arange(len(p3d)) if sel is None else np.asarray(sel)
    pw, us = np.float64(p3d)[idx], np.float64(p2d)[idx]
    d, outside = {}, set()

    e_c, e_r, e_d, skipped = ref.control_point_errors(h["cws"], pw, EIG_FLOOR)
    d.update(cws_centroid=e_c, cws_radius=e_r, cws_direction=e_d)
    if skipped:
        outside.add("eig")
    e_sum, e_pw, e_ci = ref.alpha_errors(h["alphas"], h["cws"], pw, h["ci"], COND_CAP)
    d.update(alphas_sum=e_sum, alphas_points=e_pw)
    if e_ci is None:
        outside.add("ci")
    else:
        d["ci"] = e_ci
    d["svd_orth"], d["svd_mtm"], d["svd_w"] = ref.mtm_svd_errors(h["ut"], h["w"], ref.build_m(h["alphas"], us, K))
    V = ref.basis_of(h["ut"])
    d["l_definition"] = ref.l_definition_error(h["l_6x10"], V, rng)
    d["l_columns"] = np.abs(h["l_6x10"] - ref.l_of(V)).max()
    d["rho"] = max(ref.rho_error(h["rho"], h["cws"]), np.abs(h["rho"] - ref.rho_of(pw)).max())

    d["outside"] = outside
    if not downstream:
        return d, h, None
    for N in (1, 2, 3):
        k = N - 1
        x, cond, dropped = ref.approx_solve(h["l_6x10"], h["rho"], N)
        skip_bit = bool(h["br_n"][k] & pm.BR["BKSB_SKIP"])
        if near_branch(x):
            outside.add(f"branch{N}")
        elif cond >= COND_CAP and not (dropped and skip_bit):
            outside.add(f"cond{N}")
        else:
            d[f"approx{N}"] = np.abs(h["betas0"][k] - ref.approx_betas(h["l_6x10"], h["rho"], N)[0]).max()
        b, cond_j = ref.gauss_newton(h["l_6x10"], h["rho"], h["betas0"][k])
        if cond_j >= COND_CAP:
            outside.add(f"gn{N}")
        else:
            d[f"gn{N}"] = np.abs(h["betas"][k] - b).max()
        p = ref.pose_of(h["betas"][k], V, h["alphas"], pw, us, K)
        if p["gap"] < GAP_FLOOR:
            outside.add(f"gap{N}")
        else:
            d[f"pose{N}_R"] = np.abs(h["R"][k] - p["R"]).max()
            d[f"pose{N}_t"] = np.abs(h["t"][k] - p["t"]).max()
            d[f"pose{N}_rep"] = rel(h["rep_error"][k], p["rep_error"])
            d[f"pose{N}_flags"] = float(p["sign_flip"] != bool(h["br_n"][k] & pm.BR["SIGN_FLIP"])
                                        or p["det_neg"] != bool(h["br_n"][k] & pm.BR["DET_NEG"]))

    ch = ref.chain(h["ut"], h["alphas"], pw, us, K)
    for N in (1, 2, 3):
        k = N - 1
        if not chain_comparable(ch[k]):
            outside.add(f"chain{N}")
            continue
        d[f"chain{N}_R"] = np.abs(h["R"][k] - ch[k]["R"]).max()
        d[f"chain{N}_t"] = np.abs(h["t"][k] - ch[k]["t"]).max()
        d[f"chain{N}_rep"] = rel(h["rep_error"][k], ch[k]["rep_error"])
    d["outside"] = outside
    return d, h, ch


SVD_SHAPES = [(3, 3), (6, 3), (6, 4), (6, 5), (12, 12)]


def jacobi_svd_differences():
    """The header's jacobi_svd on 20 random full-rank matrices of every shape it is called with, scales
    from 1e-3 to 1e3: the largest (reconstruction, orthonormality, singular values against
    np.linalg.svd); the values come out descending and the run without vt gives the same bits."""
    rng = np.random.default_rng(17)
    worst = {"reconstruction": 0.0, "orthonormal": 0.0, "values": 0.0}
    for m, n in SVD_SHAPES:
        for _ in range(20):
            A = rng.normal(size=(m, n)) * 10.0 ** rng.integers(-3, 4)
            Ut, W, Vt, _ = pm.jacobi_svd(A)
            e_rec, e_orth, e_w, descending = ref.svd_errors(A, Ut, W, Vt)
            assert descending, (m, n)
            for k, v in zip(worst, (e_rec, e_orth, e_w)):
                worst[k] = max(worst[k], v)
            Ut2, W2, _, _ = pm.jacobi_svd(A, want_vt=False)
            assert Ut2.tobytes() == Ut.tobytes() and W2.tobytes() == W.tobytes(), (m, n)
    return worst


def chain_comparable(c):
    """The chain's conditions for one approximation: condition numbers, no product near a branch, a
    determined rotation."""
    return c["cond"] < COND_CAP and c["gap"] >= GAP_FLOOR and not near_branch(c["products"])
