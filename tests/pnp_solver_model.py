"""ctypes loader of the CPU model of the PnPsolver hypotheses and RANSAC (tests/native/pnp_solver_model.cpp,
built to build/libpnp_solver_model.so by __graft_entry__.build()): the sampler of PnPsolver::iterate
on a std::vector, EPnP's compute_pose, CheckInliers, the keep-the-best rule and Refine, restated; and
what every step of compute_pose left behind (stages) and the header's Jacobi SVD on its own
(jacobi_svd), for tests/epnp_reference.py to be compared with.

Also the shared synthetic scenes of the PnP solver tests and an independent float64 EPnP in numpy."""
import ctypes
import pathlib
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
LIB = ROOT / "build" / "libpnp_solver_model.so"
_lib = None

BRANCHES = ["SVD_SKIP", "SVD_BETA_NEG", "SVD_BETA_POS", "SVD_SWAP", "SVD_FILL", "BKSB_SKIP", "B_NEG", "B_POS", "B1_NEG",
            "QR_ETA0", "QR_SIGMA_NEG", "SIGN_FLIP", "DET_NEG", "N2", "N3"]
BR = {name: 1 << k for k, name in enumerate(BRANCHES)}
BR_ALL = (1 << len(BRANCHES)) - 1


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not LIB.exists():  # build() makes it; a tree that skipped build() compiles it here (g++, seconds)
            sys.path.insert(0, str(ROOT))
            import __graft_entry__ as ge

            LIB.parent.mkdir(exist_ok=True)
            subprocess.run(ge.PNP_SOLVER_MODEL_CMD(LIB), check=True)
        _lib = load(LIB)
    return _lib


def load(path) -> ctypes.CDLL:
    """A build of the model with its prototypes (lib() is this on build/; the mutant test loads others)."""
    so = ctypes.CDLL(str(path))
    vp, i, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
    so.pnp_solver_model_random_int.restype = i
    so.pnp_solver_model_random_int.argtypes = [i, i]
    so.pnp_solver_model_sets.restype = i
    so.pnp_solver_model_sets.argtypes = [i, i, vp, vp]
    so.pnp_solver_model_mapping.restype = i
    so.pnp_solver_model_mapping.argtypes = [i, i, i, vp, vp]
    so.pnp_solver_model_qr_solve.restype = u
    so.pnp_solver_model_qr_solve.argtypes = [vp, vp, vp]
    so.pnp_solver_model_compute_pose.restype = u
    so.pnp_solver_model_compute_pose.argtypes = [i, vp, vp, vp, i, vp, vp, vp, vp]
    so.pnp_solver_model_stages.restype = u
    so.pnp_solver_model_stages.argtypes = [i, vp, vp, vp, i, vp] + [vp] * 14
    so.pnp_solver_model_jacobi_svd.restype = u
    so.pnp_solver_model_jacobi_svd.argtypes = [i, i, i, i, vp, vp, vp]
    so.pnp_solver_model_ransac.restype = i
    so.pnp_solver_model_ransac.argtypes = [i, vp, vp, vp, ctypes.c_float, vp, i, vp, vp, i, i] + [vp] * 17
    return so


def _p(a):
    return ctypes.c_void_p(None if a is None else a.ctypes.data)


def _f32(a, cols):
    return np.ascontiguousarray(a, np.float32).reshape(-1, cols)


def sets(N: int, rand31) -> np.ndarray:
    """The minimal sets of PnPsolver.cc:160-173 from n_hyp x 4 rand() values, on a std::vector."""
    r = np.ascontiguousarray(rand31, np.int32).reshape(-1, 4)
    out = np.zeros((len(r), 4), np.int32)
    assert lib().pnp_solver_model_sets(int(N), len(r), _p(r), _p(out)) == 0
    return out


def mapping(K: int, N: int, rand31) -> np.ndarray:
    """The kernels' closed-form mapping (csrc/orb_epnp_math.h minimal_set<K>) compiled for the host."""
    r = np.ascontiguousarray(rand31, np.int32).reshape(-1, K)
    out = np.zeros((len(r), K), np.int32)
    assert lib().pnp_solver_model_mapping(int(K), int(N), len(r), _p(r), _p(out)) == 0
    return out


def qr_solve(A, b, x0=None):
    """PnPsolver::qr_solve on a 6 x 4: (x, branch mask); x is x0 (zeros) untouched on the early return."""
    A = np.array(A, np.float64).reshape(6, 4)
    b = np.array(b, np.float64).reshape(6)
    x = np.zeros(4) if x0 is None else np.array(x0, np.float64).reshape(4)
    br = lib().pnp_solver_model_qr_solve(_p(A), _p(b), _p(x))
    return x, br


def compute_pose(p3d, p2d, K, sel=None) -> dict:
    """compute_pose on the correspondences `sel` (in that order; all when None)."""
    p3d, p2d = _f32(p3d, 3), _f32(p2d, 2)
    Kd = np.ascontiguousarray(K, np.float64).reshape(4)
    s = None if sel is None else np.ascontiguousarray(sel, np.int32).reshape(-1)
    R, t, e = np.zeros((3, 3)), np.zeros(3), np.zeros(1)
    br = lib().pnp_solver_model_compute_pose(len(p3d), _p(p3d), _p(p2d), _p(Kd), 0 if s is None else len(s), _p(s),
                                             _p(R), _p(t), _p(e))
    return {"R": R, "t": t, "rep_error": float(e[0]), "branches": int(br)}


def stages(p3d, p2d, K, sel=None) -> dict:
    """What every step of compute_pose left behind on the correspondences `sel` (all when None): cws, ci,
    alphas, ut and w of mtm_svd, l_6x10, rho; per N = 1, 2, 3 (first axis) betas0 after
    find_betas_approx_N, betas after gauss_newton, R, t, rep_error; N the strict `<` picks; br_front,
    br_n (3) and branches, the masks of the steps before the betas, of each N and of the whole call."""
    p3d, p2d = _f32(p3d, 3), _f32(p2d, 2)
    Kd = np.ascontiguousarray(K, np.float64).reshape(4)
    s = None if sel is None else np.ascontiguousarray(sel, np.int32).reshape(-1)
    n = len(p3d) if s is None else len(s)
    o = {"cws": np.zeros((4, 3)), "ci": np.zeros((3, 3)), "alphas": np.zeros((n, 4)), "ut": np.zeros((12, 12)),
         "w": np.zeros(12), "l_6x10": np.zeros((6, 10)), "rho": np.zeros(6), "betas0": np.zeros((3, 4)),
         "betas": np.zeros((3, 4)), "R": np.zeros((3, 3, 3)), "t": np.zeros((3, 3)), "rep_error": np.zeros(3),
         "N": np.zeros(1, np.int32), "br": np.zeros(5, np.uint32)}
    br = lib().pnp_solver_model_stages(len(p3d), _p(p3d), _p(p2d), _p(Kd), 0 if s is None else len(s), _p(s),
                                       *[_p(v) for v in o.values()])
    br5 = o.pop("br")
    assert int(br5[4]) == br
    o["N"] = int(o["N"][0])
    o.update(br_front=int(br5[0]), br_n=[int(b) for b in br5[1:4]], branches=int(br))
    return o


def jacobi_svd(A, want_vt=True, n1=None):
    """The header's jacobi_svd on A (m x n, n <= m): its work matrix is transpose(A), n1 >= n rows of m.
    Returns (Ut n1 x m, W n, Vt n x n or None, branch mask): A = Ut[:n].T @ diag(W) @ Vt."""
    A = np.array(A, np.float64)
    m, n = A.shape
    n1 = n if n1 is None else int(n1)
    At = np.zeros((n1, m))
    At[:n] = A.T
    W, Vt = np.zeros(n), np.zeros((n, n))
    br = lib().pnp_solver_model_jacobi_svd(m, n, n1, int(bool(want_vt)), _p(At), _p(W), _p(Vt))
    return At, W, (Vt if want_vt else None), int(br)


def ransac(p3d, p2d, sigma2, th2, K, min_inliers, sets=None, rand31=None, best_in=0) -> dict:
    """PnPsolver::iterate over the n_hyp iterations of the given sets or draws (see the C++ header)."""
    p3d, p2d = _f32(p3d, 3), _f32(p2d, 2)
    n = len(p3d)
    s2 = np.ascontiguousarray(sigma2, np.float32).reshape(-1)
    Kd = np.ascontiguousarray(K, np.float64).reshape(4)
    d = np.ascontiguousarray(sets if sets is not None else rand31, np.int32).reshape(-1, 4)
    H, W = len(d), (n + 63) // 64
    o = {"counts": np.zeros(H, np.int32), "masks": np.zeros((H, W), np.uint64), "best_at": np.zeros(H, np.int32),
         "first_ok": np.zeros(1, np.int32), "R": np.zeros((H, 9)), "t": np.zeros((H, 3)), "rep_error": np.zeros(H),
         "sets": np.zeros((H, 4), np.int32), "branches": np.zeros(H, np.uint32),
         "refined_counts": np.zeros(H, np.int32), "refined_R": np.zeros((H, 9)), "refined_t": np.zeros((H, 3)),
         "first_refined": np.zeros(1, np.int32), "pose": np.zeros(12, np.float32), "pose_mask": np.zeros(W, np.uint64),
         "pose_inliers": np.zeros(1, np.int32), "refine_calls": np.zeros(1, np.int32)}
    r = lib().pnp_solver_model_ransac(n, _p(p3d), _p(p2d), _p(s2), ctypes.c_float(float(th2)), _p(Kd), H,
                                      _p(d) if sets is not None else None, None if sets is not None else _p(d),
                                      int(min_inliers), int(best_in), *[_p(v) for v in o.values()])
    assert r == 0, r
    for k in ("first_ok", "first_refined", "pose_inliers", "refine_calls"):
        o[k] = int(o[k][0])
    return o


# ---- synthetic scenes ----------------------------------------------------------------------------------

K_CAM = (517.3, 516.5, 318.6, 255.3)


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = np.asarray(w) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def scene(n, seed, noise=0.0, outliers=0.0, K=K_CAM):
    """n world points in front of a random camera: (p3d float32, p2d float32, R, t) with p2d the
    projection of the float32 points, `noise` pixels of Gaussian noise, a fraction of gross outliers."""
    rng = np.random.default_rng(seed)
    R = rodrigues(rng.normal(size=3) * 0.4)
    t = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(3.5, 5.0)])
    p3 = rng.uniform(-1.5, 1.5, size=(n, 3)).astype(np.float32)
    pc = p3.astype(np.float64) @ R.T + t
    p2 = np.stack([K[2] + K[0] * pc[:, 0] / pc[:, 2], K[3] + K[1] * pc[:, 1] / pc[:, 2]], 1)
    p2 += rng.normal(size=p2.shape) * noise
    bad = rng.random(n) < outliers
    p2[bad] = rng.uniform(0, 480, size=(int(bad.sum()), 2))
    return p3, p2.astype(np.float32), R, t


def draws(n_hyp, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 31, size=(n_hyp, 4), dtype=np.int64).astype(np.int32)


# ---- an independent float64 EPnP (np.linalg.svd / lstsq) ------------------------------------------------


def numpy_epnp(p3d, p2d, K):
    """EPnP with the one-dimensional null space only (betas = [b, 0, 0, 0]): valid for n >= 6 points in
    general position without noise, where M has exactly one null vector.  Returns (R, t)."""
    fu, fv, uc, vc = K
    pw = np.asarray(p3d, np.float64)
    us = np.asarray(p2d, np.float64)
    n = len(pw)
    c0 = pw.mean(0)
    w, V = np.linalg.eigh((pw - c0).T @ (pw - c0))
    cws = np.vstack([c0] + [c0 + np.sqrt(w[k] / n) * V[:, k] for k in (2, 1, 0)])
    C = (cws[1:] - cws[0]).T
    a123 = np.linalg.solve(C, (pw - c0).T).T
    al = np.hstack([1 - a123.sum(1, keepdims=True), a123])
    M = np.zeros((2 * n, 12))
    for j in range(4):
        M[0::2, 3 * j] = al[:, j] * fu
        M[0::2, 3 * j + 2] = al[:, j] * (uc - us[:, 0])
        M[1::2, 3 * j + 1] = al[:, j] * fv
        M[1::2, 3 * j + 2] = al[:, j] * (vc - us[:, 1])
    v = np.linalg.svd(M)[2][-1].reshape(4, 3)
    # the scale from the control points' mutual distances, least squares
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    dv = np.array([np.linalg.norm(v[a] - v[b]) for a, b in pairs])
    dw = np.array([np.linalg.norm(cws[a] - cws[b]) for a, b in pairs])
    beta = (dv @ dw) / (dv @ dv)
    ccs = beta * v
    pcs = al @ ccs
    if pcs[0, 2] < 0:
        pcs = -pcs
    pc0, pw0 = pcs.mean(0), pw.mean(0)
    U, _, Vt = np.linalg.svd((pcs - pc0).T @ (pw - pw0))
    R = U @ Vt
    if np.linalg.det(R) < 0:
        R[2] = -R[2]
    return R, pc0 - R @ pw0
