"""ctypes loader of the CPU model of the Sim3Solver hypotheses (tests/native/sim3_solver_model.cpp,
built to build/libsim3_solver_model.so by __graft_entry__.build()): the sampler of
Sim3Solver::iterate, cv::eigen's Jacobi and computeT, restated.  CheckInliers and the keep-the-best
rule are the existing solvers model's (tests/solvers_model.py), so ``iterate`` here is the sampler,
computeT and that model in sequence, and ``Solver`` carries iterate's counters across calls as
Sim3Solver.cc:140-213 does.

Also the shared synthetic cloud of the Sim3 solver tests and an independent float64 Horn solution."""
import ctypes
import pathlib
import subprocess
import sys

import numpy as np

import solvers_model

ROOT = pathlib.Path(__file__).resolve().parents[1]
LIB = ROOT / "build" / "libsim3_solver_model.so"
FIXED_SAMPLER = 1  # variant bits (tests only)
_lib = None


def libm_variant(atan2=0, cos=0, sin=0) -> int:
    """The variant bits that move a libm result by one ulp: 0 = as is, 1 = up, 2 = down."""
    return (atan2 << 1) | (cos << 3) | (sin << 5)


LIBM_VARIANTS = [libm_variant(a, c, s) for a in range(3) for c in range(3) for s in range(3)][1:]


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not LIB.exists():  # build() makes it; a tree that skipped build() compiles it here (g++, seconds)
            sys.path.insert(0, str(ROOT))
            import __graft_entry__ as ge

            LIB.parent.mkdir(exist_ok=True)
            subprocess.run(ge.SIM3_SOLVER_MODEL_CMD(LIB), check=True)
        _lib = ctypes.CDLL(str(LIB))
        vp, i = ctypes.c_void_p, ctypes.c_int
        _lib.sim3_solver_model_sets.restype = i
        _lib.sim3_solver_model_sets.argtypes = [i, i, vp, i, vp]
        _lib.sim3_solver_model_random_int.restype = i
        _lib.sim3_solver_model_random_int.argtypes = [i, i]
        _lib.sim3_solver_model_jacobi.restype = i
        _lib.sim3_solver_model_jacobi.argtypes = [vp, vp, vp]
        _lib.sim3_solver_model_compute.restype = i
        _lib.sim3_solver_model_compute.argtypes = [i, vp, vp, i, vp, i, vp, vp, vp, vp]
    return _lib


def _p(a):
    return ctypes.c_void_p(None if a is None else a.ctypes.data)


def _f32(a, cols=0):
    a = np.ascontiguousarray(a, np.float32)
    return a.reshape(-1, cols) if cols else a.reshape(-1)


def random_int(r: int, d: int) -> int:
    """DUtils::Random::RandomInt(0, d - 1) on rand()'s value r, the double expression."""
    return lib().sim3_solver_model_random_int(int(r), int(d))


def sets(N: int, rand31, variant: int = 0) -> np.ndarray:
    r = np.ascontiguousarray(rand31, np.int32).reshape(-1, 3)
    out = np.zeros((len(r), 3), np.int32)
    assert lib().sim3_solver_model_sets(int(N), len(r), _p(r), int(variant), _p(out)) == 0
    return out


def jacobi(A):
    """cv::eigen of a symmetric 4x4 float32: (eigenvalues descending, eigenvectors as rows)."""
    A = np.ascontiguousarray(A, np.float32).reshape(16)
    W, V = np.zeros(4, np.float32), np.zeros((4, 4), np.float32)
    assert lib().sim3_solver_model_jacobi(_p(A), _p(W), _p(V)) == 0
    return W, V


def compute(x3dc1, x3dc2, sets_, variant: int = 0) -> dict:
    """computeT for (n_hyp, 3) index sets: T12 / T21 (n_hyp, 3, 4), sim3 (n_hyp, 13), quat (n_hyp, 4)."""
    x1, x2 = _f32(x3dc1, 3), _f32(x3dc2, 3)
    s = np.ascontiguousarray(sets_, np.int32).reshape(-1, 3)
    m = max(len(s), 1)
    T12, T21 = np.zeros((m, 3, 4), np.float32), np.zeros((m, 3, 4), np.float32)
    sim3, quat = np.zeros((m, 13), np.float32), np.zeros((m, 4), np.float32)
    r = lib().sim3_solver_model_compute(len(x1), _p(x1), _p(x2), len(s), _p(s), int(variant), _p(T12), _p(T21),
                                        _p(sim3), _p(quat))
    assert r == 0, "a set index is out of range"
    return {"T12": T12[:len(s)], "T21": T21[:len(s)], "sim3": sim3[:len(s)], "quat": quat[:len(s)], "sets": s}


def iterate(x3dc1, x3dc2, sigma2_1, sigma2_2, K1, K2, rand31, min_inliers, best_in=0, variant=0, errors=False,
            sets_=None) -> dict:
    """n_hyp iterations of Sim3Solver::iterate without the early return, in the shape of
    Sim3Ransac.iterate.  N < min_inliers: nothing is generated (rows of zeros, counts 0)."""
    x1 = _f32(x3dc1, 3)
    n = len(x1)
    n_hyp = len(np.asarray(rand31 if sets_ is None else sets_).reshape(-1, 3))
    if n < min_inliers:
        z = np.zeros
        T = z((n_hyp, 3, 4), np.float32)
        out = solvers_model.sim3(x3dc1, x3dc2, sigma2_1, sigma2_2, K1, K2, T, T, min_inliers, best_in, 0, errors)
        out.update(T12=T, T21=T.copy(), sim3=z((n_hyp, 13), np.float32), quat=z((n_hyp, 4), np.float32),
                   sets=z((n_hyp, 3), np.int32))
    else:
        s = sets(n, rand31, variant) if sets_ is None else np.asarray(sets_, np.int32).reshape(-1, 3)
        hyp = compute(x3dc1, x3dc2, s, variant)
        out = solvers_model.sim3(x3dc1, x3dc2, sigma2_1, sigma2_2, K1, K2, hyp["T12"], hyp["T21"], min_inliers, best_in,
                                 0, errors)
        out.update(hyp)
    h = out["first_accept"] if out["first_accept"] >= 0 else int(out["best_at"][-1])
    out["accepted"] = out["sim3"][h].copy() if h >= 0 else np.full(13, np.nan, np.float32)
    return out


class Solver:
    """Sim3Solver's iterate / find with their state (Sim3Solver.cc:114-213) over the model: rand31 is
    the stream of rand() values, three per iteration, consumed as the reference consumes them."""

    def __init__(self, x3dc1, x3dc2, sigma2_1, sigma2_2, K1, K2, index1, N1, rand31, probability=0.99, min_inliers=6,
                 max_iterations=300):
        import orbslam_jpminipc_amd as orb

        self.a = (x3dc1, x3dc2, sigma2_1, sigma2_2, K1, K2)
        self.N = len(_f32(x3dc1, 3))
        self.index1, self.N1 = np.asarray(index1), int(N1)
        self.rand31 = np.asarray(rand31, np.int64).reshape(-1, 3)
        self.used = 0
        self.min_inliers = int(min_inliers)
        self.max_its = orb.sim3_ransac_parameters(self.N, probability, min_inliers, max_iterations)["max_iterations"]
        self.iterations, self.best_inliers, self.best = 0, 0, None

    def iterate(self, n_iterations):
        """-> (sim3 of 13 floats or None, bNoMore, vbInliers (N1,), nInliers)"""
        vb = np.zeros(self.N1, bool)
        if self.N < self.min_inliers:
            return None, True, vb, 0
        run = min(n_iterations, self.max_its - self.iterations)
        if run > 0:
            r = self.rand31[self.used:self.used + run]
            m = iterate(*self.a, r, self.min_inliers, self.best_inliers)
            first = m["first_accept"]
            last = first if first >= 0 else run - 1
            self.iterations += last + 1
            self.used += last + 1
            if m["best_at"][last] >= 0:
                b = int(m["best_at"][last])
                self.best_inliers, self.best = int(m["counts"][b]), m["sim3"][b].copy()
            if first >= 0:
                vb[self.index1[m["inliers"][first]]] = True
                return self.best, False, vb, int(m["counts"][first])
        return None, self.iterations >= self.max_its, vb, 0


# ---- synthetic cases ---------------------------------------------------------------------------------
def cloud(n=200, seed=1, scale=1.7, angle=0.4, noise=0.01, outliers=0.0):
    """n points at depth 2-10 seen from two frames related by a similarity (X1 = s R X2 + t), noise
    on both sides, optionally gross outliers; octave sigma2 per point."""
    rng = np.random.default_rng(seed)
    ax = rng.normal(0, 1, 3)
    R = solvers_model.rodrigues(angle * ax / np.linalg.norm(ax))
    t = rng.normal(0, 0.5, 3)
    X2 = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2, 10, n)], 1)
    X1 = scale * X2 @ R.T + t + rng.normal(0, noise, (n, 3))
    X2 = X2 + rng.normal(0, noise, (n, 3))
    bad = rng.random(n) < outliers
    X1[bad] += rng.normal(0, 0.8, (int(bad.sum()), 3))
    l1, l2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
    return {"x3dc1": X1.astype(np.float32), "x3dc2": X2.astype(np.float32),
            "sigma2_1": solvers_model.LEVEL_SIGMA2[l1].astype(np.float32),
            "sigma2_2": solvers_model.LEVEL_SIGMA2[l2].astype(np.float32), "R": R, "t": t, "s": scale}


def horn_f64(P1, P2):
    """Horn's closed form on two (3, k) float64 arrays with numpy's eigh, the formulas of computeT:
    (R, t, s, relative gap of the two largest eigenvalues)."""
    P1, P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
    O1, O2 = P1.mean(1, keepdims=True), P2.mean(1, keepdims=True)
    Pr1, Pr2 = P1 - O1, P2 - O2
    M = Pr2 @ Pr1.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    w, v = np.linalg.eigh(N)
    q = v[:, 3]
    gap = (w[3] - w[2]) / abs(w[3]) if w[3] != 0 else 0.0
    nv = np.linalg.norm(q[1:])
    ang = np.arctan2(nv, q[0])
    R = solvers_model.rodrigues(2 * ang * q[1:] / nv) if nv > 0 else np.eye(3)
    P3 = R @ Pr2
    s = float((Pr1 * P3).sum() / (P3 * P3).sum())
    t = (O1 - s * R @ O2).reshape(3)
    return R, t, s, gap
