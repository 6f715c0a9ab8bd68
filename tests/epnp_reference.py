"""EPnP in numpy float64, written from the construction (Lepetit, Moreno-Noguer, Fua: four control
points, barycentric coordinates, the null space of M, the distance constraints between the control
points, Gauss-Newton on the betas, absolute orientation), stage by stage, for csrc/orb_epnp_math.h to
be held against (tests/test_epnp_stages.py, tests/test_gpu_epnp_reference.py).

It shares no statement with the header: np.linalg.eigh / svd / lstsq / inv / det, no fused
multiply-add, no Jacobi rotation, no index table (the order of the ten products beta_i*beta_j and of
the six control-point pairs is built from the pairs themselves).

With four correspondences M is 8 x 12 and its null space has four exact dimensions: any orthonormal
basis of it is as good as another and LAPACK's differs from Jacobi's.  So the decomposition is checked
by its properties (mtm_svd_errors) and everything downstream takes a basis as an argument: the stage
functions are fed the header's exported one, and `chain` runs from the basis and the alphas to the
three poses with nothing else of the header's."""
import numpy as np

# the six pairs of control points, and the ten products beta_i*beta_j in the order that puts every
# product of the first k betas before any that involves beta_k (the 3, 5 and 10 first columns are the
# products of 2, 3 and 4 betas)
PAIRS = [(a, b) for a in range(4) for b in range(a + 1, 4)]
PRODUCTS = [(i, j) for j in range(4) for i in range(j + 1)]
COLUMN = {p: c for c, p in enumerate(PRODUCTS)}


def products(betas):
    b = np.asarray(betas, np.float64)
    return np.array([b[i] * b[j] for i, j in PRODUCTS])


# ---- control points and barycentric coordinates ---------------------------------------------------------
def control_point_frame(pw):
    """The centroid, the eigenvalues of PW0^T PW0 in descending order and their eigenvectors (rows)."""
    pw = np.asarray(pw, np.float64)
    c0 = pw.mean(0)
    lam, vec = np.linalg.eigh((pw - c0).T @ (pw - c0))
    return c0, lam[::-1], vec[:, ::-1].T


def control_point_errors(cws, pw, floor=1e-12):
    """(centroid, radius, direction) differences of exported control points: cws[0] is the centroid,
    |cws[i] - cws[0]| = sqrt(lambda_i / n), and the direction is the eigenvector up to sign.  An offset
    whose eigenvalue is under `floor` times the largest is skipped (also returned: how many): its
    direction is that of rounding noise and its length the square root of it."""
    n = len(pw)
    c0, lam, vec = control_point_frame(pw)
    d = np.asarray(cws)[1:] - np.asarray(cws)[0]
    e_c = np.abs(cws[0] - c0).max()
    e_r, e_d, skipped = 0.0, 0.0, 0
    for i in range(3):
        if not lam[i] >= floor * lam[0] or lam[0] <= 0:
            skipped += 1
            continue
        e_r = max(e_r, abs(np.linalg.norm(d[i]) - np.sqrt(lam[i] / n)))
        u = d[i] / np.linalg.norm(d[i])
        e_d = max(e_d, min(np.abs(u - vec[i]).max(), np.abs(u + vec[i]).max()))
    return e_c, e_r, e_d, skipped


def rho_of(pw):
    """The six squared distances between the control points, from the eigenvalues alone: the three
    offsets are orthogonal, of squared length lambda_i / n."""
    _, lam, _ = control_point_frame(pw)
    r2 = np.concatenate([[0.0], np.maximum(lam, 0) / len(pw)])
    return np.array([r2[a] + r2[b] for a, b in PAIRS])


def alpha_errors(alphas, cws, pw, ci, cond_cap=1e8):
    """(rows sum to 1, alphas @ cws gives back the points, ci against inv(CC) or None when CC's
    condition number is above the cap)."""
    alphas, cws, pw = np.asarray(alphas), np.asarray(cws), np.asarray(pw, np.float64)
    e_sum = np.abs(alphas.sum(1) - 1).max()
    e_pw = np.abs(alphas @ cws - pw).max()
    CC = (cws[1:] - cws[0]).T
    e_ci = None
    if np.isfinite(CC).all() and np.linalg.cond(CC) < cond_cap:
        e_ci = np.abs(np.asarray(ci) - np.linalg.inv(CC)).max()
    return e_sum, e_pw, e_ci


# ---- M and its decomposition ------------------------------------------------------------------------------
def build_m(alphas, us, K):
    """M (2n x 12): the two projection equations of every correspondence in the twelve coordinates of
    the camera-frame control points."""
    fu, fv, uc, vc = K
    alphas, us = np.asarray(alphas), np.asarray(us, np.float64)
    M = np.zeros((2 * len(alphas), 12))
    for j in range(4):
        M[0::2, 3 * j] = alphas[:, j] * fu
        M[0::2, 3 * j + 2] = alphas[:, j] * (uc - us[:, 0])
        M[1::2, 3 * j + 1] = alphas[:, j] * fv
        M[1::2, 3 * j + 2] = alphas[:, j] * (vc - us[:, 1])
    return M


def mtm_svd_errors(ut, w, M):
    """(orthonormality of ut, ut^T diag(w) ut against M^T M, w against the squared singular values of M
    in descending order), the last two relative to w[0]."""
    ut, w = np.asarray(ut), np.asarray(w)
    sv = np.linalg.svd(M, compute_uv=False) ** 2
    sv = np.concatenate([sv, np.zeros(12 - len(sv))])[:12]
    e_orth = np.abs(ut @ ut.T - np.eye(12)).max()
    e_rec = np.abs(ut.T @ np.diag(w) @ ut - M.T @ M).max() / w[0]
    e_w = np.abs(w - sv).max() / w[0]
    return e_orth, e_rec, e_w


def basis_of(ut):
    """The four vectors the betas multiply, as 4 x (4 control points x 3): the last row of ut first."""
    return np.asarray(ut)[[11, 10, 9, 8]].reshape(4, 4, 3)


# ---- the distance constraints -----------------------------------------------------------------------------
def l_of(V):
    """L (6 x 10) from the basis: row (a, b) is the quadratic form beta -> |sum_k beta_k (v_k[a] -
    v_k[b])|^2 written in the products: Q = D D^T, an off-diagonal product collects Q_ij + Q_ji."""
    L = np.zeros((6, 10))
    for r, (a, b) in enumerate(PAIRS):
        D = V[:, a] - V[:, b]
        Q = D @ D.T
        for (i, j), c in COLUMN.items():
            L[r, c] = Q[i, i] if i == j else Q[i, j] + Q[j, i]
    return L


def l_definition_error(l_6x10, V, rng, tries=8):
    """L by its definition: for random betas, L . products is the six squared distances between the
    control points of sum_k beta_k v_k.  Relative to the largest distance."""
    worst = 0.0
    for _ in range(tries):
        beta = rng.normal(size=4)
        C = np.tensordot(beta, V, 1)
        d2 = np.array([np.sum((C[a] - C[b]) ** 2) for a, b in PAIRS])
        worst = max(worst, np.abs(np.asarray(l_6x10) @ products(beta) - d2).max() / d2.max())
    return worst


def rho_error(rho, cws):
    cws = np.asarray(cws)
    return np.abs(np.asarray(rho) - np.array([np.sum((cws[a] - cws[b]) ** 2) for a, b in PAIRS])).max()


# ---- the three approximations ---------------------------------------------------------------------------
def approx_columns(N):
    """N = 1: the products with beta_0 (the others taken as small); N = 2: the three products of the
    first two betas; N = 3: those of the first three without beta_2^2 (EPnP solves five unknowns from
    the six equations, not six)."""
    if N == 1:
        return [COLUMN[(0, j)] for j in range(4)]
    return [c for c, p in enumerate(PRODUCTS) if p[1] <= N - 1 and p != (2, 2)]


def approx_solve(L, rho, N):
    """The least-squares products of approximation N: (x by product, condition number of the
    sub-matrix, how many singular values the back-substitution's cut (2 eps sum(s)) drops)."""
    cols = approx_columns(N)
    A = np.asarray(L)[:, cols]
    U, s, Vt = np.linalg.svd(A, full_matrices=False)
    keep = s > 2 * np.finfo(np.float64).eps * s.sum()
    cond = s[0] / s[-1] if s[-1] > 0 else np.inf
    if keep.all():
        x = np.linalg.lstsq(A, np.asarray(rho), rcond=None)[0]
    else:  # the pseudo-inverse cut at the same threshold
        x = Vt[keep].T @ ((U[:, keep].T @ np.asarray(rho)) / s[keep])
    return {PRODUCTS[c]: x[k] for k, c in enumerate(cols)}, cond, int((~keep).sum())


def approx_betas(L, rho, N):
    """Betas from the products: beta_0^2 fixes the overall sign of the solution; N = 1 divides the
    mixed products by beta_0; N = 2, 3 take beta_1 from beta_1^2 (0 when its sign disagrees), the sign
    of beta_0 from beta_0*beta_1, and N = 3 beta_2 from beta_0*beta_2.  For N = 2, 3 the mixed products
    are read as solved, not re-signed with beta_0^2: that is EPnP's rule as published."""
    x, cond, dropped = approx_solve(L, rho, N)
    sgn = -1.0 if x[(0, 0)] < 0 else 1.0
    b = np.zeros(4)
    b[0] = np.sqrt(sgn * x[(0, 0)])
    if N == 1:
        for j in (1, 2, 3):
            b[j] = sgn * x[(0, j)] / b[0]
    else:
        b[1] = np.sqrt(sgn * x[(1, 1)]) if sgn * x[(1, 1)] > 0 else 0.0
        if x[(0, 1)] < 0:
            b[0] = -b[0]
        if N == 3:
            b[2] = x[(0, 2)] / b[0]
    return b, cond, dropped


# ---- Gauss-Newton -------------------------------------------------------------------------------------------
def gn_jacobian(L, betas):
    """d(L . products)/d beta_k: the product (i, j) contributes beta_j to column i and beta_i to column j."""
    J = np.zeros((6, 4))
    for (i, j), c in COLUMN.items():
        J[:, i] += L[:, c] * betas[j]
        J[:, j] += L[:, c] * betas[i]
    return J


def gauss_newton(L, rho, betas, steps=5):
    """(betas after `steps` steps, the largest condition number of a Jacobian on the way)."""
    L, b, cond = np.asarray(L), np.array(betas, np.float64), 0.0
    for _ in range(steps):
        J = gn_jacobian(L, b)
        if not np.isfinite(J).all():  # nothing to solve: the betas were not numbers to begin with
            return np.full(4, np.nan), np.inf
        cond = max(cond, np.linalg.cond(J))
        b = b + np.linalg.lstsq(J, np.asarray(rho) - L @ products(b), rcond=None)[0]
    return b, cond


# ---- the pose of a set of betas -----------------------------------------------------------------------------
def pose_of(betas, V, alphas, pw, us, K):
    """Camera-frame control points and points, the sign from the first point's depth, absolute
    orientation by SVD (the third row negated when the determinant is negative), t, and the mean pixel
    distance.  Returns a dict with R, t, rep_error, sign_flip, det_neg, gap (the smallest singular
    value of the cross-covariance over the largest: the rotation is determined only while it is not 0)."""
    fu, fv, uc, vc = K
    pw, us = np.asarray(pw, np.float64), np.asarray(us, np.float64)
    ccs = np.tensordot(np.asarray(betas), V, 1)
    pcs = np.asarray(alphas) @ ccs
    flip = bool(pcs[0, 2] < 0)
    if flip:
        pcs = -pcs
    pc0, pw0 = pcs.mean(0), pw.mean(0)
    if not np.isfinite(pcs).all():
        return {"R": np.full((3, 3), np.nan), "t": np.full(3, np.nan), "rep_error": np.nan, "sign_flip": flip,
                "det_neg": False, "gap": 0.0}
    U, s, Vt = np.linalg.svd((pcs - pc0).T @ (pw - pw0))
    R = U @ Vt
    det_neg = bool(np.linalg.det(R) < 0)
    if det_neg:
        R[2] = -R[2]
    t = pc0 - R @ pw0
    pc = pw @ R.T + t
    proj = np.stack([uc + fu * pc[:, 0] / pc[:, 2], vc + fv * pc[:, 1] / pc[:, 2]], 1)
    return {"R": R, "t": t, "rep_error": np.linalg.norm(us - proj, axis=1).mean(), "sign_flip": flip,
            "det_neg": det_neg, "gap": s[1] / s[0] if s[0] > 0 else 0.0}


def chain(ut, alphas, pw, us, K):
    """From the basis and the alphas to the three poses, nothing else taken from the header: rho from
    the eigenvalues, L from the basis, the three approximations, Gauss-Newton, the poses.  Returns a
    list of three dicts (pose_of's, plus betas0, betas, cond: the largest condition number met)."""
    V = basis_of(ut)
    L, rho = l_of(V), rho_of(pw)
    out = []
    for N in (1, 2, 3):
        b0, cond, dropped = approx_betas(L, rho, N)
        b, cond_j = gauss_newton(L, rho, b0)
        o = pose_of(b, V, alphas, pw, us, K)
        o.update(betas0=b0, betas=b, cond=max(cond, cond_j), dropped=dropped, products=approx_solve(L, rho, N)[0])
        out.append(o)
    return out


def candidates(errors, margin):
    """The N (1-based) whose error is within `margin` (relative) of the smallest."""
    e = np.asarray(errors)
    return [k + 1 for k in range(len(e)) if e[k] <= e.min() * (1 + margin)]


def strict_choice(errors):
    """N = 1 unless the second error is strictly smaller; then the third against the holder's."""
    N = 1
    if errors[1] < errors[0]:
        N = 2
    if errors[2] < errors[N - 1]:
        N = 3
    return N


# ---- the Jacobi SVD on its own ----------------------------------------------------------------------------
def svd_errors(A, Ut, W, Vt):
    """A (m x n) = Ut[:n]^T diag(W) Vt: (reconstruction relative to the largest singular value, rows of
    Ut[:rank] and of Vt orthonormal, W against np.linalg.svd relative likewise, W descending)."""
    A = np.asarray(A, np.float64)
    n = A.shape[1]
    s = np.linalg.svd(A, compute_uv=False)
    scale = s[0] if s[0] > 0 else 1.0
    e_rec = np.abs(Ut[:n].T @ np.diag(W) @ Vt - A).max() / scale
    e_orth = max(np.abs(Ut @ Ut.T - np.eye(len(Ut))).max(), np.abs(Vt @ Vt.T - np.eye(n)).max())
    e_w = np.abs(W - s).max() / scale
    return e_rec, e_orth, e_w, bool((np.diff(W) <= 0).all())
