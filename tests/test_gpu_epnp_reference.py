"""The PnP kernels held to the numpy float64 EPnP of tests/epnp_reference.py, at the
smallest shapes where the device build differs from the host build of csrc/orb_epnp_math.h: one lane
per hypothesis with the work matrix at stride 64 in LDS and alphas and pcs recomputed (`Pts4`), one
past a wave; `k_pnp_refine`'s `Mat<1>` + `PtsList` instantiation; the batch form.

Each result is first required to equal the model's bits (tests/native/pnp_solver_model.cpp), as in
test_gpu_pnp_solver.py: that equality, with the model's stage checks (test_epnp_stages.py), carries the
intermediates, which the kernels do not export.  Then R, t and the reprojection error are compared
with the all-numpy chain on the same correspondences: from the model's exported null-space basis and
alphas (with four points any basis of the null space is valid, so the reference cannot choose its
own) to the three poses.  They must equal those of one candidate N, the candidates being the N whose
reference error is within the tie margin of the smallest.  Bounds and tie margin are the CPU test's
(test_epnp_stages.BOUNDS: the chain's R 3.527e-09, t 3.728e-08, error 5.742e-06 relative, 10 x the
measured 3.527e-10, 3.728e-09, 5.742e-07): the kernel's bits are the model's."""
import numpy as np
import pytest

import epnp_reference as ref
import epnp_stage_checks as sc
import orbslam_jpminipc_amd as orb
from orbslam_jpminipc_amd import _native
import pnp_solver_model as pm
import solvers_model as model
from test_epnp_stages import BOUNDS, TIE_MARGIN
from test_gpu_pnp_solver import same

pytestmark = pytest.mark.gpu

f32 = np.float32
K32 = f32(pm.K_CAM)
K64 = np.float64(K32)
TH2 = f32(5.991)
LS2 = model.LEVEL_SIGMA2


def distinct_sets(n, n_hyp, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.sort(rng.choice(n, 4, replace=False)) for _ in range(n_hyp)]).astype(np.int32)


def hold_to_chain(R, t, rep, p3, p2, sel, what, extra=0.0):
    """R, t (and rep when given) equal the chain's for one candidate N on the correspondences `sel`;
    `extra` is a rounding the caller's values went through, relative.  Returns the candidates."""
    sel = np.asarray(sel)
    h = pm.stages(p3, p2, K64, sel)
    ch = ref.chain(h["ut"], h["alphas"], np.float64(p3)[sel], np.float64(p2)[sel], K64)
    cand = ref.candidates([c["rep_error"] for c in ch], TIE_MARGIN)
    assert all(sc.chain_comparable(ch[N - 1]) for N in cand), f"{what}: outside the chain's conditions"
    fits = []
    for N in cand:
        c = ch[N - 1]
        ok = (np.abs(R - c["R"]) <= BOUNDS["chain_R"] + extra * np.abs(c["R"])).all() and \
             (np.abs(t - c["t"]) <= BOUNDS["chain_t"] + extra * np.abs(c["t"])).all()
        if rep is not None:
            ok = ok and sc.rel(rep, c["rep_error"]) <= BOUNDS["chain_rep"]
        fits.append(ok)
    assert any(fits), (f"{what}: candidates {cand}, R off by {[np.abs(R - ch[N - 1]['R']).max() for N in cand]}, "
                       f"t by {[np.abs(t - ch[N - 1]['t']).max() for N in cand]}")
    return cand


@pytest.mark.parametrize("noise", [0.0, 1.0])
def test_hypotheses_equal_the_chain(noise):
    n, n_hyp = 30, 65
    p3, p2, _, _ = pm.scene(n, 3, noise=noise)
    sets = distinct_sets(n, n_hyp, 103)
    got = orb.PnPRansac(*K32, min_inliers=4).compute_hypotheses(p3, p2, sets=sets)
    want = pm.ransac(p3, p2, np.ones(n, f32), TH2, K64, 4, sets=sets)
    same(got["R"].reshape(-1, 9), want["R"], "R")
    same(got["t"], want["t"], "t")
    same(got["rep_error"], want["rep_error"], "rep_error")
    single = {1: 0, 2: 0, 3: 0}
    for h in range(n_hyp):
        cand = hold_to_chain(got["R"][h].reshape(3, 3), got["t"][h], got["rep_error"][h], p3, p2, sets[h],
                             f"hypothesis {h}")
        if len(cand) == 1:
            single[cand[0]] += 1
    assert min(single.values()) >= 10, single


@pytest.mark.parametrize("n", [5, 6, 45])
def test_n_point_pose_equals_the_chain(n):
    p3, p2, _, _ = pm.scene(n + 7, 200 + n, noise=1.0)
    sel = np.sort(np.random.default_rng(n).permutation(len(p3))[:n]).astype(np.int32)
    got = orb.PnPRansac(*K32, min_inliers=4).compute_pose(p3, p2, sel)
    want = pm.compute_pose(p3, p2, K64, sel)
    same(got["R"], want["R"], "R")
    same(got["t"], want["t"], "t")
    same(np.float64([got["rep_error"]]), np.float64([want["rep_error"]]), "rep_error")
    hold_to_chain(got["R"], got["t"], got["rep_error"], p3, p2, sel, f"n = {n}")


def batch_inputs(ns, cap, seed):
    """A keyframe (0) and a frame (1): frame keypoint j sees the keyframe's MapPoint perm[j] (one in
    four grossly off); solver s keeps ns[s] of those matches.  Host arrays."""
    rng = np.random.default_rng(seed)
    p3, p2, _, _ = pm.scene(cap, seed, noise=1.0, outliers=0.25)
    perm = rng.permutation(cap)
    pos = np.zeros((2, cap, 3), f32)
    pos[0, perm] = p3
    kps = np.zeros((2, cap), _native.KEYPOINT_DTYPE)
    kps["x"][1], kps["y"][1] = p2[:, 0], p2[:, 1]
    kps["octave"][1] = rng.integers(0, 3, cap)
    rows = np.full((len(ns), cap), -1, np.int32)
    for s, k in enumerate(ns):
        j = np.sort(rng.choice(cap, k, replace=False))
        rows[s, j] = perm[j]
    return kps, pos, rows


def test_batch_refined_pose_equals_the_chain():
    import torch

    S, cap, n_hyp, mi = 3, 64, 70, 10
    kps, pos, rows = batch_inputs([40, 64, 30], cap, 303)
    r = np.random.default_rng(S).integers(0, 2 ** 31, (S, n_hyp, 4)).astype(np.int32)
    tc = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    rs = orb.PnPRansac(*K32, min_inliers=mi, th2=TH2)
    out = rs.iterate_batch_device(tc(kps.view(np.uint8).reshape(2, cap, -1)), tc(np.int32([cap, cap])),
                                  tc(np.zeros(S, np.int32)), tc(np.ones(S, np.int32)), tc(rows), tc(pos), None, LS2, tc(r))
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for s in range(S):
        su = model.pnp_setup(kps[1], cap, cap, rows[s], pos[0], None, LS2)
        m = pm.ransac(su["p3d"], su["p2d"], su["sigma2"], TH2, K64, mi, rand31=r[s])
        fr = int(out["first_refined"][s])
        assert fr >= 0 and fr == m["first_refined"], f"solver {s}: no refined pose"
        same(out["pose"][s], m["pose"], f"pose of solver {s}")
        # Refine ran compute_pose on the best mask of that iteration, in index order
        mask = out["masks"][s].view(np.uint64).reshape(n_hyp, -1)[fr]
        assert np.array_equal(mask[:m["masks"].shape[1]], m["masks"][fr]), f"best mask of solver {s}"
        sel = np.flatnonzero(model.unpack(mask, su["n"])).astype(np.int32)
        assert len(sel) >= mi
        pose = np.float64(out["pose"][s])
        # the pose is the double result narrowed to float: half a unit in the last place, 2^-24 relative
        hold_to_chain(pose[:9].reshape(3, 3), pose[9:], None, su["p3d"], su["p2d"], sel, f"solver {s}", extra=2.0 ** -24)
