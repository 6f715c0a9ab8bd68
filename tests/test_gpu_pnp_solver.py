"""GPU parity of the PnPsolver hypotheses, Refine and the whole RANSAC (csrc/orb_solvers.hip:
orb_pnp_compute_hypotheses, orb_pnp_compute_pose_n, orb_pnp_ransac, orb_pnp_ransac_batch_device)
against the CPU model (tests/native/pnp_solver_model.cpp).

Every array is compared bit for bit; where the model has a NaN the kernel must have one too (a NaN's
own bits are the processor's and are not compared)."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import orbslam_jpminipc_amd as orb
from orbslam_jpminipc_amd import _native
import pnp_solver_model as pm
import solvers_model as model

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
f32 = np.float32
K32 = f32(pm.K_CAM)
K64 = np.float64(K32)
TH2 = f32(5.991)
LS2 = model.LEVEL_SIGMA2


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(ROOT / "tests" / "golden" / "pnp_solver_320x240.npz"))


def same(got, want, what):
    """NaN positions equal, every other value equal bit for bit."""
    got, want = np.asarray(got), np.asarray(want).reshape(np.shape(got))
    assert got.dtype == want.dtype, what
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
        got, want = got.copy(), want.copy()
        got[nan] = 0
        want[nan] = 0
    bad = np.flatnonzero((got.view(np.uint8) != want.view(np.uint8)).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at byte {bad[0]}"


def ransac_of(n, seed, noise=1.2, outliers=0.35):
    p3, p2, _, _ = pm.scene(n, seed, noise=noise, outliers=outliers)
    return p3, p2, np.ones(n, f32)


def check_ransac(it, want, what=""):
    for k in ("counts", "masks", "best_at", "sets", "refined_counts", "pose_mask"):
        same(it[k], want[k], f"{what}{k}")
    for k in ("R", "t", "pose"):
        same(it[k].reshape(want[k].shape), want[k], f"{what}{k}")
    for k in ("first_ok", "first_refined", "pose_inliers"):
        assert it[k] == want[k], f"{what}{k}: {it[k]} != {want[k]}"


# ---- compute_pose on minimal sets --------------------------------------------------------------------
@pytest.mark.parametrize("n_hyp", [1, 64, 65, 300])
def test_compute_hypotheses(n_hyp, golden):
    rs = orb.PnPRansac(*K32, min_inliers=4)
    for N in (4, 5, len(golden["p3d"])):
        if N == len(golden["p3d"]):
            p3, p2 = golden["p3d"], golden["p2d"]
        else:
            p3, p2, _ = ransac_of(N, 40 + N, noise=0.8, outliers=0.0)
        r = pm.draws(n_hyp, 7 * n_hyp + N)
        r[0] = 0
        r[-1] = 2 ** 31 - 1
        want = pm.ransac(p3, p2, np.ones(N, f32), TH2, K64, 4, rand31=r)
        assert np.array_equal(want["sets"], pm.sets(N, r)) and np.array_equal(want["sets"], orb.pnp_minimal_sets(N, r))
        if N == 4:  # every set the same four points, in the orders the sampler leaves
            assert all(sorted(s) == [0, 1, 2, 3] or len(set(s)) < 4 for s in want["sets"].tolist())
        for kw in ({"rand31": r}, {"sets": want["sets"]}):
            got = rs.compute_hypotheses(p3, p2, **kw)
            same(got["sets"], want["sets"], f"sets N={N}")
            same(got["R"].reshape(-1, 9), want["R"], f"R N={N} {list(kw)}")
            same(got["t"], want["t"], f"t N={N}")
            same(got["rep_error"], want["rep_error"], f"rep_error N={N}")


def degenerate_cases():
    p3, p2, R, t = pm.scene(12, 7)
    proj = lambda P: np.stack([K64[2] + K64[0] * P[:, 0] / P[:, 2], K64[3] + K64[1] * P[:, 1] / P[:, 2]], 1)  # noqa: E731
    cop = p3.copy()
    cop[:4, 2] = 0.5
    beh = p3.copy()
    beh[0] = (-R.T @ t + R.T @ np.array([0.1, 0.1, -2.0])).astype(f32)
    nan = p3.copy()
    nan[1, 1] = np.nan
    noisy3, noisy2, _, _ = pm.scene(30, 11, noise=2.0, outliers=0.3)
    gen = pm.sets(30, pm.draws(64, 3))
    return {"coplanar": (cop, proj(cop.astype(np.float64) @ R.T + t).astype(f32), [[0, 1, 2, 3]]),
            "repeated": (p3, p2, [[0, 1, 1, 2], [0, 0, 1, 1]]),  # (two pairs: the one input seen to make the SVD's sort swap)
            "identical": (p3, p2, [[3, 3, 3, 3]]),
            "behind": (beh, p2, [[0, 1, 2, 3]]),
            "nan": (nan, p2, [[0, 1, 2, 3]]),
            "general": (noisy3, noisy2, gen)}


def test_degenerate_sets_reach_every_branch():
    rs = orb.PnPRansac(*K32, min_inliers=4)
    seen, by_case = 0, {}
    for name, (p3, p2, sets) in degenerate_cases().items():
        sets = np.int32(sets)
        want = pm.ransac(p3, p2, np.ones(len(p3), f32), TH2, K64, 4, sets=sets)
        got = rs.compute_hypotheses(p3, p2, sets=sets)
        same(got["R"].reshape(-1, 9), want["R"], f"R of {name}")
        same(got["t"], want["t"], f"t of {name}")
        same(got["rep_error"], want["rep_error"], f"rep_error of {name}")
        by_case[name] = int(np.bitwise_or.reduce(want["branches"]))
        seen |= by_case[name]
    B = pm.BR
    assert by_case["coplanar"] & B["SVD_FILL"] and by_case["coplanar"] & B["BKSB_SKIP"]
    assert by_case["repeated"] & B["BKSB_SKIP"] and by_case["repeated"] & B["SVD_SWAP"]
    assert by_case["identical"] & B["QR_ETA0"]
    assert by_case["behind"] & B["SIGN_FLIP"]
    assert by_case["general"] & B["DET_NEG"] and by_case["general"] & B["B_NEG"] and by_case["general"] & B["B_POS"]
    assert np.isnan(pm.ransac(*degenerate_cases()["nan"][:2], np.ones(12, f32), TH2, K64, 4,
                              sets=np.int32([[0, 1, 2, 3]]))["R"]).all()
    missing = [n for n in pm.BRANCHES if not seen & B[n]]
    assert not missing, f"branches no case reached: {missing}"


# ---- Refine's n-point pose ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 65, 8192])
def test_n_point_pose(n):
    rs = orb.PnPRansac(*K32, min_inliers=4)
    p3, p2, _ = ransac_of(max(n, 8) + 3 if n < 8192 else n, 90 + n % 97, noise=0.7, outliers=0.0)
    sel = np.random.default_rng(n).permutation(len(p3))[:n].astype(np.int32)
    sel.sort()
    want = pm.compute_pose(p3, p2, K64, sel)
    got = rs.compute_pose(p3, p2, sel)
    same(got["R"], want["R"], "R")
    same(got["t"], want["t"], "t")
    same(np.float64([got["rep_error"]]), np.float64([want["rep_error"]]), "rep_error")
    assert np.isfinite(want["R"]).all() and want["rep_error"] < 5


# ---- the whole iterate ---------------------------------------------------------------------------------
def test_ransac_equals_model_and_check_inliers_on_its_own_poses(golden):
    g = golden
    rs = orb.PnPRansac(*g["K"], min_inliers=int(g["min_inliers"]), th2=float(g["th2"]))
    it = rs.iterate(g["p3d"], g["p2d"], g["sigma2"], rand31=g["rand31"])
    want = {k: g[k] for k in ("counts", "masks", "best_at", "sets", "refined_counts", "pose_mask", "R", "t", "pose")}
    want.update({k: int(g[k]) for k in ("first_ok", "first_refined", "pose_inliers")})
    check_ransac(it, want)
    # the fixture is the model's answer today too
    m = pm.ransac(g["p3d"], g["p2d"], g["sigma2"], g["th2"], np.float64(g["K"]), int(g["min_inliers"]), rand31=g["rand31"])
    check_ransac(it, m, "model today: ")
    assert it["first_refined"] >= 0 and it["pose_inliers"] == it["refined_counts"][it["first_refined"]]
    ck = rs.check(g["p3d"], g["p2d"], g["sigma2"], it["R"], it["t"])
    for k in ("counts", "masks", "best_at"):
        same(it[k], ck[k], f"{k} against orb_pnp_check_inliers")
    assert it["first_ok"] == ck["first_ok"]
    # the refined pose scored on its own gives the returned mask and count
    h = it["first_refined"]
    sel = np.flatnonzero(it["inliers"][h]).astype(np.int32)
    rp = rs.compute_pose(g["p3d"], g["p2d"], sel)
    same(f32(np.concatenate([rp["R"].reshape(9), rp["t"]])), it["pose"], "pose against orb_pnp_compute_pose_n")
    ck = rs.check(g["p3d"], g["p2d"], g["sigma2"], rp["R"].reshape(1, 9), rp["t"].reshape(1, 3))
    same(ck["masks"][0], it["pose_mask"], "pose_mask")
    assert int(ck["counts"][0]) == it["pose_inliers"]


def iterate_against_model(n, n_hyp, seed, K=(260.0, 260.0, 160.0, 120.0)):
    """orb_pnp_ransac on n correspondences of a scene against the model, every output bit for bit."""
    p3, p2, s2 = ransac_of(max(n, 4), seed)
    p3, p2, s2 = p3[:n], p2[:n], s2[:n]
    r = np.random.default_rng(seed + n).integers(0, 2 ** 31, (n_hyp, 4)).astype(np.int32)
    it = orb.PnPRansac(*K, min_inliers=10, th2=float(TH2)).iterate(p3, p2, s2, rand31=r)
    check_ransac(it, pm.ransac(p3, p2, s2, TH2, np.float64(K), 10, rand31=r), f"n = {n}: ")
    return it


def test_staging_reuse_across_sizes():
    """One thread, one context: a small call, one large enough to grow the device arena and the pinned
    staging, a small one again and the empty input, each against the model: a layout that leans on
    what an earlier call left in the staging, or on where the arena was before it grew, fails.  Then
    the n-point pose, which shares the arena and lays it out with a selection list."""
    for n, n_hyp in [(65, 1), (130, 65), (1, 1), (0, 1)]:
        it = iterate_against_model(n, n_hyp, 5)
        assert it["masks"].shape == (n_hyp, (n + 63) // 64) and it["pose_mask"].shape == ((n + 63) // 64,)
    test_n_point_pose(65)


def test_three_entry_points_share_one_arena():
    """PnP RANSAC at the large size, then the initializer's RANSAC on a small pair, then OptimizeSim3, on
    one thread: each against its own model, so a layout that reads what another entry point left in
    the arena or the staging fails."""
    import sim3_optimization_model as s3m
    import test_gpu_initializer_ransac as tir
    import test_gpu_sim3_optimization as tso

    iterate_against_model(130, 65, 5)
    k1, k2, m12 = tir.two_view_case(40, 65, 50)
    tir.run_find(k1, k2, m12, tir.draws(1, 3))
    c = s3m.host_cases()["pairs_65"]
    tso.same_as_model(tso.run_host(orb.Optimizer(0), c), c["model"], "after two other entry points")


# (seed, min_inliers, the replacing iterations, their refined counts, first_refined) found with the model
REFINE_CASES = {"equal: Refine fails": (5, 20, [31], [20], -1),
                "one more: Refine succeeds": (5, 19, [31], [20], 31),
                "a later replacing iteration is the first to succeed": (78, 25, [1, 10], [25, 27], 10)}


@pytest.mark.parametrize("name", list(REFINE_CASES))
def test_refine_is_strict_and_the_loop_goes_on(name):
    seed, mi, rep, rc, first_refined = REFINE_CASES[name]
    p3, p2, s2 = ransac_of(40, seed)
    r = pm.draws(40, seed)
    want = pm.ransac(p3, p2, s2, TH2, K64, mi, rand31=r)
    assert [h for h in range(40) if want["best_at"][h] == h] == rep
    assert want["refined_counts"][rep].tolist() == rc and want["first_refined"] == first_refined
    it = orb.PnPRansac(*K32, min_inliers=mi, th2=TH2).iterate(p3, p2, s2, rand31=r)
    check_ransac(it, want)
    if first_refined < 0:  # the best pose and mask, not a refined one
        h = int(it["best_at"][-1])
        same(it["pose"], f32(np.concatenate([it["R"][h].reshape(9), it["t"][h]])), "mBestTcw")
        same(it["pose_mask"], it["masks"][h], "mvbBestInliers")
        assert it["pose_inliers"] == it["counts"][h]


def test_best_in_that_is_never_replaced_and_no_more():
    p3, p2, s2 = ransac_of(40, 5)
    r = pm.draws(40, 5)
    rs = orb.PnPRansac(*K32, min_inliers=10, th2=TH2)
    it = rs.iterate(p3, p2, s2, rand31=r, best_in=41)
    check_ransac(it, pm.ransac(p3, p2, s2, TH2, K64, 10, rand31=r, best_in=41))
    assert (it["best_at"] == -2).all() and it["first_refined"] == -1 and (it["refined_counts"] == -1).all()
    assert np.isnan(it["pose"]).all() and not it["pose_mask"].any() and it["pose_inliers"] == 41
    assert it["first_ok"] >= 0
    # N < min_inliers: bNoMore, nothing is generated
    it = rs.iterate(p3[:9], p2[:9], s2[:9], rand31=r)
    check_ransac(it, pm.ransac(p3[:9], p2[:9], s2[:9], TH2, K64, 10, rand31=r))
    assert not it["R"].any() and not it["t"].any() and not it["sets"].any() and not it["counts"].any()
    assert (it["best_at"] == -1).all() and it["first_ok"] == -1 and it["first_refined"] == -1
    assert np.isnan(it["pose"]).all() and it["pose_inliers"] == 0
    # no correspondences at all
    it = rs.iterate(p3[:0], p2[:0], s2[:0], rand31=r)
    assert not it["counts"].any() and it["first_refined"] == -1 and np.isnan(it["pose"]).all()


def test_null_outputs_and_refusals():
    lib, p = _native.hip_lib(), _native.ptr
    p3, p2, s2 = ransac_of(40, 5)
    r = pm.draws(6, 5)
    head = (40, p(p3), p(p2), p(s2), float(TH2), *K64, 6, None, p(r), 10, 0)
    _native.check(lib.orb_pnp_ransac(*head, *([None] * 12), 0))
    pose = np.zeros(12, f32)
    _native.check(lib.orb_pnp_ransac(*head, *([None] * 9), p(pose), None, None, 0))
    same(pose, orb.PnPRansac(*K32, min_inliers=10, th2=TH2).iterate(p3, p2, s2, rand31=r)["pose"], "pose alone")
    _native.check(lib.orb_pnp_compute_hypotheses(40, p(p3), p(p2), *K64, 6, None, p(r), None, None, None, None, 0))

    def code(fn):
        with pytest.raises(_native.OrbError) as e:
            fn()
        assert str(e.value).split(":", 1)[1].strip(), "a refusal carries a message"
        return e.value.code

    EINVAL, ENOTSUP = _native.ORB_EINVAL, _native.ORB_ENOTSUP
    rs = orb.PnPRansac(*K32, min_inliers=10, th2=TH2)
    assert code(lambda: orb.PnPRansac(*K32, min_inliers=3).iterate(p3, p2, s2, rand31=r)) == EINVAL
    ok = np.zeros((4, 4), np.int32)
    for bad in (-1, 40):
        s = ok.copy()
        s[2, 1] = bad
        assert code(lambda: rs.iterate(p3, p2, s2, sets=s)) == EINVAL
        assert code(lambda: rs.compute_hypotheses(p3, p2, sets=s)) == EINVAL
        assert code(lambda: rs.compute_pose(p3, p2, [0, 1, bad, 2])) == EINVAL
    rr = ok.copy()
    rr[3, 0] = -5
    assert code(lambda: rs.iterate(p3, p2, s2, rand31=rr)) == EINVAL
    assert code(lambda: rs.compute_hypotheses(p3, p2, rand31=rr)) == EINVAL
    assert code(lambda: rs.compute_hypotheses(p3[:3], p2[:3], rand31=ok)) == EINVAL  # n < 4 with draws
    assert code(lambda: rs.compute_pose(p3, p2, [])) == EINVAL
    assert code(lambda: _native.check(lib.orb_pnp_ransac(*head[:10], p(ok), p(ok), 10, 0, *([None] * 12), 0))) == EINVAL
    assert code(lambda: _native.check(lib.orb_pnp_ransac(*head[:10], None, None, 10, 0, *([None] * 12), 0))) == EINVAL
    assert code(lambda: rs.iterate(p3, p2, s2, rand31=np.zeros((1025, 4), np.int32))) == EINVAL
    assert code(lambda: rs.iterate(p3, p2, s2, rand31=np.zeros((0, 4), np.int32))) == EINVAL
    big = ransac_of(8193, 3)
    assert code(lambda: rs.iterate(*big, rand31=ok)) == ENOTSUP
    bad_s2 = s2.copy()
    bad_s2[3] = np.nan
    assert code(lambda: rs.iterate(p3, p2, bad_s2, rand31=ok)) == EINVAL


# ---- the batch form ------------------------------------------------------------------------------------
def synthetic_batch(ns, cap, seed):
    """A keyframe (0) and a frame (1) without an extractor: frame keypoint j sees the keyframe's
    MapPoint perm[j] (one in four grossly off); solver s keeps ns[s] of those matches."""
    import torch

    rng = np.random.default_rng(seed)
    S = len(ns)
    p3, p2, _, _ = pm.scene(cap, seed, noise=1.0, outliers=0.25)
    perm = rng.permutation(cap)
    pos = np.zeros((2, cap, 3), f32)
    pos[0, perm] = p3
    kps = np.zeros((2, cap), _native.KEYPOINT_DTYPE)
    kps["x"][1], kps["y"][1] = p2[:, 0], p2[:, 1]
    kps["octave"][1] = rng.integers(0, 3, cap)
    rows = np.full((S, cap), -1, np.int32)
    for s, n in enumerate(ns):
        j = np.sort(rng.choice(cap, n, replace=False))
        rows[s, j] = perm[j]
    bad = (rng.random((2, cap)) < 0.1).astype(np.uint8)
    tc = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    dev = {"d_kps": tc(kps.view(np.uint8).reshape(2, cap, -1)), "d_cnt": tc(np.int32([cap, cap])),
           "pa": tc(np.zeros(S, np.int32)), "pb": tc(np.ones(S, np.int32)), "rows": tc(rows), "pos": tc(pos),
           "bad": tc(bad)}
    return {"rows": rows, "pos": pos, "kps": kps, "bad": bad, "cap": cap, "dev": dev}


def check_batch(out, b, rs, r, best_in, bad, solvers):
    cap, n_hyp = b["cap"], r.shape[1]
    W = (cap + 63) // 64
    seen = []
    for s in solvers:
        su = model.pnp_setup(b["kps"][1], cap, cap, b["rows"][s], b["pos"][0], bad, LS2)
        n = su["n"]
        seen.append(n)
        assert int(out["n"][s]) == n and np.array_equal(out["index"][s], su["index"])
        it = rs.iterate(su["p3d"], su["p2d"], su["sigma2"], rand31=r[s], best_in=int(best_in[s]))
        for k, cols in (("R", 9), ("t", 3), ("sets", 4)):
            same(out[k][s].reshape(n_hyp, cols), it[k].reshape(n_hyp, cols), f"{k} of solver {s} (n = {n})")
        for k in ("counts", "best_at", "refined_counts"):
            same(out[k][s], it[k], f"{k} of solver {s} (n = {n})")
        for k in ("first_ok", "first_refined", "pose_inliers"):
            assert int(out[k][s]) == it[k], f"{k} of solver {s} (n = {n})"
        same(out["pose"][s], it["pose"], f"pose of solver {s}")
        masks, pmask = out["masks"][s].view(np.uint64), out["pose_mask"][s].view(np.uint64)
        wm = it["masks"].shape[1]
        assert masks.shape[1] == W and np.array_equal(masks[:, :wm], it["masks"]) and not masks[:, wm:].any()
        assert np.array_equal(pmask[:wm], it["pose_mask"]) and not pmask[wm:].any()
    return seen


@pytest.mark.parametrize("S,cap", [(1, 64), (3, 64), (17, 256)])
def test_batch_equals_host_call(S, cap):
    import torch

    ns = ([40], [0, cap, 30], [0, 3, 4, 90, cap, 9, 10, 64, 65, 128, 5, 200, 33, 150, 12, 255, 70])[(1, 3, 17).index(S)]
    b = synthetic_batch(ns, cap, 300 + S)
    n_hyp, mi = 70, 10
    rng = np.random.default_rng(S)
    r = rng.integers(0, 2 ** 31, (S, n_hyp, 4)).astype(np.int32)
    r[:, 0], r[:, 1] = 0, 2 ** 31 - 1
    best_in = rng.integers(0, 3, S).astype(np.int32)
    rs = orb.PnPRansac(*K32, min_inliers=mi, th2=TH2)
    d = b["dev"]
    tc = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    for with_bad in (True, False):
        out = rs.iterate_batch_device(d["d_kps"], d["d_cnt"], d["pa"], d["pb"], d["rows"], d["pos"],
                                      d["bad"] if with_bad else None, LS2, tc(r), tc(best_in))
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in out.items()}
        seen = check_batch(out, b, rs, r, best_in, b["bad"][0] if with_bad else None, range(S))
        if not with_bad:
            assert seen == ns
            if S > 1:
                assert (out["first_refined"] >= 0).any() and (out["first_refined"] < 0).any()


def test_device_call_then_host_call_without_a_synchronise(golden):
    import torch

    g, S, cap = golden, 5, 256
    b = synthetic_batch([200, 120, 60, 256, 8], cap, 77)
    r = np.random.default_rng(21).integers(0, 2 ** 31, (S, 300, 4)).astype(np.int32)
    rs = orb.PnPRansac(*K32, min_inliers=10, th2=TH2)
    d = b["dev"]
    d_r = torch.from_numpy(r).cuda()
    torch.cuda.synchronize()
    out = rs.iterate_batch_device(d["d_kps"], d["d_cnt"], d["pa"], d["pb"], d["rows"], d["pos"], d["bad"], LS2, d_r)
    it = orb.PnPRansac(*g["K"], min_inliers=int(g["min_inliers"]), th2=float(g["th2"])).iterate(
        g["p3d"], g["p2d"], g["sigma2"], rand31=g["rand31"])
    same(it["counts"], g["counts"], "host counts")
    same(it["pose"], g["pose"], "host pose")
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    check_batch(out, b, rs, r, np.zeros(S, np.int32), b["bad"][0], (0, 3, 4))


def test_pose_feeds_pose_optimization_unchanged():
    import torch

    S, cap = 4, 256
    b = synthetic_batch([200, 150, 100, 256], cap, 55)
    r = np.random.default_rng(8).integers(0, 2 ** 31, (S, 100, 4)).astype(np.int32)
    d = b["dev"]
    out = orb.PnPRansac(*K32, min_inliers=20, th2=TH2).iterate_batch_device(
        d["d_kps"], d["d_cnt"], d["pa"], d["pb"], d["rows"], d["pos"], None, LS2, torch.from_numpy(r).cuda())
    # PoseOptimization's problems: the frame's keypoints with the MapPoints the rows name
    rows = b["rows"]
    mp = np.zeros((S, cap, 3), f32)
    has = (rows >= 0).astype(np.uint8)
    for s in range(S):
        mp[s, rows[s] >= 0] = b["pos"][0][rows[s][rows[s] >= 0]]
    tc = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    opt = orb.Optimizer()
    args = (d["d_kps"], d["d_cnt"], d["pb"], tc(mp), tc(has), (1 / LS2).astype(f32), K32)
    a = opt.pose_optimization_batch_device(*args, out["pose"])
    torch.cuda.synchronize()
    pose = out["pose"].cpu().numpy()
    assert np.isfinite(pose).all() and (out["first_refined"].cpu().numpy() >= 0).all()
    c = opt.pose_optimization_batch_device(*args, tc(pose.copy()))
    torch.cuda.synchronize()
    for k in ("pose", "pose_f64", "outlier", "n_inliers"):
        assert a[k].cpu().numpy().tobytes() == c[k].cpu().numpy().tobytes(), k


# ---- the C++ facade ----------------------------------------------------------------------------------
def _fnv(flags):
    h = 2166136261
    for v in flags:
        h = ((h ^ int(bool(v))) * 16777619) & 0xFFFFFFFF
    return h


def test_native_facade(tmp_path):
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge

    exe = ROOT / "build" / "pnp_solver_facade"
    if not exe.exists():
        exe.parent.mkdir(exist_ok=True)
        subprocess.run(ge.PNP_SOLVER_FACADE_CMD(exe), check=True)
    rng = np.random.default_rng(41)
    nk, mi, max_its, block = 300, 10, 300, 5
    p3, p2, _, _ = pm.scene(nk, 12, noise=1.0, outliers=0.4)
    kps = np.zeros(nk, _native.KEYPOINT_DTYPE)
    kps["x"], kps["y"] = p2[:, 0], p2[:, 1]
    kps["octave"] = rng.integers(0, 8, nk)
    usable = (rng.random(nk) < 0.7).astype(np.uint8)
    r = rng.integers(0, 2 ** 31, (max_its + block, 4)).astype(np.int32)
    path = tmp_path / "pnp_solver.bin"
    with open(path, "wb") as f:
        f.write(np.int32([nk, len(LS2), mi, max_its, block, len(r)]).tobytes())
        f.write(K32.tobytes())
        for a in (kps, LS2.astype(f32), usable, p3, r):
            f.write(np.ascontiguousarray(a).tobytes())
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    # the same walk with the model: iterate(block) with the state carried, then one find
    su = model.pnp_setup(kps, nk, nk, np.where(usable, np.arange(nk), -1), p3, None, LS2)
    par = orb.pnp_ransac_parameters(su["n"], 0.99, mi, max_its, 4, 0.5, 5.991)
    want = [f"PNP N={su['n']} min={par['min_inliers']} maxits={par['max_iterations']}"]

    def walk(step, tag):
        its, best, used = 0, 0, 0
        best_pose, best_flags = np.zeros(12, f32), np.zeros(su["n"], bool)
        while True:
            k = orb.PnPRansac.iterations(par["max_iterations"], its, step)
            m = pm.ransac(su["p3d"], su["p2d"], su["sigma2"], TH2, K64, par["min_inliers"], rand31=r[used:used + k],
                          best_in=best)
            fr = m["first_refined"]
            last = fr if fr >= 0 else k - 1
            its, used = its + last + 1, used + last + 1
            if m["best_at"][last] >= 0:
                h = int(m["best_at"][last])
                best, best_flags = int(m["counts"][h]), model.unpack(m["masks"][h], su["n"])
                best_pose = f32(np.concatenate([m["R"][h], m["t"][h]]))
            vb, n_in, pose = np.zeros(nk, bool), 0, None
            if fr >= 0:
                vb[su["index"][:su["n"]][model.unpack(m["pose_mask"], su["n"])]] = True
                n_in, pose = m["pose_inliers"], m["pose"]
            elif best >= par["min_inliers"]:
                vb[su["index"][:su["n"]][best_flags]] = True
                n_in, pose = best, best_pose
            ok, no_more = pose is not None, fr < 0
            if not ok:
                vb = np.zeros(0, bool)  # vbInliers.clear() and nothing more
            head = f"ITER ok={int(ok)} nomore={int(no_more)}" if tag == "ITER" else f"FIND ok={int(ok)}"
            tail = f" used={(last + 1) * 4}" if tag == "ITER" else ""
            want.append(f"{head} its={its} best={best} n={n_in} flags={int(vb.sum())} hash={_fnv(vb):08x}{tail}")
            if ok or no_more:
                if ok:
                    want.append("TCW " + " ".join(f"{int(v):08x}" for v in pose.view(np.uint32)))
                return ok, fr

    ok_a, _ = walk(block, "ITER")
    ok_b, fr_b = walk(par["max_iterations"], "FIND")
    want.append("pnp solver facade OK")
    assert lines == want
    assert ok_a and ok_b and fr_b >= block, "the pose must not come in the first five iterations"
