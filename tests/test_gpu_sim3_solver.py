"""GPU parity of the Sim3Solver hypotheses and the whole RANSAC (csrc/orb_solvers.hip:
orb_sim3_compute_hypotheses, orb_sim3_ransac, orb_sim3_ransac_batch_device) against the CPU model
(tests/native/sim3_solver_model.cpp with tests/native/solvers_model.cpp).

Sets and the quaternion (everything before the first libm call) are compared bit for bit.  T12, T21
and the Sim3 are compared within the tolerance that scripts/gen_sim3_solver_golden.py measured on the
CPU and stored in the fixture: 4 x the largest deviation among the model's variants that move atan2,
cos and sin by one ulp.  That deviation is 0 on the fixture (a one-ulp change of a double moves its
float rounding with probability 2^-29), so the bound is 0 and the comparison is exact.  Counts,
masks, best_at and first_accept are exact."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import orbslam_jpminipc_amd as orb
from orbslam_jpminipc_amd import _native
import sim3_solver_model as s3
import solvers_model as model

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
f32 = np.float32
K_SMALL = f32([260, 260, 160, 120])
LS2 = model.LEVEL_SIGMA2
N_CASES = [3, 4, 63, 64, 65, 200]
HYP_CASES = [1, 63, 64, 65, 300, 1024]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(ROOT / "tests" / "golden" / "sim3_solver_320x240.npz"))


def r_for(randi, size):
    return (randi * 2 ** 31 + 2 ** 30) // size


def draws(n, n_hyp, seed):
    """rand() values with 0, 2^31 - 1 and, from the third triple on, one in eight that lands on the
    overwritten entry (the removal quirk)."""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 2 ** 31, (n_hyp, 3))
    r[0] = 0
    if n_hyp > 1:
        r[1] = 2 ** 31 - 1
    if n >= 5:
        for h in range(2, n_hyp, 8):
            i0 = int(rng.integers(0, n - 2))
            r[h] = [r_for(i0, n), r_for(i0, n - 1), r_for(i0, n - 2)]
    return r.astype(np.int32)


def close(got, want, tol, what):
    """NaN positions equal, everything else within tol (absolute); returns the largest deviation."""
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ"
    with np.errstate(invalid="ignore"):
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    d = float(np.nanmax(d)) if np.isfinite(d).any() else 0.0
    assert d <= tol, f"{what}: deviation {d:.3e} above the bound {tol:.3e}"
    return d


def same_bits(a, b, what):
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), what


def synthetic_batch(ns, cap=256, seed=0):
    """A two-keyframe batch without an extractor: solver s has exactly ns[s] correspondences (the
    keypoint records are zeros: octave 0)."""
    import torch

    rng = np.random.default_rng(seed)
    S = len(ns)
    rows = np.full((S, cap), -1, np.int32)
    for s, n in enumerate(ns):
        i1 = np.sort(rng.choice(cap, n, replace=False))
        rows[s, i1] = rng.permutation(cap)[:n]
    pos = np.stack([rng.uniform(-2, 2, (2, cap)), rng.uniform(-1.5, 1.5, (2, cap)), rng.uniform(2, 8, (2, cap))],
                   2).astype(f32)
    pose = np.zeros((2, 12), f32)
    pose[:, [0, 4, 8]] = 1
    pose[1, 9:] = [0.1, -0.05, 0.2]
    kps = np.zeros((2, cap), _native.KEYPOINT_DTYPE)
    tc = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    dev = {"d_kps": tc(kps.view(np.uint8).reshape(2, cap, -1)), "d_cnt": tc(np.int32([cap, cap])),
           "pa": tc(np.zeros(S, np.int32)), "pb": tc(np.ones(S, np.int32)), "rows": tc(rows), "pos": tc(pos),
           "pose": tc(pose)}
    return {"rows": rows, "pos": pos, "pose": pose, "kps": kps, "cap": cap, "dev": dev}


def setup_of(b, s, kps1, n1, kps2, n2, f1, f2, bad=None):
    return model.sim3_setup(kps1, n1, kps2, n2, b["rows"][s], b["pos"][f1], None if bad is None else bad[f1],
                            b["pos"][f2], None if bad is None else bad[f2], b["pose"][f1], b["pose"][f2], LS2)


# ---- the sets and the quaternion ---------------------------------------------------------------------
@pytest.mark.parametrize("n_hyp", HYP_CASES)
def test_sets_and_quaternion_are_exact(n_hyp):
    import torch

    rs = orb.Sim3Ransac(K_SMALL, None, 3)
    b = synthetic_batch(N_CASES, seed=n_hyp)
    r_all = np.stack([draws(n, n_hyp, 10 * n_hyp + n) for n in N_CASES])
    d = b["dev"]
    out = rs.iterate_batch_device(d["d_kps"], d["d_cnt"], d["pa"], d["pb"], d["rows"], d["pos"], None, d["pose"], LS2,
                                  torch.from_numpy(r_all).cuda())
    torch.cuda.synchronize()
    sets_b, n_b = out["sets"].cpu().numpy(), out["n"].cpu().numpy()
    quirk = 0
    for s, n in enumerate(N_CASES):
        r = r_all[s]
        want = orb.sim3_minimal_sets(n, r)
        assert np.array_equal(want, s3.sets(n, r))
        quirk += int((want != orb.sim3_minimal_sets(n, r, fixed=True)).any(1).sum())
        su = setup_of(b, s, b["kps"][0], b["cap"], b["kps"][1], b["cap"], 0, 1)
        assert su["n"] == n == int(n_b[s])
        hyp = rs.compute_hypotheses(su["x3dc1"], su["x3dc2"], rand31=r)
        assert np.array_equal(hyp["sets"], want), f"compute_hypotheses sets, n = {n}"
        m = s3.compute(su["x3dc1"], su["x3dc2"], want)
        same_bits(hyp["quat"], m["quat"], f"quaternion, n = {n}: an operation before the first libm call differs")
        by_sets = rs.compute_hypotheses(su["x3dc1"], su["x3dc2"], sets=want)
        same_bits(by_sets["quat"], m["quat"], "quaternion from sets")
        same_bits(by_sets["T12"], hyp["T12"], "the same sets give the same hypotheses")
        it = rs.iterate(su["x3dc1"], su["x3dc2"], su["sigma2_1"], su["sigma2_2"], rand31=r)
        assert np.array_equal(it["sets"], want), f"ransac sets, n = {n}"
        assert np.array_equal(sets_b[s], want), f"batch sets, n = {n}"
    if n_hyp >= 63:
        assert quirk >= 8, "the removal quirk must show in the draws"


# ---- R, t, s -----------------------------------------------------------------------------------------
def test_golden_hypotheses_within_the_measured_tolerance(golden, capsys):
    g = golden
    rs = orb.Sim3Ransac(g["K"], g["K"], int(g["min_inliers"]))
    hyp = rs.compute_hypotheses(g["x3dc1"], g["x3dc2"], rand31=g["rand31"])
    assert np.array_equal(hyp["sets"], g["sets"])
    assert np.array_equal(g["sets"], orb.sim3_minimal_sets(len(g["x3dc1"]), g["rand31"]))
    same_bits(hyp["quat"], g["quat"], "quaternion")
    with capsys.disabled():
        dev = {k: close(hyp[k], g[k], np.inf, k) for k in ("T12", "T21", "sim3")}
        print(f"\nsim3 hypotheses GPU vs model: deviation {dev}, bound "
              f"{ {k: float(g['tol_' + k]) for k in dev} }")
    for k in ("T12", "T21", "sim3"):
        close(hyp[k], g[k], float(g["tol_" + k]), k)


def test_degenerate_sets_are_not_repaired():
    x2 = f32([[1, 2, 4], [2, -4, 1], [-3, 2, -5], [0.5, 0.25, 8], [1, 1, 3]])
    x1 = 2 * x2 + f32([1, 2, 4])
    sets = [[0, 1, 2], [3, 3, 3], [1, 4, 4], [0, 1, 3]]
    rs = orb.Sim3Ransac(K_SMALL, None, 3)
    hyp = rs.compute_hypotheses(x1, x2, sets=sets)
    m = s3.compute(x1, x2, sets)
    same_bits(hyp["quat"], m["quat"], "quaternion")
    assert hyp["quat"][0].tolist() == [1, 0, 0, 0] and np.isnan(hyp["T12"][0]).all() and np.isnan(hyp["T21"][0]).all()
    assert np.isnan(hyp["sim3"][1]).any(), "three times one point divides 0 by 0"
    for k in ("T12", "T21", "sim3"):
        close(hyp[k], m[k], 0.0, k)
    s2 = np.ones(5, f32)
    it = rs.iterate(x1, x2, s2, s2, sets=sets)
    want = s3.iterate(x1, x2, s2, s2, K_SMALL, K_SMALL, None, 3, sets_=sets)
    model.same_result(it, want, "first_accept")
    assert it["counts"][0] == 0 and it["counts"][1] == 0, "a NaN error is an outlier"


# ---- the host fused call -----------------------------------------------------------------------------
def test_ransac_equals_check_inliers_on_its_own_hypotheses_and_the_model(golden):
    g = golden
    a = (g["x3dc1"], g["x3dc2"], g["sigma2_1"], g["sigma2_2"])
    mi = int(g["min_inliers"])
    rs = orb.Sim3Ransac(g["K"], g["K"], mi)
    for best_in in (0, 30):
        it = rs.iterate(*a, rand31=g["rand31"], best_in=best_in)
        chk = orb.Sim3Consensus(g["K"], g["K"], mi).check(*a, it["T12"], it["T21"], best_in)
        model.same_result(it, chk, "first_accept")
    it = rs.iterate(*a, rand31=g["rand31"])
    assert np.array_equal(it["counts"], g["counts"]), "counts differ from the fixture"
    assert np.array_equal(it["masks"], g["masks"]), "masks differ from the fixture"
    assert np.array_equal(it["best_at"], g["best_at"]) and it["first_accept"] == int(g["first_accept"])
    close(it["accepted"], g["accepted"], float(g["tol_sim3"]), "accepted")
    same_bits(it["accepted"], it["sim3"][it["first_accept"]], "accepted is the first accepted hypothesis")
    # nothing accepted: accepted is mBestT12's Sim3; the earlier calls' best still standing: NaN
    hi = orb.Sim3Ransac(g["K"], g["K"], 199)
    it = hi.iterate(*a, rand31=g["rand31"][:40])
    assert it["first_accept"] == -1
    same_bits(it["accepted"], it["sim3"][it["best_at"][-1]], "accepted without an acceptance")
    it = hi.iterate(*a, rand31=g["rand31"][:40], best_in=199)
    assert set(it["best_at"]) == {-2} and np.isnan(it["accepted"]).all()
    # bNoMore: fewer correspondences than min_inliers
    it = hi.iterate(a[0][:50], a[1][:50], a[2][:50], a[3][:50], rand31=g["rand31"][:70])
    assert not it["counts"].any() and it["first_accept"] == -1 and not it["sets"].any()
    assert not it["T12"].any() and not it["T21"].any() and not it["sim3"].any() and not it["masks"].any()


def iterate_against_model(golden, n, n_hyp, seed):
    """orb_sim3_ransac on the first n points of a cloud: the sets and the quaternion bit for bit, the
    hypotheses and the accepted one within the fixture's bound (0), the consensus exact."""
    tol = {k: float(golden["tol_" + k]) for k in ("T12", "T21", "sim3")}
    c = s3.cloud(130, seed=seed, outliers=0.3)
    a = tuple(c[k][:n] for k in ("x3dc1", "x3dc2", "sigma2_1", "sigma2_2"))
    r = draws(n, n_hyp, seed)
    rs = orb.Sim3Ransac(K_SMALL, None, 10)
    it = rs.iterate(*a, rand31=r)
    want = s3.iterate(*a, K_SMALL, K_SMALL, r, 10)
    model.same_result(it, want, "first_accept")
    assert np.array_equal(it["sets"], want["sets"]), f"sets, n = {n}"
    for k in ("T12", "T21", "sim3"):
        close(it[k], want[k], tol[k], f"{k}, n = {n}")
    close(it["accepted"], want["accepted"], tol["sim3"], f"accepted, n = {n}")
    if n >= 3:
        hyp = rs.compute_hypotheses(a[0], a[1], rand31=r)
        same_bits(hyp["quat"], s3.compute(a[0], a[1], hyp["sets"])["quat"], f"quaternion, n = {n}")
    return it


def test_staging_reuse_across_sizes(golden):
    """One thread, one context: a small call, one large enough to grow the device arena and the pinned
    staging, a small one again and the empty input, each against the model: a layout that leans on
    what an earlier call left in the staging, or on where the arena was before it grew, fails."""
    for n, n_hyp in [(65, 1), (130, 65), (1, 1), (0, 1)]:
        it = iterate_against_model(golden, n, n_hyp, 8)
        assert it["masks"].shape == (n_hyp, (n + 63) // 64)


def test_null_outputs_host():
    lib, p = _native.hip_lib(), _native.ptr
    c = s3.cloud(130, seed=8, outliers=0.3)
    r = draws(130, 5, 3)
    K = K_SMALL
    a = (130, p(c["x3dc1"]), p(c["x3dc2"]), p(c["sigma2_1"]), p(c["sigma2_2"]), p(K), p(K), 5, None, p(r), 10, 0)
    _native.check(lib.orb_sim3_ransac(*a, *([None] * 9), 0))
    counts = np.zeros(5, np.int32)
    _native.check(lib.orb_sim3_ransac(*a, p(counts), *([None] * 8), 0))
    want = s3.iterate(c["x3dc1"], c["x3dc2"], c["sigma2_1"], c["sigma2_2"], K, K, r, 10)
    assert np.array_equal(counts, want["counts"])
    _native.check(lib.orb_sim3_compute_hypotheses(130, p(c["x3dc1"]), p(c["x3dc2"]), 5, None, p(r), *([None] * 5), 0))


# ---- the batch form ----------------------------------------------------------------------------------
B, CAP_W, CAP_H, NF = 6, 320, 240, 500


@pytest.fixture(scope="module")
def batch():
    """A 6-keyframe extractor batch with SearchByBoW(KF, KF) rows for every ordered pair, MapPoint
    positions / bad flags and poses, as tests/test_gpu_solvers.py builds its own; row 1 is all -1
    and row 4 keeps exactly three matches."""
    import torch

    from vocab_util import random_vocabulary

    frames = orb.synth_stream(CAP_W, CAP_H, stream=5, first=0, count=B)
    ext = orb.ORBextractor(NF, 1.2, 8, orb.FAST_SCORE, 20, device=0, max_batch=B)
    d_kps, d_desc, d_cnt = ext.extract_batch_device(torch.from_numpy(frames).cuda())
    voc = orb.ORBVocabulary.from_arrays(8, 3, 0, 0, *random_vocabulary(8, 3, seed=3))
    fv = voc.transform_batch_device(d_desc, d_cnt, 1)
    pairs = [(a, b) for a in range(B) for b in range(B) if a != b]
    pa = torch.tensor([p[0] for p in pairs], dtype=torch.int32, device="cuda")
    pb = torch.tensor([p[1] for p in pairs], dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(78)
    cap = int(d_kps.shape[1])
    m, _ = orb.ORBmatcher(0.9, True).search_by_bow_batch_device(True, d_kps, d_desc, d_cnt, fv, pa, pb)
    rows = m.cpu().numpy().copy()
    cnt = d_cnt.cpu().numpy()
    kps = d_kps.cpu().numpy().view(_native.KEYPOINT_DTYPE).reshape(B, cap)
    bad = (rng.random((B, cap)) < 0.1).astype(np.uint8)
    rows[1, :] = -1
    rows[2, 5] = cap + 100  # beyond every count
    f1, f2 = pairs[4]
    ok = np.flatnonzero((rows[4] >= 0) & (rows[4] < cnt[f2]) & (np.arange(cap) < cnt[f1]))
    ok = ok[(bad[f1, ok] == 0) & (bad[f2, rows[4][ok]] == 0)]
    rows[4, ok[3:]] = -1
    pose = np.zeros((B, 12), f32)
    for b in range(B):
        pose[b, :9] = model.rodrigues(rng.normal(0, 0.05, 3)).reshape(9)
        pose[b, 9:] = rng.normal(0, 0.1, 3)
    # the second keyframe's MapPoints where the first one's are (camera coordinates, a third of them
    # displaced), so that good minimal sets find inliers; a MapPoint of a keyframe serves one pair
    pos = np.stack([rng.uniform(-2, 2, (B, cap)), rng.uniform(-1.5, 1.5, (B, cap)), rng.uniform(2, 8, (B, cap))],
                   2).astype(f32)
    return {"d_kps": d_kps, "d_cnt": d_cnt, "kps": kps, "cnt": cnt, "cap": cap, "pairs": pairs, "rows": rows,
            "pos": pos, "bad": bad, "pose": pose}


def _case(b, S, seed):
    """S solvers cycling over the pairs; per-solver consistent MapPoint positions are not possible
    with shared keyframes, so every solver of a call uses pairs (a, b) with the positions of b made
    consistent with a for the first pair that names b."""
    idx = [s % len(b["pairs"]) for s in range(S)]
    k1 = [b["pairs"][i][0] for i in idx]
    k2 = [b["pairs"][i][1] for i in idx]
    rows = b["rows"][idx]
    pos = b["pos"].copy()
    rng = np.random.default_rng(seed)
    cap = b["cap"]
    done = set()
    for s in range(S):
        if k2[s] in done or k2[s] == 0:
            continue
        done.add(k2[s])
        i1 = np.flatnonzero((rows[s] >= 0) & (rows[s] < b["cnt"][k2[s]]) & (np.arange(cap) < b["cnt"][k1[s]]))
        Ra, ta = b["pose"][k1[s], :9].reshape(3, 3).astype(np.float64), b["pose"][k1[s], 9:].astype(np.float64)
        Rb, tb = b["pose"][k2[s], :9].reshape(3, 3).astype(np.float64), b["pose"][k2[s], 9:].astype(np.float64)
        Xc = pos[k1[s], i1].astype(np.float64) @ Ra.T + ta + rng.normal(0, 0.003, (len(i1), 3))
        pos[k2[s], rows[s][i1]] = ((Xc - tb) @ Rb).astype(f32)
    return idx, k1, k2, rows, pos


@pytest.mark.parametrize("S", [1, 3, 50])
def test_batch_equals_host_call(batch, S):
    import torch

    b, cap, n_hyp, mi = batch, batch["cap"], 70, 3
    idx, k1, k2, rows, pos = _case(b, S, S)
    rng = np.random.default_rng(200 + S)
    r = rng.integers(0, 2 ** 31, (S, n_hyp, 3)).astype(np.int32)
    r[:, 0], r[:, 1] = 0, 2 ** 31 - 1
    best_in = rng.integers(0, 3, S).astype(np.int32)
    rs = orb.Sim3Ransac(K_SMALL, None, mi)
    tc = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    out = rs.iterate_batch_device(b["d_kps"], b["d_cnt"], tc(np.int32(k1)), tc(np.int32(k2)), tc(rows), tc(pos),
                                  tc(b["bad"]), tc(b["pose"]), LS2, tc(r), tc(best_in))
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    W = (cap + 63) // 64
    seen = set()
    for s in range(S):
        su = model.sim3_setup(b["kps"][k1[s]], b["cnt"][k1[s]], b["kps"][k2[s]], b["cnt"][k2[s]], rows[s], pos[k1[s]],
                              b["bad"][k1[s]], pos[k2[s]], b["bad"][k2[s]], b["pose"][k1[s]], b["pose"][k2[s]], LS2)
        n = su["n"]
        seen.add(n)
        assert int(out["n"][s]) == n and np.array_equal(out["index"][s], su["index"])
        it = rs.iterate(su["x3dc1"], su["x3dc2"], su["sigma2_1"], su["sigma2_2"], rand31=r[s], best_in=int(best_in[s]))
        for k, cols in (("T12", 12), ("T21", 12), ("sim3", 13), ("sets", 3)):
            same_bits(out[k][s].reshape(n_hyp, cols), it[k].reshape(n_hyp, cols), f"{k} of solver {s} (n = {n})")
        assert np.array_equal(out["counts"][s], it["counts"]) and np.array_equal(out["best_at"][s], it["best_at"])
        assert int(out["first_accept"][s]) == it["first_accept"]
        masks = out["masks"][s].view(np.uint64)
        wm = it["masks"].shape[1]
        assert masks.shape[1] == W and np.array_equal(masks[:, :wm], it["masks"]) and not masks[:, wm:].any()
        same_bits(out["accepted"][s], it["accepted"], f"accepted of solver {s}")
        h = it["first_accept"] if it["first_accept"] >= 0 else int(it["best_at"][-1])
        am = out["accepted_mask"][s].view(np.uint64)
        assert np.array_equal(am, masks[h]) if h >= 0 else not am.any()
        if n >= mi:
            assert np.array_equal(it["sets"], orb.sim3_minimal_sets(n, r[s]))
        else:
            assert not it["sets"].any() and not it["counts"].any() and it["first_accept"] == -1
    if S >= 3:
        assert 0 in seen and max(seen) >= 8
    if S == 50:
        assert 3 in seen and out["counts"].max() >= 6 and (out["first_accept"] >= 0).any()


def test_batch_null_outputs_and_no_bad_flags(batch):
    import torch

    b, cap = batch, batch["cap"]
    idx, k1, k2, rows, pos = _case(b, 3, 5)
    r = np.random.default_rng(9).integers(0, 2 ** 31, (3, 4, 3)).astype(np.int32)
    tc = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d = [tc(np.int32(k1)), tc(np.int32(k2)), tc(rows), tc(pos), tc(b["pose"]), tc(r)]
    acc = torch.full((3, 13), -1, dtype=torch.float32, device="cuda")
    p = _native.ptr
    lib = _native.hip_lib()
    head = (p(b["d_kps"]), p(b["d_cnt"]), cap, 3, p(d[0]), p(d[1]), p(d[2]), p(d[3]), None, p(d[4]), p(LS2), len(LS2),
            p(K_SMALL), 4, p(d[5]), 3, None)
    _native.check(lib.orb_sim3_ransac_batch_device(*head, *([None] * 13)))
    _native.check(lib.orb_sim3_ransac_batch_device(*head, *([None] * 10), p(acc), None, None))
    torch.cuda.synchronize()
    rs = orb.Sim3Ransac(K_SMALL, None, 3)
    for s in range(3):
        su = model.sim3_setup(b["kps"][k1[s]], b["cnt"][k1[s]], b["kps"][k2[s]], b["cnt"][k2[s]], rows[s], pos[k1[s]], None,
                              pos[k2[s]], None, b["pose"][k1[s]], b["pose"][k2[s]], LS2)
        it = rs.iterate(su["x3dc1"], su["x3dc2"], su["sigma2_1"], su["sigma2_2"], rand31=r[s])
        same_bits(acc[s].cpu().numpy(), it["accepted"], f"accepted of solver {s}")


def test_device_call_then_host_call_without_a_synchronise(batch, golden):
    import torch

    b, S, n_hyp = batch, 50, 300
    idx, k1, k2, rows, pos = _case(b, S, 6)
    r = np.random.default_rng(21).integers(0, 2 ** 31, (S, n_hyp, 3)).astype(np.int32)
    tc = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d = (tc(np.int32(k1)), tc(np.int32(k2)), tc(rows), tc(pos), tc(b["bad"]), tc(b["pose"]), tc(r))
    rs = orb.Sim3Ransac(K_SMALL, None, 5)
    g = golden
    torch.cuda.synchronize()
    out = rs.iterate_batch_device(b["d_kps"], b["d_cnt"], d[0], d[1], d[2], d[3], d[4], d[5], LS2, d[6])
    it = orb.Sim3Ransac(g["K"], g["K"], int(g["min_inliers"])).iterate(g["x3dc1"], g["x3dc2"], g["sigma2_1"],
                                                                       g["sigma2_2"], rand31=g["rand31"])
    assert np.array_equal(it["counts"], g["counts"]) and np.array_equal(it["masks"], g["masks"])
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for s in (0, 1, 17, 49):
        su = model.sim3_setup(b["kps"][k1[s]], b["cnt"][k1[s]], b["kps"][k2[s]], b["cnt"][k2[s]], rows[s], pos[k1[s]],
                              b["bad"][k1[s]], pos[k2[s]], b["bad"][k2[s]], b["pose"][k1[s]], b["pose"][k2[s]], LS2)
        want = rs.iterate(su["x3dc1"], su["x3dc2"], su["sigma2_1"], su["sigma2_2"], rand31=r[s])
        assert np.array_equal(out["counts"][s], want["counts"]) and int(out["first_accept"][s]) == want["first_accept"]
        same_bits(out["accepted"][s], want["accepted"], f"accepted of solver {s}")


# ---- the chain into OptimizeSim3 ---------------------------------------------------------------------
def test_accepted_feeds_optimize_sim3_unchanged(batch):
    import torch

    b, S = batch, 8
    idx, k1, k2, rows, pos = _case(b, S, 7)
    keep = [s for s in range(S) if s not in (1, 4)]  # not the empty row and the three-match row
    k1, k2, rows = [k1[s] for s in keep], [k2[s] for s in keep], rows[keep]
    r = np.random.default_rng(33).integers(0, 2 ** 31, (len(keep), 100, 3)).astype(np.int32)
    tc = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d = (tc(np.int32(k1)), tc(np.int32(k2)), tc(rows), tc(pos), tc(b["bad"]), tc(b["pose"]))
    out = orb.Sim3Ransac(K_SMALL, None, 5).iterate_batch_device(b["d_kps"], b["d_cnt"], *d, LS2, tc(r))
    opt = orb.Optimizer()
    a = opt.optimize_sim3_batch_device(b["d_kps"], b["d_cnt"], d[0], d[1], d[2], d[3], d[4], d[5], LS2, K_SMALL,
                                       out["accepted"])
    torch.cuda.synchronize()
    acc = out["accepted"].cpu().numpy()
    assert np.isfinite(acc).all()
    c = opt.optimize_sim3_batch_device(b["d_kps"], b["d_cnt"], d[0], d[1], d[2], d[3], d[4], d[5], LS2, K_SMALL,
                                       tc(acc.copy()))
    torch.cuda.synchronize()
    for k in ("match", "sim3", "sim3_f64", "n_inliers"):
        same_bits(a[k].cpu().numpy(), c[k].cpu().numpy(), k)


# ---- refusals ----------------------------------------------------------------------------------------
def test_refusals():
    def code(fn):
        with pytest.raises(_native.OrbError) as e:
            fn()
        assert str(e.value).split(":", 1)[1].strip(), "a refusal carries a message"
        return e.value.code

    c = s3.cloud(20, seed=9)
    a = (c["x3dc1"], c["x3dc2"], c["sigma2_1"], c["sigma2_2"])
    ok = np.zeros((4, 3), np.int32)
    rs = orb.Sim3Ransac(K_SMALL, None, 6)
    EINVAL, ENOTSUP = _native.ORB_EINVAL, _native.ORB_ENOTSUP
    assert code(lambda: orb.Sim3Ransac(K_SMALL, None, 2).iterate(*a, rand31=ok)) == EINVAL  # min_inliers < 3
    for bad in (-1, 20):
        s = ok.copy()
        s[2, 1] = bad
        assert code(lambda: rs.iterate(*a, sets=s)) == EINVAL
        assert code(lambda: rs.compute_hypotheses(a[0], a[1], sets=s)) == EINVAL
    r = ok.copy()
    r[3, 0] = -5
    assert code(lambda: rs.iterate(*a, rand31=r)) == EINVAL
    assert code(lambda: rs.compute_hypotheses(a[0], a[1], rand31=r)) == EINVAL
    lib, p = _native.hip_lib(), _native.ptr

    def raw(sets, rand31):
        _native.check(lib.orb_sim3_compute_hypotheses(20, p(a[0]), p(a[1]), 4, sets, rand31, *([None] * 5), 0))

    assert code(lambda: raw(p(ok), p(ok))) == EINVAL  # both
    assert code(lambda: raw(None, None)) == EINVAL    # neither
    assert code(lambda: rs.iterate(*a, rand31=np.zeros((1025, 3), np.int32))) == EINVAL
    assert code(lambda: rs.iterate(*a, rand31=np.zeros((0, 3), np.int32))) == EINVAL
    big = s3.cloud(8193, seed=10)
    assert code(lambda: rs.iterate(big["x3dc1"], big["x3dc2"], big["sigma2_1"], big["sigma2_2"], rand31=ok)) == ENOTSUP
    assert code(lambda: rs.compute_hypotheses(big["x3dc1"], big["x3dc2"], rand31=ok)) == ENOTSUP
    s2 = c["sigma2_2"].copy()
    s2[3] = np.nan
    assert code(lambda: rs.iterate(a[0], a[1], a[2], s2, rand31=ok)) == EINVAL
    # the batch form: min_inliers < 3, n_hyp and the solver limit
    b = synthetic_batch([5], cap=64)
    d = b["dev"]
    import torch

    def batch_call(mi, n_hyp, S=1, cap=64):
        r = torch.zeros((max(S, 1), n_hyp, 3), dtype=torch.int32, device="cuda")
        _native.check(lib.orb_sim3_ransac_batch_device(
            p(d["d_kps"]), p(d["d_cnt"]), cap, S, p(d["pa"]), p(d["pb"]), p(d["rows"]), p(d["pos"]), None, p(d["pose"]),
            p(LS2), len(LS2), p(K_SMALL), n_hyp, p(r), mi, *([None] * 14)))

    batch_call(3, 4)
    assert code(lambda: batch_call(2, 4)) == EINVAL
    assert code(lambda: batch_call(3, 1025)) == EINVAL
    assert code(lambda: batch_call(3, 4, S=65536)) == ENOTSUP
    assert code(lambda: batch_call(3, 4, cap=8193)) == ENOTSUP


# ---- the C++ facade ----------------------------------------------------------------------------------
def _fnv(flags):
    h = 2166136261
    for v in flags:
        h = ((h ^ int(bool(v))) * 16777619) & 0xFFFFFFFF
    return h


def test_native_facade(tmp_path):
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge

    exe = ROOT / "build" / "sim3_solver_facade"
    if not exe.exists():
        exe.parent.mkdir(exist_ok=True)
        subprocess.run(ge.SIM3_SOLVER_FACADE_CMD(exe), check=True)
    rng = np.random.default_rng(41)
    n, N1, mi, max_its, block = 150, 400, 40, 300, 5
    c = s3.cloud(n, seed=6, outliers=0.6)
    idx1 = np.sort(rng.choice(N1, n, replace=False)).astype(np.int32)
    r = rng.integers(0, 2 ** 31, (max_its, 3)).astype(np.int32)
    path = tmp_path / "sim3_solver.bin"
    with open(path, "wb") as f:
        f.write(np.int32([n, N1, mi, max_its, block, max_its]).tobytes())
        f.write(K_SMALL.tobytes())
        for a in (c["x3dc1"], c["x3dc2"], c["sigma2_1"], c["sigma2_2"], idx1, r):
            f.write(np.ascontiguousarray(a).tobytes())
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    # the same walk with the Python wrapper: blocks of 5 with the state carried, then one find
    rs = orb.Sim3Ransac(K_SMALL, None, mi)
    par = orb.sim3_ransac_parameters(n, 0.99, mi, max_its)
    a = (c["x3dc1"], c["x3dc2"], c["sigma2_1"], c["sigma2_2"])
    want = [f"SIM3 N={n} min={mi} maxits={par['max_iterations']}"]

    def walk(step, tag):
        its, best, used, est = 0, 0, 0, np.zeros(13, f32)
        while True:
            k = min(step, par["max_iterations"] - its)
            m = rs.iterate(*a, rand31=r[used:used + k], best_in=best)
            first = m["first_accept"]
            last = first if first >= 0 else k - 1
            its, used = its + last + 1, used + last + 1
            if m["best_at"][last] >= 0:
                h = int(m["best_at"][last])
                best, est = int(m["counts"][h]), m["sim3"][h]
            vb = np.zeros(N1, bool)
            n_in = 0
            if first >= 0:
                vb[idx1[m["inliers"][first]]] = True
                n_in = int(m["counts"][first])
            no_more = first < 0 and its >= par["max_iterations"]
            head = f"ITER ok={int(first >= 0)} nomore={int(no_more)}" if tag == "ITER" else f"FIND ok={int(first >= 0)}"
            want.append(f"{head} its={its} best={best} n={n_in} flags={int(vb.sum())} hash={_fnv(vb):08x}")
            if first >= 0 or no_more:
                want.append("EST " + " ".join(f"{int(v):08x}" for v in est.view(np.uint32)))
                return first >= 0, its, est, m

    ok_a, its_a, est_a, _ = walk(block, "ITER")
    ok_b, its_b, est_b, m = walk(par["max_iterations"], "FIND")
    want.append("sim3 solver facade OK")
    assert lines == want
    # iterate(5, ...) called repeatedly equals one find; R, t and s are `accepted`
    assert ok_a and ok_b and its_a == its_b and est_a.tobytes() == est_b.tobytes()
    assert est_b.tobytes() == m["accepted"].tobytes()
    assert sum(line.startswith("ITER") for line in lines) >= 2, "the acceptance must not come in the first block"
