"""GPU parity of the PnP / Sim3 RANSAC consensus (csrc/orb_solvers.hip: orb_pnp_check_inliers,
orb_sim3_check_inliers and their batch forms) against the CPU model (tests/native/solvers_model.cpp).
Counts, masks, best_at and the first indices are compared exactly: there is no tolerance."""
import ctypes
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import orbslam_jpminipc_amd as orb
from orbslam_jpminipc_amd import _native
import solvers_model as model

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
f32 = np.float32
TH2 = 5.991
N_CASES = [0, 1, 63, 64, 65, 127, 128, 129, 1000, 8192]
HYP_CASES = [1, 63, 64, 65, 300, 1024]


def run_pnp(c, min_inliers, best_in=0, th2=TH2):
    got = orb.PnPConsensus(*c["K"], min_inliers=min_inliers, th2=th2).check(c["p3d"], c["p2d"], c["sigma2"], c["R"],
                                                                            c["t"], best_in)
    want = model.pnp(c["p3d"], c["p2d"], c["sigma2"], th2, c["K"], c["R"], c["t"], min_inliers, best_in)
    model.same_result(got, want, "first_ok")
    return got


def run_sim3(c, min_inliers, best_in=0):
    a = (c["x3dc1"], c["x3dc2"], c["sigma2_1"], c["sigma2_2"])
    got = orb.Sim3Consensus(c["K1"], c["K2"], min_inliers).check(*a, c["T12"], c["T21"], best_in)
    want = model.sim3(*a, c["K1"], c["K2"], c["T12"], c["T21"], min_inliers, best_in)
    model.same_result(got, want, "first_accept")
    return got


def _bits_past_n_are_zero(r):
    n = r["n"]
    if n % 64 and r["masks"].shape[1]:
        assert not np.any(r["masks"][:, -1] >> np.uint64(n % 64)), "mask bits past n must be zero"


@pytest.mark.parametrize("n", N_CASES)
def test_correspondence_counts(n):
    r = run_pnp(model.pnp_case(n, 70, seed=n), min_inliers=max(4, n // 3))
    assert r["masks"].shape == (70, (n + 63) // 64)
    _bits_past_n_are_zero(r)
    r = run_sim3(model.sim3_case(n, 70, seed=n + 1), min_inliers=max(4, n // 3))
    assert r["masks"].shape == (70, (n + 63) // 64)
    _bits_past_n_are_zero(r)
    if n >= 63:
        assert r["counts"].max() > 0 and r["counts"].min() < n


@pytest.mark.parametrize("n_hyp", HYP_CASES)
def test_hypothesis_counts(n_hyp):
    # backwards: the running best changes hands along the way
    c = model.pnp_case(200, n_hyp, seed=n_hyp)
    c["R"], c["t"] = c["R"][::-1].copy(), c["t"][::-1].copy()
    r = run_pnp(c, min_inliers=40)
    s = model.sim3_case(200, n_hyp, seed=n_hyp + 1)
    s["T12"], s["T21"] = s["T12"][::-1].copy(), s["T21"][::-1].copy()
    q = run_sim3(s, min_inliers=40)
    if n_hyp >= 63:
        assert len(set(r["best_at"])) > 2 and len(set(q["best_at"])) > 2


REUSE = [(65, 1), (130, 65), (1, 1), (0, 1)]  # (n, n_hyp): mask words 2, 3, 1, 0; one and two tiles of hypotheses


@pytest.mark.parametrize("which", ["pnp", "sim3"])
def test_staging_reuse_across_sizes(which):
    """One thread, one context: a small call, one large enough to grow the device arena and the pinned
    staging, a small one again and the empty input, each against the model: a layout that leans on
    what an earlier call left in the staging, or on where the arena was before it grew, fails."""
    for n, n_hyp in REUSE:
        if which == "pnp":
            r = run_pnp(model.pnp_case(n, n_hyp, seed=n), min_inliers=max(4, n // 3))
        else:
            r = run_sim3(model.sim3_case(n, n_hyp, seed=n + 1), min_inliers=max(4, n // 3))
        assert r["masks"].shape == (n_hyp, (n + 63) // 64)
        _bits_past_n_are_zero(r)


def test_golden_fixture():
    g = np.load(ROOT / "tests" / "golden" / "solvers_320x240.npz")
    r = orb.PnPConsensus(*g["K"], min_inliers=int(g["pnp_min"]), th2=float(g["th2"])).check(
        g["p3d"], g["p2d"], g["pnp_sigma2"], g["R"], g["t"])
    assert np.array_equal(r["counts"], g["pnp_counts"]), "PnP counts differ from the fixture"
    assert np.array_equal(r["masks"], g["pnp_masks"]), "PnP masks differ from the fixture (float pattern?)"
    assert np.array_equal(r["best_at"], g["pnp_best_at"]) and r["first_ok"] == int(g["pnp_first_ok"])
    r = orb.Sim3Consensus(g["K"], g["K"], int(g["sim3_min"])).check(g["x3dc1"], g["x3dc2"], g["sigma2_1"],
                                                                    g["sigma2_2"], g["T12"], g["T21"])
    assert np.array_equal(r["counts"], g["sim3_counts"]), "Sim3 counts differ from the fixture"
    assert np.array_equal(r["masks"], g["sim3_masks"]), "Sim3 masks differ from the fixture (pattern or bound?)"
    assert np.array_equal(r["best_at"], g["sim3_best_at"]) and r["first_accept"] == int(g["sim3_first_accept"])


def test_boundary_nan_infinity_and_behind_camera():
    I3, T0 = np.eye(3).reshape(1, 9), np.zeros((1, 3))
    K = (100.0, 100.0, 0.0, 0.0)
    nx = np.nextafter(f32(25), f32(26))
    # PnP, th2 = 1: at the bound (outlier), one float above it (inlier), NaN, infinite, behind the
    # camera and consistent (inlier), behind the camera and not
    c = {"p3d": f32([[0, 0, 1], [0, 0, 1], [0, 0, 0], [1, 1, 0], [0.5, 0.25, -2], [0.5, 0.25, -2]]),
         "p2d": f32([[3, 4], [3, 4], [0, 0], [0, 0], [-24, -12.5], [26, 12.5]]),
         "sigma2": f32([25, nx, 1e30, 1e30, 2, 2]), "R": I3, "t": T0, "K": K}
    r = run_pnp(c, 1, th2=1.0)
    assert r["inliers"][0].tolist() == [False, True, False, False, True, False]
    # Sim3, fx = 96, identity: err = 9 at level 0 (bound 9: outlier), one float inside, level 1
    # err 13.14 (bound 13: outlier), err 12.25 (inlier), NaN, infinite, behind both cameras (inlier)
    TI = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(f32).reshape(1, 12)
    K96 = f32([96, 96, 0, 0])
    x2 = f32([[1 / 32, 0, 1], [np.nextafter(f32(1 / 32), f32(0)), 0, 1], [3.625 / 96, 0, 1], [3.5 / 96, 0, 1],
              [0, 0, 0], [1, 1, 0], [0.25, 0, -1]])
    x1 = f32([[0, 0, 1]] * 6 + [[0.25, 0, -1]])
    s = {"x3dc1": x1, "x3dc2": x2, "sigma2_1": f32([1, 1, 1.44, 1.44, 1, 1, 1]),
         "sigma2_2": f32([1, 1, 1.44, 1.44, 1, 1, 1]), "T12": TI, "T21": TI, "K1": K96, "K2": K96}
    r = run_sim3(s, 1)
    assert r["inliers"][0].tolist() == [False, True, False, True, False, False, True]


def test_keep_the_best_rules_and_best_in():
    c = model.pnp_case(100, 1, 3, outliers=0.5)
    c["R"], c["t"] = np.repeat(c["R"], 70, 0), np.repeat(c["t"], 70, 0)
    n_in = int(run_pnp(c, 4)["counts"][0])
    r = run_pnp(c, n_in)  # count == min_inliers qualifies; identical hypotheses: the first wins
    assert r["first_ok"] == 0 and set(r["best_at"]) == {0}
    assert run_pnp(c, n_in + 1)["first_ok"] == -1
    assert set(run_pnp(c, 4, best_in=n_in)["best_at"]) == {-2}
    assert set(run_pnp(c, 4, best_in=n_in - 1)["best_at"]) == {0}
    s = model.sim3_case(100, 1, 4, outliers=0.5)
    s["T12"], s["T21"] = np.repeat(s["T12"], 70, 0), np.repeat(s["T21"], 70, 0)
    n_in = int(run_sim3(s, 4)["counts"][0])
    r = run_sim3(s, n_in)  # count == min_inliers does not accept; identical hypotheses: the last wins
    assert r["first_accept"] == -1 and r["best_at"].tolist() == list(range(70))
    assert run_sim3(s, n_in - 1)["first_accept"] == 0
    assert set(run_sim3(s, 4, best_in=n_in + 1)["best_at"]) == {-2}
    assert run_sim3(s, 4, best_in=n_in)["best_at"].tolist() == list(range(70))


def test_null_outputs():
    lib = _native.hip_lib()
    c = model.pnp_case(130, 5, 7)
    R, t = np.ascontiguousarray(c["R"].reshape(-1, 9)), np.ascontiguousarray(c["t"])
    K = [float(f32(x)) for x in c["K"]]
    p = _native.ptr
    args = (130, p(c["p3d"]), p(c["p2d"]), p(c["sigma2"]), TH2, *K, 5, p(R), p(t), 10, 0)
    _native.check(lib.orb_pnp_check_inliers(*args, None, None, None, None, 0))
    counts = np.zeros(5, np.int32)
    _native.check(lib.orb_pnp_check_inliers(*args, p(counts), None, None, None, 0))
    want = model.pnp(c["p3d"], c["p2d"], c["sigma2"], TH2, c["K"], R, t, 10)
    assert np.array_equal(counts, want["counts"])
    first = ctypes.c_int32(-7)
    _native.check(lib.orb_pnp_check_inliers(*args, None, None, None, ctypes.byref(first), 0))
    assert first.value == want["first_ok"]
    s = model.sim3_case(130, 5, 8)
    a = (130, p(s["x3dc1"]), p(s["x3dc2"]), p(s["sigma2_1"]), p(s["sigma2_2"]), p(s["K1"]), p(s["K2"]), 5, p(s["T12"]),
         p(s["T21"]), 10, 0)
    _native.check(lib.orb_sim3_check_inliers(*a, None, None, None, None, 0))
    best_at = np.zeros(5, np.int32)
    _native.check(lib.orb_sim3_check_inliers(*a, None, None, p(best_at), None, 0))
    want = model.sim3(s["x3dc1"], s["x3dc2"], s["sigma2_1"], s["sigma2_2"], s["K1"], s["K2"], s["T12"], s["T21"], 10)
    assert np.array_equal(best_at, want["best_at"])
    r = orb.Sim3Consensus(s["K1"], s["K2"], 10).check(s["x3dc1"], s["x3dc2"], s["sigma2_1"], s["sigma2_2"], s["T12"],
                                                      s["T21"], want_masks=False)
    assert "masks" not in r and np.array_equal(r["counts"], want["counts"])


def test_refusals():
    def code(fn):
        with pytest.raises(_native.OrbError) as e:
            fn()
        assert str(e.value).split(":", 1)[1].strip(), "a refusal carries a message"
        return e.value.code

    pnp = orb.PnPConsensus(*model.K_TUM, min_inliers=10)
    sim = orb.Sim3Consensus(model.K_TUM, None, 10)
    big, ok = model.pnp_case(8193, 2, 1), model.pnp_case(20, 1025, 2)
    assert code(lambda: pnp.check(big["p3d"], big["p2d"], big["sigma2"], big["R"], big["t"])) == _native.ORB_ENOTSUP
    assert code(lambda: pnp.check(ok["p3d"], ok["p2d"], ok["sigma2"], ok["R"], ok["t"])) == _native.ORB_EINVAL
    assert code(lambda: pnp.check(ok["p3d"], ok["p2d"], ok["sigma2"], ok["R"][:0], ok["t"][:0])) == _native.ORB_EINVAL
    for bad in (np.nan, np.inf, -1.0):
        s2 = ok["sigma2"].copy()
        s2[7] = bad
        assert code(lambda: pnp.check(ok["p3d"], ok["p2d"], s2, ok["R"][:4], ok["t"][:4])) == _native.ORB_EINVAL
    sb, so = model.sim3_case(8193, 2, 3), model.sim3_case(20, 1025, 4)
    a = lambda c, **kw: (c["x3dc1"], c["x3dc2"], kw.get("s1", c["sigma2_1"]), kw.get("s2", c["sigma2_2"]))  # noqa: E731
    assert code(lambda: sim.check(*a(sb), sb["T12"], sb["T21"])) == _native.ORB_ENOTSUP
    assert code(lambda: sim.check(*a(so), so["T12"], so["T21"])) == _native.ORB_EINVAL
    assert code(lambda: sim.check(*a(so), so["T12"][:0], so["T21"][:0])) == _native.ORB_EINVAL
    for bad in (np.nan, np.inf, -1.0, 1.1e18):  # 9.21 * 1.1e18 > 2^63
        s2 = so["sigma2_2"].copy()
        s2[3] = bad
        assert code(lambda: sim.check(*a(so, s2=s2), so["T12"][:4], so["T21"][:4])) == _native.ORB_EINVAL
    s1 = so["sigma2_1"].copy()
    s1[0] = 1e18  # 9.21e18 < 2^63 = 9.22e18: the largest bounds still run
    sim.check(*a(so, s1=s1), so["T12"][:4], so["T21"][:4])


# ---- the batch entry points ---------------------------------------------------------------------------
B, CAP_W, CAP_H, NF = 6, 320, 240, 500
K_SMALL = f32([260, 260, 160, 120])
LS2 = model.LEVEL_SIGMA2


@pytest.fixture(scope="module")
def batch():
    """A 6-frame extractor batch with its FeatureVectors, SearchByBoW rows for every ordered pair in
    both forms, MapPoint positions / bad flags and keyframe poses."""
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
    rng = np.random.default_rng(77)
    cap = int(d_kps.shape[1])
    rows = {}
    for kf_kf in (False, True):
        m, _ = orb.ORBmatcher(0.9, True).search_by_bow_batch_device(kf_kf, d_kps, d_desc, d_cnt, fv, pa, pb)
        rows[kf_kf] = m.cpu().numpy().copy()
    cnt = d_cnt.cpu().numpy()
    kps = d_kps.cpu().numpy().view(_native.KEYPOINT_DTYPE).reshape(B, cap)
    for m in rows.values():
        m[1, :] = -1                                   # an all -1 row
        m[2, 5] = cap + 100                            # beyond every count
        m[2, 9] = int(cnt.max())                       # beyond the keyframe's count, inside the capacity
        m[3, min(cap - 1, int(cnt.max()))] = 0         # an entry at an index past the row's count
    pos = np.stack([rng.uniform(-2, 2, (B, cap)), rng.uniform(-1.5, 1.5, (B, cap)), rng.uniform(2, 8, (B, cap))],
                   2).astype(f32)
    bad = (rng.random((B, cap)) < 0.15).astype(np.uint8)
    pose = np.zeros((B, 12), f32)
    for b in range(B):
        pose[b, :9] = model.rodrigues(rng.normal(0, 0.05, 3)).reshape(9)
        pose[b, 9:] = rng.normal(0, 0.1, 3)
    return {"d_kps": d_kps, "d_cnt": d_cnt, "kps": kps, "cnt": cnt, "cap": cap, "pairs": pairs, "rows": rows,
            "pos": pos, "bad": bad, "pose": pose}


def _solvers(b, S):
    """S solvers cycling over the fixture's pairs."""
    idx = [s % len(b["pairs"]) for s in range(S)]
    return idx, [b["pairs"][i][0] for i in idx], [b["pairs"][i][1] for i in idx]


def _check_rows(out, s, want, n, index, cap, first_key):
    W = (cap + 63) // 64
    assert int(out["n"][s]) == n
    assert np.array_equal(out["index"][s], index), "index list"
    assert np.array_equal(out["counts"][s], want["counts"])
    masks = out["masks"][s].view(np.uint64)
    assert masks.shape[1] == W
    wm = want["masks"].shape[1]
    assert np.array_equal(masks[:, :wm], want["masks"]) and not masks[:, wm:].any()
    assert np.array_equal(out["best_at"][s], want["best_at"])
    assert int(out[first_key][s]) == want[first_key]


@pytest.mark.parametrize("S", [1, 3, 50])
def test_pnp_batch_equals_host_and_model(batch, S):
    import torch

    b, cap, n_hyp = batch, batch["cap"], 70
    idx, kf, fr = _solvers(b, S)
    rng = np.random.default_rng(S)
    rows = b["rows"][False][idx]
    # hypotheses around the identity, from exact to a few pixels off
    amp = 0.0004 * (np.arange(n_hyp) % 35)
    R = np.stack([model.rodrigues(rng.normal(0, amp[h] + 1e-7, 3)) for _ in range(S) for h in range(n_hyp)])
    R = R.reshape(S, n_hyp, 9)
    t = rng.normal(0, 1, (S, n_hyp, 3)) * (2.5 * amp)[None, :, None]
    best_in = rng.integers(0, 3, S).astype(np.int32)
    # MapPoints that the frame sees where the identity pose puts them, so that counts are not all 0
    pos = b["pos"].copy()
    for s in range(S):
        j = np.flatnonzero((rows[s] >= 0) & (rows[s] < b["cnt"][kf[s]]) & (np.arange(cap) < b["cnt"][fr[s]]))
        z = pos[kf[s], rows[s][j], 2]
        pos[kf[s], rows[s][j], 0] = (b["kps"][fr[s]]["x"][j] - K_SMALL[2]) / K_SMALL[0] * z
        pos[kf[s], rows[s][j], 1] = (b["kps"][fr[s]]["y"][j] - K_SMALL[3]) / K_SMALL[1] * z
    cons = orb.PnPConsensus(*K_SMALL, min_inliers=5, th2=TH2)
    tc = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    out = cons.check_batch_device(b["d_kps"], b["d_cnt"], tc(np.int32(kf)), tc(np.int32(fr)), tc(rows), tc(pos),
                                  tc(b["bad"]), LS2, tc(R), tc(t), tc(best_in))
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    seen = set()
    for s in range(S):
        su = model.pnp_setup(b["kps"][fr[s]], b["cnt"][fr[s]], b["cnt"][kf[s]], rows[s], pos[kf[s]], b["bad"][kf[s]], LS2)
        want = model.pnp(su["p3d"], su["p2d"], su["sigma2"], TH2, K_SMALL, R[s], t[s], 5, int(best_in[s]))
        _check_rows(out, s, want, su["n"], su["index"], cap, "first_ok")
        seen.add(su["n"])
        if s < 3:  # the host entry point on the compact arrays
            got = cons.check(su["p3d"], su["p2d"], su["sigma2"], R[s], t[s], int(best_in[s]))
            model.same_result(got, want, "first_ok")
    if S >= 3:
        assert 0 in seen and max(seen) >= 8 and out["counts"].max() >= 5


@pytest.mark.parametrize("S", [1, 3, 50])
def test_sim3_batch_equals_host_and_model(batch, S):
    import torch

    b, cap, n_hyp = batch, batch["cap"], 70
    idx, k1, k2 = _solvers(b, S)
    rng = np.random.default_rng(100 + S)
    rows = b["rows"][True][idx]
    T12 = np.zeros((S, n_hyp, 3, 4), f32)
    T21 = np.zeros((S, n_hyp, 3, 4), f32)
    for s in range(S):
        for h in range(n_hyp):
            e = 0.0004 * (h % 35)  # around the identity, from exact to a few pixels off
            Rr, tt, sc = model.rodrigues(rng.normal(0, e + 1e-7, 3)), rng.normal(0, 2.5 * e + 1e-7, 3), 1 + rng.normal(0, e)
            T12[s, h, :, :3], T12[s, h, :, 3] = sc * Rr, tt
            T21[s, h, :, :3], T21[s, h, :, 3] = Rr.T / sc, -(Rr.T / sc) @ tt
    best_in = rng.integers(0, 3, S).astype(np.int32)
    # the second keyframe's MapPoints where the first one's are (in camera coordinates), so that
    # the near-identity hypotheses find inliers
    pos = b["pos"].copy()
    for s in range(S):
        i1 = np.flatnonzero((rows[s] >= 0) & (rows[s] < b["cnt"][k2[s]]) & (np.arange(cap) < b["cnt"][k1[s]]))
        Ra, ta = b["pose"][k1[s], :9].reshape(3, 3).astype(np.float64), b["pose"][k1[s], 9:].astype(np.float64)
        Rb, tb = b["pose"][k2[s], :9].reshape(3, 3).astype(np.float64), b["pose"][k2[s], 9:].astype(np.float64)
        Xc = pos[k1[s], i1].astype(np.float64) @ Ra.T + ta
        pos[k2[s], rows[s][i1]] = ((Xc - tb) @ Rb).astype(f32)
    cons = orb.Sim3Consensus(K_SMALL, None, 5)
    tc = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    out = cons.check_batch_device(b["d_kps"], b["d_cnt"], tc(np.int32(k1)), tc(np.int32(k2)), tc(rows), tc(pos),
                                  tc(b["bad"]), tc(b["pose"]), LS2, tc(T12), tc(T21), tc(best_in))
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    seen = set()
    for s in range(S):
        su = model.sim3_setup(b["kps"][k1[s]], b["cnt"][k1[s]], b["kps"][k2[s]], b["cnt"][k2[s]], rows[s], pos[k1[s]],
                              b["bad"][k1[s]], pos[k2[s]], b["bad"][k2[s]], b["pose"][k1[s]], b["pose"][k2[s]], LS2)
        a = (su["x3dc1"], su["x3dc2"], su["sigma2_1"], su["sigma2_2"])
        want = model.sim3(*a, K_SMALL, K_SMALL, T12[s], T21[s], 5, int(best_in[s]))
        _check_rows(out, s, want, su["n"], su["index"], cap, "first_accept")
        seen.add(su["n"])
        if s < 3:
            model.same_result(cons.check(*a, T12[s], T21[s], int(best_in[s])), want, "first_accept")
    if S >= 3:
        assert 0 in seen and max(seen) >= 8 and out["counts"].max() >= 5


def test_batch_outputs_may_be_null_and_mp_bad_is_optional(batch):
    import torch

    b, cap = batch, batch["cap"]
    idx, kf, fr = _solvers(b, 3)
    rows = b["rows"][False][idx]
    rng = np.random.default_rng(9)
    R = np.stack([model.rodrigues(rng.normal(0, 0.02, 3)) for _ in range(3 * 4)]).reshape(3, 4, 9)
    t = rng.normal(0, 0.05, (3, 4, 3))
    tc = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d = [tc(np.int32(kf)), tc(np.int32(fr)), tc(rows), tc(b["pos"]), tc(R), tc(t)]
    counts = torch.full((3, 4), -1, dtype=torch.int32, device="cuda")
    p = _native.ptr
    K = [float(x) for x in K_SMALL]
    _native.check(_native.hip_lib().orb_pnp_check_inliers_batch_device(
        p(b["d_kps"]), p(b["d_cnt"]), cap, 3, p(d[0]), p(d[1]), p(d[2]), p(d[3]), None, p(LS2), len(LS2), TH2, *K, 4,
        p(d[4]), p(d[5]), 5, None, None, None, p(counts), None, None, None, None))
    torch.cuda.synchronize()
    for s in range(3):
        su = model.pnp_setup(b["kps"][fr[s]], b["cnt"][fr[s]], b["cnt"][kf[s]], rows[s], b["pos"][kf[s]], None, LS2)
        want = model.pnp(su["p3d"], su["p2d"], su["sigma2"], TH2, K_SMALL, R[s], t[s], 5)
        assert np.array_equal(counts[s].cpu().numpy(), want["counts"])


def test_device_call_then_host_call_without_a_synchronise(batch):
    """The batch form on the default stream, followed at once by a host call: each is complete and
    right on its own."""
    import torch

    b, cap, S, n_hyp = batch, batch["cap"], 50, 300
    idx, kf, fr = _solvers(b, S)
    rows = b["rows"][False][idx]
    rng = np.random.default_rng(21)
    R = np.stack([model.rodrigues(rng.normal(0, 0.02, 3)) for _ in range(S * n_hyp)]).reshape(S, n_hyp, 9)
    t = rng.normal(0, 0.05, (S, n_hyp, 3))
    tc = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d = (tc(np.int32(kf)), tc(np.int32(fr)), tc(rows), tc(b["pos"]), tc(b["bad"]), tc(R), tc(t))
    c = model.pnp_case(1000, 300, 5)
    cons = orb.PnPConsensus(*K_SMALL, min_inliers=5, th2=TH2)
    torch.cuda.synchronize()
    out = cons.check_batch_device(b["d_kps"], b["d_cnt"], d[0], d[1], d[2], d[3], d[4], LS2, d[5], d[6])
    got = orb.PnPConsensus(*c["K"], min_inliers=100).check(c["p3d"], c["p2d"], c["sigma2"], c["R"], c["t"])
    model.same_result(got, model.pnp(c["p3d"], c["p2d"], c["sigma2"], TH2, c["K"], c["R"], c["t"], 100), "first_ok")
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for s in (0, 1, 17, 49):
        su = model.pnp_setup(b["kps"][fr[s]], b["cnt"][fr[s]], b["cnt"][kf[s]], rows[s], b["pos"][kf[s]], b["bad"][kf[s]],
                             LS2)
        want = model.pnp(su["p3d"], su["p2d"], su["sigma2"], TH2, K_SMALL, R[s], t[s], 5)
        _check_rows(out, s, want, su["n"], su["index"], cap, "first_ok")


# ---- the C++ facade -----------------------------------------------------------------------------------
def _fnv(flags):
    h = 2166136261
    for v in flags:
        h = ((h ^ int(bool(v))) * 16777619) & 0xFFFFFFFF
    return h


def test_native_facade(tmp_path):
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge

    exe = ROOT / "build" / "solvers_facade"
    if not exe.exists():
        exe.parent.mkdir(exist_ok=True)
        subprocess.run(ge.SOLVERS_FACADE_CMD(exe), check=True)
    rng = np.random.default_rng(31)
    nk, n_hyp, block, pnp_min, sim3_min = 300, 23, 5, 10, 20
    c = model.pnp_case(nk, n_hyp, 12, K=tuple(float(x) for x in K_SMALL))
    c["R"], c["t"] = c["R"][::-1].copy(), c["t"][::-1].copy()
    kps = np.zeros(nk, _native.KEYPOINT_DTYPE)
    kps["x"], kps["y"] = c["p2d"][:, 0], c["p2d"][:, 1]
    kps["octave"] = rng.integers(0, 8, nk)
    usable = (rng.random(nk) < 0.7).astype(np.uint8)
    s = model.sim3_case(120, n_hyp, 13, K=tuple(float(x) for x in K_SMALL))
    s["T12"], s["T21"] = s["T12"][::-1].copy(), s["T21"][::-1].copy()
    N1 = 400
    idx1 = np.sort(rng.choice(N1, 120, replace=False)).astype(np.int32)
    path = tmp_path / "solvers.bin"
    with open(path, "wb") as f:
        f.write(np.int32([nk, len(LS2), n_hyp, block, pnp_min, 120, N1, sim3_min]).tobytes())
        f.write(K_SMALL.tobytes())
        for a in (kps, LS2.astype(f32), usable, c["p3d"], c["R"].reshape(-1, 9), c["t"], s["x3dc1"], s["x3dc2"],
                  s["sigma2_1"], s["sigma2_2"], idx1, s["T12"].reshape(-1, 12), s["T21"].reshape(-1, 12)):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout + r.stderr
    # the same walk on the model
    su = model.pnp_setup(kps, nk, nk, np.where(usable, np.arange(nk), -1), c["p3d"], None, LS2)
    par = orb.pnp_ransac_parameters(su["n"], 0.99, pnp_min, 300, 4, 0.5, 5.991)
    want = [f"PNP N={su['n']} min={par['min_inliers']} maxits={par['max_iterations']}"]
    best, its, flags = 0, 0, np.zeros(su["n"], bool)
    pa = (su["p3d"], su["p2d"], su["sigma2"], TH2, K_SMALL)
    for h0 in range(0, n_hyp, block):
        m = model.pnp(*pa, c["R"][h0:h0 + block], c["t"][h0:h0 + block], par["min_inliers"], best)
        first = m["first_ok"]
        last = first if first >= 0 else len(m["counts"]) - 1
        its += last + 1
        if m["best_at"][last] >= 0:
            best, flags = int(m["counts"][m["best_at"][last]]), m["inliers"][m["best_at"][last]]
        by_kp = np.zeros(nk, bool)
        by_kp[su["index"][:su["n"]][flags]] = True
        want.append(f"PNP first={first} its={its} best={best} flags={int(by_kp.sum())} hash={_fnv(by_kp):08x}")
    m = model.pnp(*pa, c["R"][:1], c["t"][:1], par["min_inliers"])
    want.append(f"PNP refine count={int(m['counts'][0])} flags={int(m['inliers'][0].sum())} hash={_fnv(m['inliers'][0]):08x}")
    par = orb.sim3_ransac_parameters(120, 0.99, sim3_min, 300)
    want.append(f"SIM3 N=120 min={sim3_min} maxits={par['max_iterations']}")
    best, its = 0, 0
    sa = (s["x3dc1"], s["x3dc2"], s["sigma2_1"], s["sigma2_2"], K_SMALL, K_SMALL)
    for h0 in range(0, n_hyp, block):
        m = model.sim3(*sa, s["T12"][h0:h0 + block], s["T21"][h0:h0 + block], sim3_min, best)
        first = m["first_accept"]
        last = first if first >= 0 else len(m["counts"]) - 1
        its += last + 1
        if m["best_at"][last] >= 0:
            best = int(m["counts"][m["best_at"][last]])
        vb = np.zeros(N1, bool)
        n_in = 0
        if first >= 0:
            vb[idx1[m["inliers"][first]]] = True
            n_in = int(m["counts"][first])
        want.append(f"SIM3 first={first} its={its} best={best} n={n_in} flags={int(vb.sum())} hash={_fnv(vb):08x}")
    want.append("solvers facade OK")
    assert r.stdout.strip().splitlines() == want
    assert any("first=-1" in w for w in want) and any("first=-1" not in w and "first=" in w for w in want)
