"""GPU parity of Optimizer::PoseOptimization (csrc/orb_optimizer.hip: orb_pose_optimization and its
batch form) against the CPU model (tests/native/pose_optimization_model.cpp).

Flags, n_inliers, n_initial, n_bad and rounds are compared exactly, with no edge left out: every
case keeps every classified chi2 at least FLAG_MARGIN from its threshold in the model (asserted),
so the model alone decides each flag.  The f64 pose is compared within POSE_TOL, and the float
pose must be the rounding of the f64 one, bit for bit."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import orbslam_jpminipc_amd as orb
from orbslam_jpminipc_amd import _native
from orbslam_jpminipc_amd.optimizer import INFO_DTYPE
import pose_optimization_model as pom

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
f32 = np.float32
# 100 x the model's own spread over these cases (7.02e-10 in a pose entry between its
# three sum orders and between its -ffp-contract=off and -ffp-contract=fast -mfma builds;
# scripts/gen_pose_optimization_golden.py --spread)
POSE_TOL = 7.0e-8
_worst = {"pose": 0.0}


@pytest.fixture(scope="module")
def cases():
    return pom.host_cases()


@pytest.fixture(scope="module")
def opt():
    return orb.Optimizer(0)


def run_host(opt, c):
    return opt.pose_optimization(c["obs"], c["p3d"], c["has_mp"], pose_in=c["pose_in"], K=c["K"],
                                 inv_sigma2=c["inv_sigma2"])


def same_as_model(got, want, what=""):
    """got: a host-call result (or the same keys from a batch row); want: the model's."""
    assert pom.decisive(want), what
    assert np.array_equal(got["outlier"].astype(np.uint8), want["outlier"]), f"{what}: mvbOutlier differs"
    wi, gi = want["info"], got["info"]
    assert got["n_inliers"] == want["n_inliers"], what
    assert (gi["n_initial"], gi["n_bad"], gi["rounds"]) == (wi.n_initial, wi.n_bad, wi.rounds), what
    assert np.array_equal(got["pose"], got["pose_f64"].astype(f32)), f"{what}: pose_out != float32(pose_out_f64)"
    if np.isfinite(want["pose_f64"]).all():
        dev = float(np.abs(got["pose_f64"] - want["pose_f64"]).max())
        _worst["pose"] = max(_worst["pose"], dev)
        print(f"{what}: pose deviation {dev:.3e} (worst so far {_worst['pose']:.3e}), iterations "
              f"{gi['iterations']} vs {list(wi.iterations)}, trials {gi['trials']} vs {wi.trials}")
        assert dev <= POSE_TOL, f"{what}: pose off by {dev:.3e}"
    else:
        assert np.array_equal(np.isnan(got["pose_f64"]), np.isnan(want["pose_f64"])), what


@pytest.mark.parametrize("n", pom.EDGE_COUNTS)
def test_edge_counts(opt, cases, n):
    c = cases[f"edges_{n}"]
    r = run_host(opt, c)
    same_as_model(r, c["model"], f"edges_{n}")
    assert r["info"]["rounds"] == (1 if n < 10 else 4)
    if n >= 63:
        assert 0 < r["outlier"].sum() < n


@pytest.mark.parametrize("name", ["holes_5_of_2000", "holes_300_of_2000", "holes_257_of_1025"])
def test_has_mp_holes(opt, cases, name):
    c = cases[name]
    r = run_host(opt, c)
    same_as_model(r, c["model"], name)
    assert not r["outlier"][c["has_mp"] == 0].any() and r["info"]["n_initial"] == int(c["has_mp"].sum())


@pytest.mark.parametrize("name", ["outliers_0", "outliers_50", "level_0_only", "behind_camera", "identical_points"])
def test_outlier_shares_levels_and_degenerate_geometry(opt, cases, name):
    c = cases[name]
    same_as_model(run_host(opt, c), c["model"], name)


def test_every_edge_an_outlier_after_round_one(opt, cases):
    c = cases["all_outliers_after_round_1"]
    r = run_host(opt, c)
    same_as_model(r, c["model"], "all_outliers")
    assert r["outlier"].all() and r["n_inliers"] == 0 and r["info"]["rounds"] == 4
    assert r["info"]["iterations"][1:] == [0, 0, 0], "rounds 2-4 have no active edge"
    # the pose is round 1's: the same data as one round (9 edges would stop after it; here the
    # model's own round-1 pose is what the later rounds must not move)
    assert r["info"]["iterations"][0] == c["model"]["info"].iterations[0]


@pytest.mark.parametrize("name", ["z_zero_nan", "z_zero_inf"])
def test_non_finite_chi2(opt, cases, name):
    c = cases[name]
    r = run_host(opt, c)  # status OK
    same_as_model(r, c["model"], name)
    assert not r["outlier"].any() and r["info"]["iterations"] == [10, 10, 7, 5] and r["info"]["trials"] == 32
    assert np.array_equal(r["pose"], c["pose_in"])


def test_chi2_exactly_at_the_threshold_is_an_inlier(opt):
    """Two edges on one point straight ahead of an identity pose, observed one pixel to its left and
    to its right with invSigma2 = 9.210f: their contributions to b cancel exactly in any order, so
    the step is exactly 0, the trial ends where it began (rho == 0: rejected, terminate) and both
    chi2 are 1 * (9.210f * 1) = the round's threshold to the bit.  `>` leaves them inliers
    (Optimizer.cc:261); `>=` would flag both."""
    K = pom.K_DEFAULT
    I12 = np.concatenate([np.eye(3).reshape(9), np.zeros(3)]).astype(f32)
    p3d = f32([[0, 0, 1], [0, 0, 1]])
    obs = f32([[K[2] + 1, K[3]], [K[2] - 1, K[3]]])
    s = f32([9.210, 9.210])
    m = pom.pose_optimization(p3d, obs, s, None, K, I12)
    assert np.array_equal(m["chi2"][0], [float(f32(9.210))] * 2), "the case is built on exact equality"
    r = opt.pose_optimization(obs, p3d, None, pose_in=I12, K=K, inv_sigma2=s)
    assert not r["outlier"].any() and r["n_inliers"] == 2 and r["info"]["n_bad"] == 0
    assert not m["outlier"].any() and m["n_inliers"] == 2
    assert (r["info"]["iterations"], r["info"]["trials"]) == ([1, 0, 0, 0], 1)
    assert np.array_equal(r["pose"], I12)
    # one float above the threshold: both are outliers
    s2 = np.nextafter(s, f32(10))
    r = opt.pose_optimization(obs, p3d, None, pose_in=I12, K=K, inv_sigma2=s2)
    assert r["outlier"].all() and r["n_inliers"] == 0
    assert pom.pose_optimization(p3d, obs, s2, None, K, I12)["outlier"].all()


def test_octave_outside_the_table_is_clamped_by_the_wrapper(opt):
    c = pom.make_case(370, 90, octave_out=True)
    kps = np.zeros(90, _native.KEYPOINT_DTYPE)
    kps["x"], kps["y"], kps["octave"] = c["obs"][:, 0], c["obs"][:, 1], c["octave"]
    r = opt.pose_optimization(kps, c["p3d"], c["has_mp"], pose_in=c["pose_in"], K=c["K"],
                              inv_level_sigma2_=f32(1.0) / pom.LEVEL_SIGMA2)
    same_as_model(r, c["model"], "octave_out")


def test_view_input(opt):
    c = pom.make_case(371, 80)
    kps = np.zeros(80, _native.KEYPOINT_DTYPE)
    kps["x"], kps["y"], kps["octave"] = c["obs"][:, 0], c["obs"][:, 1], c["octave"]
    from orbslam_jpminipc_amd.views import View

    v = View(kps, np.zeros((80, 32), np.uint8), calib=c["K"], Rcw=c["pose_in"][:9], tcw=c["pose_in"][9:],
             scale_factors=np.sqrt(pom.LEVEL_SIGMA2), level_sigma2=pom.LEVEL_SIGMA2)
    r = opt.pose_optimization(v, c["p3d"])
    same_as_model(r, c["model"], "view")
    assert r["Tcw"].shape == (4, 4) and np.array_equal(r["Tcw"][:3, 3], r["pose"][9:])


def test_same_call_twice_gives_the_same_bytes(opt, cases):
    for name in ("edges_1000", "edges_257", "outliers_50"):
        a, b = run_host(opt, cases[name]), run_host(opt, cases[name])
        assert a["pose_f64"].tobytes() == b["pose_f64"].tobytes() and a["outlier"].tobytes() == b["outlier"].tobytes()
        assert a["info"] == b["info"]


def test_staging_reuse_across_sizes(opt, cases):
    """One thread, one context: a small call, one large enough to grow the device arena and the pinned
    staging, a small one again and the empty input, each against the model: a layout that leans on
    what an earlier call left in the staging, or on where the arena was before it grew, fails."""
    seq = [cases["edges_65"], pom.make_case(230, 130), cases["edges_1"], cases["edges_0"]]
    for c in seq:
        same_as_model(run_host(opt, c), c["model"], f"reuse, n = {len(c['obs'])}")


def test_refusals_and_the_call_after(opt, cases):
    def code(fn):
        with pytest.raises(_native.OrbError) as e:
            fn()
        assert str(e.value).split(":", 1)[1].strip(), "a refusal carries a message"
        return e.value.code, str(e.value)

    c = cases["edges_65"]
    big = pom.make_case(1, 8193)
    assert code(lambda: run_host(opt, big))[0] == _native.ORB_ENOTSUP
    for k, bad in ((3, np.nan), (10, np.inf)):
        p = c["pose_in"].copy()
        p[k] = bad
        st, msg = code(lambda: opt.pose_optimization(c["obs"], c["p3d"], None, pose_in=p, K=c["K"],
                                                     inv_sigma2=c["inv_sigma2"]))
        assert st == _native.ORB_EINVAL and "pose_in" in msg
    for K, name in (((0.0, 300, 160, 120), "fx"), ((300, 0.0, 160, 120), "fy"), ((300, 300, np.nan, 120), "cx"),
                    ((300, np.inf, 160, 120), "fy")):
        st, msg = code(lambda: opt.pose_optimization(c["obs"], c["p3d"], None, pose_in=c["pose_in"], K=K,
                                                     inv_sigma2=c["inv_sigma2"]))
        assert st == _native.ORB_EINVAL and name in msg
    same_as_model(run_host(opt, c), c["model"], "served after refusals")


def test_null_outputs(opt, cases):
    c = cases["edges_64"]
    lib, p = _native.hip_lib(), _native.ptr
    pose, outl, n_in = np.zeros(12, f32), np.zeros(64, np.uint8), np.zeros(1, np.int32)
    hm = np.ascontiguousarray(c["has_mp"])
    for has in (p(hm), None):  # has_mp NULL: every keypoint has a MapPoint
        _native.check(lib.orb_pose_optimization(64, p(c["p3d"]), p(c["obs"]), p(c["inv_sigma2"]), has, *c["K"],
                                                p(c["pose_in"]), p(pose), None, p(outl), p(n_in), None, 0))
        assert np.array_equal(pose, run_host(opt, c)["pose"]) and np.array_equal(outl, c["model"]["outlier"])
        assert int(n_in[0]) == c["model"]["n_inliers"]


def test_golden_fixture(opt):
    g = np.load(ROOT / "tests" / "golden" / "pose_optimization_320x240.npz")
    r = opt.pose_optimization(g["obs"], g["p3d"], g["has_mp"], pose_in=g["pose_in"], K=g["K"],
                              inv_sigma2=g["inv_sigma2"])
    assert np.array_equal(r["outlier"].astype(np.uint8), g["outlier"]), "flags differ from the fixture"
    assert r["n_inliers"] == int(g["n_inliers"]) and r["info"]["rounds"] == int(g["rounds"])
    assert r["info"]["n_initial"] == int(g["n_initial"]) and r["info"]["n_bad"] == int(g["n_bad"])
    assert np.abs(r["pose_f64"] - g["pose_f64"]).max() <= POSE_TOL
    # the diagnostics of this one problem: the schedule takes the model's path (iterations and trials)
    # and ends at its lambda, which is re-initialised in every round from max |diag H|
    assert r["info"]["iterations"] == g["iterations"].tolist() and r["info"]["trials"] == int(g["trials"])
    assert abs(r["info"]["lambda"] - float(g["lambda_"])) <= 1e-6 * float(g["lambda_"])
    # the model of this checkout gives the fixture's answer bit for bit
    m = pom.pose_optimization(g["p3d"], g["obs"], g["inv_sigma2"], g["has_mp"], g["K"], g["pose_in"])
    assert np.array_equal(m["pose_f64"], g["pose_f64"]) and np.array_equal(m["outlier"], g["outlier"])


# ---- the batch entry point ----------------------------------------------------------------------------
W, H, NF = 320, 240, 500
K_SMALL = f32([260, 258, 160, 120])
INV_LS2 = (f32(1.0) / pom.LEVEL_SIGMA2).astype(f32)


@pytest.fixture(scope="module")
def batch():
    """3 frames extracted on the device (the third flat: no keypoints) and S = 5 problems over them:
    MapPoints are each frame's own keypoints back-projected under a true pose, with outliers and
    holes; frame 0 is used twice with different start poses, problem 4 is the flat frame."""
    import torch

    frames = np.concatenate([orb.synth_stream(W, H, stream=5, first=0, count=2),
                             orb.synth_special(orb.SYN_FLAT, W, H)[None]])
    ext = orb.ORBextractor(NF, 1.2, 8, orb.FAST_SCORE, 20, device=0, max_batch=3)
    d_kps, _, d_cnt = ext.extract_batch_device(torch.from_numpy(frames).cuda())
    cap = int(d_kps.shape[1])
    kps_h = d_kps.cpu().numpy().view(_native.KEYPOINT_DTYPE).reshape(3, cap).copy()
    cnt = d_cnt.cpu().numpy()
    assert cnt[0] > 64 and cnt[1] > 64 and cnt[2] == 0
    # octaves outside the table in frame 1 (clamped on the device)
    kps_h["octave"][1, 0:cnt[1]:7] = 11
    kps_h["octave"][1, 3:cnt[1]:7] = -2
    d_kps = torch.from_numpy(kps_h.view(np.uint8).reshape(3, cap, 28)).cuda()
    frame_of = np.int32([0, 1, 0, 1, 2])
    S = len(frame_of)
    for seed in range(500, 540):
        rng = np.random.default_rng(seed)
        pos, has, pose_in = np.zeros((S, cap, 3), f32), np.zeros((S, cap), np.uint8), np.zeros((S, 12), f32)
        # garbage past the counts: must be neither read as an edge nor written as a flag
        pos[:] = rng.normal(0, 100, pos.shape)
        has[:] = 1
        want = []
        for s, f in enumerate(frame_of):
            n = int(cnt[f])
            Rt, tt = pom.rot(rng.normal(0, 0.2, 3)), rng.normal(0, 0.5, 3)
            z = rng.uniform(4, 12, n)
            u = kps_h["x"][f, :n] + rng.normal(0, 0.7, n)
            v = kps_h["y"][f, :n] + rng.normal(0, 0.7, n)
            bad = rng.random(n) < 0.2
            u[bad] += rng.uniform(-40, 40, int(bad.sum()))
            Xc = np.stack([(u - K_SMALL[2]) / K_SMALL[0] * z, (v - K_SMALL[3]) / K_SMALL[1] * z, z], 1)
            pos[s, :n] = ((Xc - tt) @ Rt).astype(f32)
            has[s, :n] = rng.random(n) < 0.8
            pose_in[s] = np.concatenate([(pom.rot(rng.normal(0, 0.02, 3)) @ Rt).reshape(9),
                                         tt + rng.normal(0, 0.1, 3)]).astype(f32)
            k = kps_h[f, :n]
            inv = INV_LS2[np.clip(k["octave"], 0, 7)]
            obs = np.stack([k["x"], k["y"]], 1)
            want.append({"obs": obs, "p3d": pos[s, :n].copy(), "has_mp": has[s, :n].copy(), "inv_sigma2": inv,
                         "pose_in": pose_in[s], "K": tuple(K_SMALL), "n": n,
                         "model": pom.pose_optimization(pos[s, :n], obs, inv, has[s, :n], K_SMALL, pose_in[s])})
        if all(pom.decisive(w["model"]) for w in want):
            break
    else:
        raise AssertionError("no decisive seed")
    tc = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return {"d_kps": d_kps, "d_cnt": d_cnt, "cap": cap, "cnt": cnt, "frame_of": frame_of, "want": want,
            "args": (d_kps, d_cnt, tc(frame_of), tc(pos), tc(has), INV_LS2, K_SMALL, tc(pose_in))}


def _row(out, s, n):
    info = out["info"][s].view(INFO_DTYPE)[0]
    return {"pose": out["pose"][s], "pose_f64": out["pose_f64"][s], "outlier": out["outlier"][s, :n].astype(bool),
            "n_inliers": int(out["n_inliers"][s]),
            "info": {"n_initial": int(info["n_initial"]), "n_bad": int(info["n_bad"]), "rounds": int(info["rounds"]),
                     "iterations": info["iterations"].tolist(), "trials": int(info["trials"]),
                     "lambda": float(info["lambda"]), "chi2": float(info["chi2"])}}


def test_batch_equals_host_bitwise_and_model(opt, batch):
    import torch

    out = opt.pose_optimization_batch_device(*batch["args"])
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for s, w in enumerate(batch["want"]):
        got = _row(out, s, w["n"])
        same_as_model(got, w["model"], f"batch problem {s}")
        host = run_host(opt, w)
        assert host["pose_f64"].tobytes() == got["pose_f64"].tobytes(), f"problem {s}: batch != host call"
        assert host["pose"].tobytes() == got["pose"].tobytes() and np.array_equal(host["outlier"], got["outlier"])
        assert host["info"] == got["info"] and host["n_inliers"] == got["n_inliers"]
        assert not out["outlier"][s, w["n"]:].any(), "d_outlier past the count must be 0"
    # one frame, two start poses: two different problems
    assert out["pose_f64"][0].tobytes() != out["pose_f64"][2].tobytes()
    assert out["info"][0].view(INFO_DTYPE)[0]["rounds"] == 4
    # the flat frame: no edge, 0 inliers, the pose is pose_in after the quaternion round trip
    flat = _row(out, 4, 0)
    assert flat["n_inliers"] == 0 and flat["info"]["n_initial"] == 0 and flat["info"]["rounds"] == 1
    assert np.abs(flat["pose_f64"] - batch["want"][4]["pose_in"].astype(np.float64)).max() < 2e-7
    assert np.array_equal(flat["pose_f64"], batch["want"][4]["model"]["pose_f64"])


def test_batch_optional_outputs_may_be_null(opt, batch):
    import torch

    full = opt.pose_optimization_batch_device(*batch["args"])
    lean = opt.pose_optimization_batch_device(*batch["args"], want_f64=False, want_info=False)
    torch.cuda.synchronize()
    assert "pose_f64" not in lean and "info" not in lean
    for k in ("pose", "outlier", "n_inliers"):
        assert torch.equal(full[k], lean[k]), k


def test_batch_refusals(opt, batch):
    a = list(batch["args"])
    with pytest.raises(_native.OrbError) as e:
        opt.pose_optimization_batch_device(*a[:6], f32([0, 258, 160, 120]), a[7])
    assert e.value.code == _native.ORB_EINVAL and "fx" in str(e.value)
    with pytest.raises(_native.OrbError) as e:
        opt.pose_optimization_batch_device(*a[:5], np.ones(17, f32), a[6], a[7])
    assert e.value.code == _native.ORB_EINVAL


def test_cpp_facade(opt, tmp_path):
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge

    exe = ROOT / "build" / "optimizer_facade"
    if not exe.exists():
        exe.parent.mkdir(exist_ok=True)
        subprocess.run(ge.OPTIMIZER_FACADE_CMD(exe), check=True)
    c = pom.make_case(380, 400, edges=300)
    kps = np.zeros(400, _native.KEYPOINT_DTYPE)
    kps["x"], kps["y"], kps["octave"] = c["obs"][:, 0], c["obs"][:, 1], c["octave"]
    path = tmp_path / "optimizer_facade.bin"
    with open(path, "wb") as f:
        f.write(np.int32([400, 8]).tobytes() + f32(c["K"]).tobytes() + c["pose_in"].tobytes() + kps.tobytes() +
                INV_LS2.tobytes() + c["has_mp"].tobytes() + c["p3d"].tobytes())
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FAIL" not in r.stdout and "optimizer facade OK" in r.stdout, r.stdout + r.stderr
    m = c["model"]
    h = 2166136261
    for b in m["outlier"]:
        h = ((h ^ int(b)) * 16777619) & 0xFFFFFFFF
    lines = r.stdout.splitlines()
    assert lines[0] == f"POSEOPT inliers={m['n_inliers']} flags={int(m['outlier'].sum())} hash={h:08x} rounds=4"
    host = run_host(opt, c)
    assert lines[1] == "TCW " + " ".join(f"{int(x):08x}" for x in host["pose"].view(np.uint32))
