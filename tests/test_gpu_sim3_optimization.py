"""GPU parity of Optimizer::OptimizeSim3 (csrc/orb_sim3opt.hip: orb_optimize_sim3 and its batch form)
against the CPU model (tests/native/sim3_optimization_model.cpp).

kept, n_inliers, n_correspondences, n_bad and more_iterations are compared exactly, with no slot left
out: every case keeps every classified chi2 at least MARGIN from th2 in the model (asserted), so the
model alone decides each slot.  The f64 Sim3 is compared within SIM3_TOL, and the float Sim3 must be
the rounding of the f64 one, bit for bit."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import orbslam_jpminipc_amd as orb
from orbslam_jpminipc_amd import _native
from orbslam_jpminipc_amd.optimizer import SIM3_INFO_DTYPE
import sim3_optimization_model as s3m

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
f32 = np.float32
# 100 x the model's own spread over these cases (3.17e-7 in a Sim3 entry between its
# three sum orders and between its -ffp-contract=off and -ffp-contract=fast -mfma builds;
# scripts/gen_sim3_optimization_golden.py --spread), rounded down
SIM3_TOL = 3.1e-5
_worst = {"sim3": 0.0}


@pytest.fixture(scope="module")
def cases():
    return s3m.host_cases()


@pytest.fixture(scope="module")
def opt():
    return orb.Optimizer(0)


def run_host(opt, c):
    return opt.optimize_sim3(c["x3dc1"], c["x3dc2"], c["obs1"], c["obs2"], c["inv_sigma2_1"], c["sigma2_2"], c["K1"],
                             c["K2"], c["sim3_in"], th2=c["th2"], usable=c["usable"])


def matrix13(s8) -> np.ndarray:
    """toRotationMatrix, t, s of the f64 output, as the model states Eigen's formula."""
    x, y, z, w = s8[:4]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx,
         1 - (txx + tyy)]
    return np.concatenate([R, s8[4:7], s8[7:8]])


def same_as_model(got, want, what=""):
    """got: a host-call result (or the same keys from a batch row); want: the model's."""
    assert s3m.decisive(want), what
    assert np.array_equal(got["kept"].astype(np.uint8), want["kept"]), f"{what}: the kept slots differ"
    wi, gi = want["info"], got["info"]
    assert got["n_inliers"] == want["n_inliers"], what
    assert (gi["n_correspondences"], gi["n_bad"], gi["more_iterations"]) == \
        (wi.n_correspondences, wi.n_bad, wi.more_iterations), what
    with np.errstate(invalid="ignore", over="ignore"):
        assert np.array_equal(got["sim3"], matrix13(got["sim3_f64"]).astype(f32), equal_nan=True), \
            f"{what}: sim3_out != float32(sim3_out_f64)"
    if np.isfinite(want["sim3_f64"]).all():
        dev = float(np.abs(got["sim3_f64"] - want["sim3_f64"]).max())
        _worst["sim3"] = max(_worst["sim3"], dev)
        print(f"{what}: Sim3 deviation {dev:.3e} (worst so far {_worst['sim3']:.3e}), iterations "
              f"{gi['iterations']} vs {list(wi.iterations)}, trials {gi['trials']} vs {wi.trials}")
        assert dev <= SIM3_TOL, f"{what}: Sim3 off by {dev:.3e}"
    else:
        assert np.array_equal(np.isnan(got["sim3_f64"]), np.isnan(want["sim3_f64"])), what


@pytest.mark.parametrize("n", s3m.PAIR_COUNTS)
def test_pair_counts(opt, cases, n):
    c = cases[f"pairs_{n}"]
    r = run_host(opt, c)
    same_as_model(r, c["model"], f"pairs_{n}")
    assert r["info"]["n_correspondences"] == n
    if n < 10:  # nothing can survive: the result is 0 and the Sim3 is the input's
        assert r["n_inliers"] == 0 and r["info"]["more_iterations"] == 0
        assert np.abs(r["sim3"] - c["sim3_in"]).max() < 2e-7
    if n >= 63:
        assert 0 < r["info"]["n_bad"] < n and r["info"]["more_iterations"] == 10


def test_usable_holes(opt, cases):
    c = cases["holes_300"]
    r = run_host(opt, c)
    same_as_model(r, c["model"], "holes_300")
    assert not r["kept"][c["usable"] == 0].any() and r["info"]["n_correspondences"] == 200


@pytest.mark.parametrize("name", ["outliers_0", "outliers_10", "outliers_45", "octaves", "scale_0.5", "scale_1.0",
                                  "scale_2.0"])
def test_outlier_shares_octaves_and_scales(opt, cases, name):
    c = cases[name]
    r = run_host(opt, c)
    same_as_model(r, c["model"], name)
    if name == "outliers_0":
        assert r["info"]["n_bad"] == 0 and r["info"]["more_iterations"] == 5 and r["kept"].all()
    if name.startswith("scale_"):
        assert abs(r["s"] - float(name[6:])) < 0.02 * float(name[6:])
    if name == "octaves":
        assert set(c["oct1"]) == set(range(8)) and set(c["oct2"]) == set(range(8))


def test_survivor_boundary(opt, cases):
    """20 pairs: 11 removed leave 9 (return 0, the input Sim3, the 11 slots cleared), 10 removed leave
    10 (the second optimisation runs)."""
    c9, c10 = cases["survivors_9"], cases["survivors_10"]
    r9, r10 = run_host(opt, c9), run_host(opt, c10)
    same_as_model(r9, c9["model"], "survivors_9")
    same_as_model(r10, c10["model"], "survivors_10")
    assert r9["info"]["n_bad"] == 11 and r9["n_inliers"] == 0 and r9["info"]["more_iterations"] == 0
    assert int(r9["kept"].sum()) == 9 and r9["info"]["iterations"][1] == 0
    assert np.array_equal(r9["sim3_f64"], s3m.optimize_sim3(*[c9[k] for k in (
        "x3dc1", "x3dc2", "obs1", "obs2", "inv_sigma2_1", "sigma2_2")], np.zeros(20, np.uint8), c9["K1"], c9["K2"],
        c9["th2"], c9["sim3_in"])["sim3_f64"]), "the input Sim3 after the quaternion conversion, to the bit"
    assert r10["info"]["n_bad"] == 10 and r10["n_inliers"] == 10 and r10["info"]["more_iterations"] == 10


def test_update_branches(opt, cases):
    """Started far from the optimum the accepted updates have theta >= 1e-5, started at its float32
    rounding they have theta < 1e-5 (R = I + Omega + Omega^2): the model's branch record."""
    far, near = cases["start_far"], cases["start_near"]
    assert far["model"]["branches"] & 0b1010 and not near["model"]["branches"] & 0b1010
    same_as_model(run_host(opt, far), far["model"], "start_far")
    same_as_model(run_host(opt, near), near["model"], "start_near")


@pytest.mark.parametrize("name", ["z_zero_inf", "nan_pair"])
def test_degenerate_depth_and_nan_pair(opt, cases, name):
    """A point with z = 0 after the map poisons the sums: every trial is rejected, the errors left are
    NaN, a NaN chi2 is not > th2, so every pair stays and counts as an inlier."""
    c = cases[name]
    r = run_host(opt, c)  # status OK
    same_as_model(r, c["model"], name)
    assert r["kept"].all() and r["n_inliers"] == 40 and r["info"]["n_bad"] == 0
    assert r["info"]["iterations"] == [5, 5] and r["info"]["trials"] == 10
    assert np.array_equal(r["sim3"], s3m.IDENTITY13)


def test_chi2_exactly_at_the_threshold_stays(opt):
    """s3m.threshold_case: b is exactly 0 in any summation order, the step is 0, and chi2(e12) of pairs
    0 and 1 equals th2 to the bit.  `>` keeps them (Optimizer.cc:1869, 1903); `>=` would clear both."""
    c = s3m.threshold_case()
    m = s3m.run_case(c)
    assert np.array_equal(m["chi2"][:, 0, :2], np.full((2, 2), float(s3m.TH2))), "the case is built on exact equality"
    assert m["kept"].all() and m["n_inliers"] == 12 and m["info"].n_bad == 0
    r = run_host(opt, c)
    assert r["kept"].all() and r["n_inliers"] == 12 and r["info"]["n_bad"] == 0 and r["info"]["more_iterations"] == 5
    assert (r["info"]["iterations"], r["info"]["trials"]) == ([1, 1], 2)
    assert np.array_equal(r["sim3"], s3m.IDENTITY13)
    # one float above the threshold: both pairs go, 10 are left and the routine goes on
    c2 = s3m.threshold_case(np.nextafter(s3m.TH2, f32(11)))
    r = run_host(opt, c2)
    m2 = s3m.run_case(c2)
    assert not r["kept"][:2].any() and r["kept"][2:].all() and r["info"]["n_bad"] == 2 and r["n_inliers"] == 10
    assert np.array_equal(m2["kept"], r["kept"].astype(np.uint8)) and m2["n_inliers"] == 10
    assert r["info"]["more_iterations"] == 10


def test_same_call_twice_gives_the_same_bytes(opt, cases):
    for name in ("pairs_1000", "pairs_257", "outliers_45"):
        a, b = run_host(opt, cases[name]), run_host(opt, cases[name])
        assert a["sim3_f64"].tobytes() == b["sim3_f64"].tobytes() and a["kept"].tobytes() == b["kept"].tobytes()
        assert a["info"] == b["info"]


def test_staging_reuse_across_sizes(opt, cases):
    """One thread, one context: a small call, one large enough to grow the device arena and the pinned
    staging, a small one again and the empty input, each against the model: a layout that leans on
    what an earlier call left in the staging, or on where the arena was before it grew, fails."""
    seq = [cases["pairs_65"], s3m.make_case(230, 130, outliers=0.1), cases["pairs_1"], cases["pairs_0"]]
    for c in seq:
        same_as_model(run_host(opt, c), c["model"], f"reuse, n = {len(c['x3dc1'])}")


def test_refusals_and_the_call_after(opt, cases):
    def code(fn):
        with pytest.raises(_native.OrbError) as e:
            fn()
        assert str(e.value).split(":", 1)[1].strip(), "a refusal carries a message"
        return e.value.code, str(e.value)

    c = cases["pairs_65"]

    def call(**kw):
        d = dict(c)
        d.update(kw)
        return run_host(opt, d)

    big = {k: (np.zeros((8193,) + np.shape(v)[1:], np.asarray(v).dtype) if k in (
        "x3dc1", "x3dc2", "obs1", "obs2", "inv_sigma2_1", "sigma2_2", "usable") else v) for k, v in c.items()}
    assert code(lambda: run_host(opt, big))[0] == _native.ORB_ENOTSUP
    for k, bad in ((3, np.nan), (10, np.inf), (12, np.nan)):
        p = c["sim3_in"].copy()
        p[k] = bad
        st, msg = code(lambda: call(sim3_in=p))
        assert st == _native.ORB_EINVAL and "sim3_in" in msg
    for which in ("K1", "K2"):
        for K, name in (((0.0, 300, 160, 120), "fx"), ((300, 0.0, 160, 120), "fy"), ((300, 300, np.nan, 120), "cx"),
                        ((300, np.inf, 160, 120), "fy"), ((300, 300, 160, -np.inf), "cy")):
            st, msg = code(lambda: call(**{which: f32(K)}))
            assert st == _native.ORB_EINVAL and name in msg and which in msg
    for th2 in (np.nan, np.inf, -1.0):
        st, msg = code(lambda: call(th2=th2))
        assert st == _native.ORB_EINVAL and "th2" in msg
    same_as_model(run_host(opt, c), c["model"], "served after refusals")


def test_null_outputs(opt, cases):
    c = cases["pairs_64"]
    lib, p = _native.hip_lib(), _native.ptr
    kept = np.zeros(64, np.uint8)
    us = np.ascontiguousarray(c["usable"])
    a = [p(np.ascontiguousarray(c[k])) for k in ("x3dc1", "x3dc2", "obs1", "obs2", "inv_sigma2_1", "sigma2_2")]
    for usable in (p(us), None):  # usable NULL: every slot is usable
        _native.check(lib.orb_optimize_sim3(64, *a, usable, p(c["K1"]), p(c["K2"]), float(c["th2"]), p(c["sim3_in"]),
                                            p(kept), None, None, None, None, 0))
        assert np.array_equal(kept, c["model"]["kept"])
    n_in, o32 = np.zeros(1, np.int32), np.zeros(13, f32)
    _native.check(lib.orb_optimize_sim3(64, *a, None, p(c["K1"]), p(c["K2"]), float(c["th2"]), p(c["sim3_in"]), p(kept),
                                        None, p(o32), p(n_in), None, 0))
    assert int(n_in[0]) == c["model"]["n_inliers"] and np.array_equal(o32, run_host(opt, c)["sim3"])


def test_golden_fixture(opt):
    g = np.load(ROOT / "tests" / "golden" / "sim3_optimization_320x240.npz")
    r = opt.optimize_sim3(g["x3dc1"], g["x3dc2"], g["obs1"], g["obs2"], g["inv_sigma2_1"], g["sigma2_2"], g["K1"],
                          g["K2"], g["sim3_in"], th2=float(g["th2"]), usable=g["usable"])
    assert np.array_equal(r["kept"].astype(np.uint8), g["kept"]), "kept differs from the fixture"
    assert r["n_inliers"] == int(g["n_inliers"]) and r["info"]["n_bad"] == int(g["n_bad"])
    assert r["info"]["n_correspondences"] == int(g["n_correspondences"])
    assert r["info"]["more_iterations"] == int(g["more_iterations"]) == 10
    assert np.abs(r["sim3_f64"] - g["sim3_f64"]).max() <= SIM3_TOL
    # the model of this checkout gives the fixture's answer bit for bit
    m = s3m.optimize_sim3(g["x3dc1"], g["x3dc2"], g["obs1"], g["obs2"], g["inv_sigma2_1"], g["sigma2_2"], g["usable"],
                          g["K1"], g["K2"], g["th2"], g["sim3_in"])
    assert np.array_equal(m["sim3_f64"], g["sim3_f64"]) and np.array_equal(m["kept"], g["kept"])
    assert s3m.decisive(m)


# ---- the batch entry point ----------------------------------------------------------------------------
W, H, NF = 320, 240, 500
K_SMALL = f32([260, 258, 160, 120])
PAIRS = [(0, 1), (0, 2), (2, 1), (1, 3), (3, 0)]  # keyframe 0 in two pairs as the first side; 3 is flat


@pytest.fixture(scope="module")
def batch():
    """4 frames extracted on the device (the fourth flat: no keypoints) and S = 5 candidate pairs.
    Match rows are built on the host as SearchByBoW leaves them (row[i1] = idx2 or -1).  Every
    keyframe's MapPoints are placed so that each pair is consistent with a true Sim3 of its own; the
    two pairs that share keyframe 0 as first side use its even and its odd keypoints.  Rows carry
    entries out of range, garbage past the counts, and some MapPoints are bad."""
    import torch

    frames = np.concatenate([orb.synth_stream(W, H, stream=5, first=0, count=3),
                             orb.synth_special(orb.SYN_FLAT, W, H)[None]])
    ext = orb.ORBextractor(NF, 1.2, 8, orb.FAST_SCORE, 20, device=0, max_batch=4)
    d_kps, _, d_cnt = ext.extract_batch_device(torch.from_numpy(frames).cuda())
    cap = int(d_kps.shape[1])
    kps = d_kps.cpu().numpy().view(_native.KEYPOINT_DTYPE).reshape(4, cap).copy()
    cnt = d_cnt.cpu().numpy()
    assert (cnt[:3] > 64).all() and cnt[3] == 0
    S, B = len(PAIRS), 4
    for seed in range(700, 760):
        rng = np.random.default_rng(seed)
        pos = rng.normal(0, 100, (B, cap, 3)).astype(f32)   # garbage where nothing is placed
        bad = np.zeros((B, cap), np.uint8)
        pose = np.zeros((B, 12), f32)
        for b in range(B):
            pose[b] = np.concatenate([s3m.rot(rng.normal(0, 0.05, 3)).reshape(9), rng.normal(0, 0.1, 3)])
        rows = rng.integers(-50, 2 * cap, (S, cap)).astype(np.int32)  # garbage past the counts
        sim3_in = np.zeros((S, 13), f32)
        placed = np.zeros((B, cap), bool)
        for s, (a, b) in enumerate(PAIRS):
            na, nb = int(cnt[a]), int(cnt[b])
            rows[s, :na] = -1
            if na == 0 or nb == 0:
                sim3_in[s] = s3m.IDENTITY13
                continue
            R12, t12, sc = s3m.rot(rng.normal(0, 0.1, 3)), rng.normal(0, 0.3, 3), float(rng.uniform(0.8, 1.25))
            free_a = np.flatnonzero(~placed[a, :na] & ((np.arange(na) % 2 == s % 2) if a == 0 else True))
            free_b = np.flatnonzero(~placed[b, :nb])
            k = min(len(free_a), len(free_b), 150)
            ia, ib = np.sort(rng.choice(free_a, k, replace=False)), rng.choice(free_b, k, replace=False)
            rows[s, ia] = ib
            placed[a, ia] = placed[b, ib] = True
            # X2c projects where keypoint ia is seen under S12 (e12), X1c where ib is seen under S21 (e21)
            ka, kb = kps[a, ia], kps[b, ib]
            za, zb = rng.uniform(4, 12, k), rng.uniform(4, 12, k)
            ua = ka["x"] + rng.normal(0, 0.5, k)
            ua[rng.random(k) < 0.15] += 40
            va = ka["y"] + rng.normal(0, 0.5, k)
            P1 = np.stack([(ua - K_SMALL[2]) / K_SMALL[0] * za, (va - K_SMALL[3]) / K_SMALL[1] * za, za], 1)
            X2c = ((P1 - t12) @ R12) / sc
            sg = s3m.LEVEL_SIGMA2[np.clip(kb["octave"], 0, 7)].astype(np.float64)
            ub, vb = kb["x"] + rng.normal(0, 0.5, k) / np.sqrt(sg), kb["y"] + rng.normal(0, 0.5, k) / np.sqrt(sg)
            P2 = np.stack([(ub - K_SMALL[2]) / K_SMALL[0] * zb, (vb - K_SMALL[3]) / K_SMALL[1] * zb, zb], 1)
            X1c = sc * (P2 @ R12.T) + t12
            Ra, ta = pose[a, :9].reshape(3, 3).astype(np.float64), pose[a, 9:].astype(np.float64)
            Rb, tb = pose[b, :9].reshape(3, 3).astype(np.float64), pose[b, 9:].astype(np.float64)
            pos[a, ia] = ((X1c - ta) @ Ra).astype(f32)
            pos[b, ib] = ((X2c - tb) @ Rb).astype(f32)
            bad[a, ia[::11]] = 1
            bad[b, ib[5::13]] = 1
            sim3_in[s] = s3m.sim3_13(s3m.rot(rng.normal(0, 0.02, 3)) @ R12, t12 + rng.normal(0, 0.05, 3),
                                     sc * (1 + rng.normal(0, 0.02)))
        # entries out of range inside the counts of row 0
        free0 = np.flatnonzero(rows[0, :cnt[0]] < 0)
        rows[0, free0[0]] = cap + 100          # beyond every count
        rows[0, free0[1]] = int(cnt[1])        # beyond keyframe b's count, inside the capacity
        want = []
        for s, (a, b) in enumerate(PAIRS):
            su = s3m.batch_setup(kps[a], int(cnt[a]), kps[b], int(cnt[b]), rows[s], pos[a], bad[a], pos[b], bad[b],
                                 pose[a], pose[b])
            su.update(K1=K_SMALL, K2=K_SMALL, th2=s3m.TH2, sim3_in=sim3_in[s])
            su["model"] = s3m.run_case(su)
            want.append(su)
        if all(s3m.decisive(w["model"]) for w in want):
            break
    else:
        raise AssertionError("no decisive seed")
    tc = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    pa, pb = np.int32([p[0] for p in PAIRS]), np.int32([p[1] for p in PAIRS])
    return {"cap": cap, "cnt": cnt, "rows": rows, "want": want,
            "args": (d_kps, d_cnt, tc(pa), tc(pb), tc(rows), tc(pos), tc(bad), tc(pose), s3m.LEVEL_SIGMA2, K_SMALL,
                     tc(sim3_in))}


def _row(out, s, n):
    info = out["info"][s].view(SIM3_INFO_DTYPE)[0]
    return {"sim3": out["sim3"][s], "sim3_f64": out["sim3_f64"][s], "n_inliers": int(out["n_inliers"][s]),
            "info": {"n_correspondences": int(info["n_correspondences"]), "n_bad": int(info["n_bad"]),
                     "more_iterations": int(info["more_iterations"]), "iterations": info["iterations"].tolist(),
                     "trials": int(info["trials"]), "lambda": float(info["lambda"]), "chi2": float(info["chi2"])}}


def test_batch_equals_host_bitwise_and_model(opt, batch):
    import torch

    out = opt.optimize_sim3_batch_device(*batch["args"])
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    rows, cap = batch["rows"], batch["cap"]
    for s, w in enumerate(batch["want"]):
        n = len(w["usable"])
        got = _row(out, s, n)
        m = w["model"]
        # the row out: as it came, the cleared slots at -1
        cleared = (w["usable"] == 1) & (m["kept"] == 0)
        expect = rows[s].copy()
        expect[:n][cleared] = -1
        assert np.array_equal(out["match"][s], expect), f"problem {s}: d_match_out"
        got["kept"] = (w["usable"] == 1) & (out["match"][s, :n] >= 0)
        same_as_model(got, m, f"batch problem {s}")
        host = run_host(opt, w)
        assert host["sim3_f64"].tobytes() == got["sim3_f64"].tobytes(), f"problem {s}: batch != host call"
        assert host["sim3"].tobytes() == got["sim3"].tobytes() and np.array_equal(host["kept"], got["kept"])
        assert host["info"] == got["info"] and host["n_inliers"] == got["n_inliers"]
    # keyframe 0 in two pairs: two different problems, both run to the end
    assert out["sim3_f64"][0].tobytes() != out["sim3_f64"][1].tobytes()
    assert all(batch["want"][s]["model"]["info"].more_iterations == 10 for s in (0, 1, 2))
    assert all(batch["want"][s]["model"]["info"].n_bad > 0 for s in (0, 1, 2))
    # the pairs with the flat frame: no correspondence, 0 inliers, the Sim3 is the input's
    for s in (3, 4):
        r = _row(out, s, 0)
        assert r["n_inliers"] == 0 and r["info"]["n_correspondences"] == 0 and r["info"]["more_iterations"] == 0
        assert np.array_equal(r["sim3_f64"], batch["want"][s]["model"]["sim3_f64"])


def test_batch_optional_outputs_may_be_null(opt, batch):
    import torch

    full = opt.optimize_sim3_batch_device(*batch["args"])
    lean = opt.optimize_sim3_batch_device(*batch["args"], want_f64=False, want_info=False)
    a = list(batch["args"])
    nobad = opt.optimize_sim3_batch_device(*a[:6], None, *a[7:])
    torch.cuda.synchronize()
    assert "sim3_f64" not in lean and "info" not in lean
    for k in ("sim3", "match", "n_inliers"):
        assert torch.equal(full[k], lean[k]), k
    # without d_mp_bad more slots are usable
    assert int(nobad["info"][0].cpu().numpy().view(SIM3_INFO_DTYPE)[0]["n_correspondences"]) > \
        batch["want"][0]["model"]["info"].n_correspondences


def test_batch_refusals(opt, batch):
    a = list(batch["args"])
    with pytest.raises(_native.OrbError) as e:
        opt.optimize_sim3_batch_device(*a[:9], f32([0, 258, 160, 120]), a[10])
    assert e.value.code == _native.ORB_EINVAL and "fx" in str(e.value)
    with pytest.raises(_native.OrbError) as e:
        opt.optimize_sim3_batch_device(*a[:8], np.ones(17, f32), a[9], a[10])
    assert e.value.code == _native.ORB_EINVAL
    with pytest.raises(_native.OrbError) as e:
        opt.optimize_sim3_batch_device(*a, th2=-1.0)
    assert e.value.code == _native.ORB_EINVAL and "th2" in str(e.value)
    lib, p = _native.hip_lib(), _native.ptr
    tab = np.ones(8, f32)
    assert lib.orb_optimize_sim3_batch_device(None, None, 8193, 1, None, None, None, None, None, None, p(tab), p(tab), 8,
                                              p(K_SMALL), 10.0, None, None, None, None, None, None,
                                              None) == _native.ORB_ENOTSUP
    assert lib.orb_optimize_sim3_batch_device(None, None, 64, 65536, None, None, None, None, None, None, p(tab), p(tab),
                                              8, p(K_SMALL), 10.0, None, None, None, None, None, None,
                                              None) == _native.ORB_ENOTSUP


def test_cpp_facade(opt, tmp_path):
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge

    exe = ROOT / "build" / "sim3_optimizer_facade"
    if not exe.exists():
        exe.parent.mkdir(exist_ok=True)
        subprocess.run(ge.SIM3_OPTIMIZER_FACADE_CMD(exe), check=True)
    n = 240
    c = s3m.make_case(380, n, usable=(np.arange(n) % 4 != 1), moderate=0.2)
    kps1, kps2 = np.zeros(n, _native.KEYPOINT_DTYPE), np.zeros(n, _native.KEYPOINT_DTYPE)
    perm = np.random.default_rng(380).permutation(n)  # slot i's partner is keypoint perm[i] of KF2
    kps1["x"], kps1["y"], kps1["octave"] = c["obs1"][:, 0], c["obs1"][:, 1], c["oct1"]
    kps2["x"][perm], kps2["y"][perm], kps2["octave"][perm] = c["obs2"][:, 0], c["obs2"][:, 1], c["oct2"]
    matches = np.where(c["usable"] == 1, perm, -1).astype(np.int32)
    path = tmp_path / "sim3_optimizer_facade.bin"
    with open(path, "wb") as f:
        f.write(np.int32([n, n, 8]).tobytes() + f32(c["K1"]).tobytes() + f32(c["K2"]).tobytes() +
                f32([c["th2"]]).tobytes() + c["sim3_in"].tobytes() + kps1.tobytes() + kps2.tobytes() +
                s3m.INV_LEVEL_SIGMA2.tobytes() + s3m.LEVEL_SIGMA2.tobytes() + matches.tobytes() +
                c["x3dc1"].tobytes() + c["x3dc2"].tobytes())
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FAIL" not in r.stdout and "sim3 optimizer facade OK" in r.stdout, r.stdout + r.stderr
    m = c["model"]
    h = 2166136261
    for b in m["kept"]:
        h = ((h ^ int(b)) * 16777619) & 0xFFFFFFFF
    lines = r.stdout.splitlines()
    assert lines[0] == (f"SIM3OPT inliers={m['n_inliers']} matched={int(m['kept'].sum())} hash={h:08x} "
                        f"bad={m['info'].n_bad} more={m['info'].more_iterations}")
    host = run_host(opt, c)
    assert lines[1] == "S12 " + " ".join(f"{int(x):08x}" for x in host["sim3"].view(np.uint32))
