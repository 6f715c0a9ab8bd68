"""The CPU model of the Initializer's reconstruction (tests/native/initializer_reconstruct_model.cpp)
proved on its own: cases worked by hand, both acceptance rules at every boundary, the model against
float64 mathematics, the scenes of the golden fixture, and the stand-alone program under the
sanitizers.  No GPU."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import initializer_reconstruct_model as model
import initializer_reconstruct_scenes as scenes

ROOT = pathlib.Path(__file__).resolve().parents[1]
GOLD = dict(np.load(ROOT / "tests" / "golden" / "initializer_reconstruct.npz"))
f32 = np.float32
up = lambda x: np.nextafter(f32(x), f32(np.inf))  # noqa: E731
down = lambda x: np.nextafter(f32(x), f32(-np.inf))  # noqa: E731


# ---- cases worked by hand ----------------------------------------------------------------------

def test_triangulate_closed_form():
    """K = I, P1 = [I|0], P2 = [I|(-1, 0, 0)]: the point (1, 2, 4) is seen at (1/4, 1/2) and (0, 1/2);
    all four coordinates are exact in float32 and the four rows of A vanish on (1, 2, 4, 1)."""
    P1 = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(f32)
    P2 = np.hstack([np.eye(3), [[-1.0], [0.0], [0.0]]]).astype(f32)
    x = model.triangulate([0.25, 0.5], [0.0, 0.5], P1, P2)
    assert np.abs(x - [1, 2, 4]).max() < 4 * 8 * np.finfo(f32).eps  # 8 ulp of the largest coordinate


def test_decompose_e_of_a_chosen_motion():
    R = scenes.rodrigues((0.3, -1.0, 0.2), 0.2)
    t = np.array([0.5, -0.2, 0.1])
    R1, R2, tu = model.decompose_e((scenes.skew(t) @ R).astype(f32))
    assert abs(np.linalg.det(R1.astype(np.float64)) - 1) < 1e-5 and abs(np.linalg.det(R2.astype(np.float64)) - 1) < 1e-5
    assert min(np.abs(R1 - R).max(), np.abs(R2 - R).max()) < 1e-5
    assert min(np.abs(tu - t / np.linalg.norm(t)).max(), np.abs(tu + t / np.linalg.norm(t)).max()) < 1e-5
    assert abs(np.linalg.norm(tu.astype(np.float64)) - 1) < 1e-6
    # the four motions in the reference's order: (R1,t), (R2,t), (R1,-t), (R2,-t)
    n, Rs, ts, _ = model.motions((scenes.skew(t) @ R).astype(f32), False, [1, 1, 0, 0])
    assert n == 4 and np.array_equal(Rs[0], Rs[2]) and np.array_equal(Rs[1], Rs[3]) and not np.array_equal(Rs[0], Rs[1])
    assert np.array_equal(ts[0], ts[1]) and np.array_equal(ts[2], ts[3]) and np.array_equal(ts[2], f32(0) - ts[0])
    assert np.array_equal(Rs[0], R1) and np.array_equal(Rs[1], R2) and np.array_equal(ts[0], tu)


@pytest.mark.parametrize("which", ["d1/d2", "d2/d3"])
def test_h_gate_at_its_threshold(which):
    """K = I and a diagonal H: the decomposition rotates nothing, the singular values are the
    diagonal.  float32(1.00001) lies above the double 1.00001 (the gate lets it pass), the float
    below it lies under (no motion is generated)."""
    edge = f32(1.00001)
    assert float(edge) > 1.00001 > float(down(edge))
    for ratio, want in ((edge, 8), (down(edge), 0)):
        d = (ratio, 1.0, 0.5) if which == "d1/d2" else (2.0, ratio, 1.0)
        n, _, _, sv = model.motions(np.diag(d).astype(f32), True, [1, 1, 0, 0])
        assert np.array_equal(sv, np.array(d, f32)) and n == want


# ---- the acceptance rules on hand-made tables ----------------------------------------------------

def test_rule_f_boundaries():
    P = [2.0] * 4
    assert model.rule_f([90, 0, 0, 0], P, 100) == 0 and model.rule_f([89, 0, 0, 0], P, 100) == -1  # maxGood < nMinGood
    assert model.rule_f([0, 50, 0, 0], P, 10) == 1 and model.rule_f([0, 49, 0, 0], P, 10) == -1  # minTriangulated
    assert model.rule_f([53, 0, 0, 0], P, 59) == 0 and model.rule_f([52, 0, 0, 0], P, 59) == -1  # (int)(0.9 * 59) = 53
    assert model.rule_f([50, 0, 0, 0], P, 55) == 0  # (int)(49.5) = 49, so 50 rules
    assert model.rule_f([0, 0, 100, 70], P, 100) == 2 and model.rule_f([0, 0, 100, 71], P, 100) == -1  # > 0.7 maxGood
    assert model.rule_f([0, 0, 0, 100], [9, 9, 9, 1.0], 100) == -1  # parallax > minParallax is strict
    assert model.rule_f([0, 0, 0, 100], [9, 9, 9, up(1.0)], 100) == 3
    # the else-if chain: the first hypothesis equal to maxGood decides alone (reachable with maxGood = 0)
    assert model.rule_f([0, 0, 0, 0], [0.5, 2, 2, 2], 0, 1.0, 0) == -1 and model.rule_f([0, 0, 0, 0], [2, 0, 0, 0], 0, 1.0, 0) == 0


def test_rule_h_boundaries():
    P = [2.0] * 8
    z = [0] * 6
    assert model.rule_h([100, 74] + z, P, 100) == 0 and model.rule_h([100, 75] + z, P, 100) == -1  # second < 0.75 best
    assert model.rule_h([100, 100] + z, P, 100) == -1  # an equal count is second best (strict >), never best
    assert model.rule_h([60, 100, 70] + z[:5], P, 100) == 1  # best and second best in hypothesis order
    assert model.rule_h([60, 100, 75] + z[:5], P, 100) == -1
    assert model.rule_h([100] + [0] * 7, [1.0] * 8, 100) == 0  # bestParallax >= minParallax
    assert model.rule_h([100] + [0] * 7, [down(1.0)] * 8, 100) == -1
    assert model.rule_h([51] + [0] * 7, P, 50) == 0 and model.rule_h([50] + [0] * 7, P, 50) == -1  # > minTriangulated
    assert model.rule_h([91] + [0] * 7, P, 100) == 0 and model.rule_h([90] + [0] * 7, P, 100) == -1  # > 0.9 N
    assert model.rule_h([0] * 8, P, 0, 1.0, 0) == -1  # nothing counted: bestParallax stays -1


# ---- the model against mathematics ---------------------------------------------------------------

def _closest(R, t, Rs, ts):
    tu = t / np.linalg.norm(t)
    return min(max(np.abs(Rs[k] - R).max(), np.abs(ts[k] - tu).max()) for k in range(len(Rs)))


def test_model_against_float64():
    """20 random motions: the four / eight motions contain the true (R, t/|t|), and 50 noise-free
    triangulations each agree with numpy's SVD of the same float32 inputs.  Largest deviations
    observed: F 5.85e-7, H 4.81e-6, points 6.15e-6 (relative); the bounds are 8 x those.  Points whose
    two smallest singular values are closer than 1e-4 of the largest are left out (0 of 1000 here,
    cap 5 %)."""
    devF = devH = devX = 0.0
    left = total = 0
    K = scenes.K_of()
    for seed in range(20):
        rng = np.random.default_rng(seed)
        R = scenes.rodrigues(rng.normal(size=3), rng.uniform(0.02, 0.1))
        t = rng.normal(size=3) * 0.3
        n, Rs, ts, _ = model.motions(scenes.F_of(R, t), False, scenes.K4)
        assert n == 4
        devF = max(devF, _closest(R, t, Rs[:4].astype(np.float64), ts[:4].astype(np.float64)))
        n, Rs, ts, _ = model.motions(scenes.H_of(R, t, np.array([-0.8, -0.1, 1.0]), 3.0), True, scenes.K4)
        assert n == 8
        devH = max(devH, _closest(R, t, Rs.astype(np.float64), ts.astype(np.float64)))
        X = scenes.volume_points(50, seed)
        P1 = np.hstack([K, np.zeros((3, 1))]).astype(f32)
        P2 = (K @ np.hstack([R, t[:, None]])).astype(f32)
        x1 = scenes.project(X, np.eye(3), np.zeros(3), K).astype(f32)
        x2 = scenes.project(X, R, t, K).astype(f32)
        Q1, Q2 = P1.astype(np.float64), P2.astype(np.float64)
        for i in range(50):
            total += 1
            A = np.stack([x1[i, 0] * Q1[2] - Q1[0], x1[i, 1] * Q1[2] - Q1[1], x2[i, 0] * Q2[2] - Q2[0],
                          x2[i, 1] * Q2[2] - Q2[1]])
            _, s, vt = np.linalg.svd(A)
            if (s[2] - s[3]) / s[0] < 1e-4:
                left += 1
                continue
            ref = vt[3, :3] / vt[3, 3]
            got = model.triangulate(x1[i], x2[i], P1, P2).astype(np.float64)
            devX = max(devX, np.abs(got - ref).max() / np.linalg.norm(ref))
    print(f"F {devF:.3e} H {devH:.3e} points {devX:.3e}, left out {left} of {total}")
    assert left <= 0.05 * total
    assert devF <= 8 * 5.85e-7 and devH <= 8 * 4.81e-6 and devX <= 8 * 6.15e-6


# ---- the scenes and the golden fixture -----------------------------------------------------------

KEYS = ("ok", "R21", "t21", "P3D", "triangulated", "n_motion", "motion_R", "motion_t", "n_good", "cos_parallax",
        "parallax_deg", "best", "n_inliers")


def golden_scene(name):
    return {k[len(name) + 1:]: v for k, v in GOLD.items() if k.startswith(name + ".")}


@pytest.mark.parametrize("name", scenes.SCENE_NAMES)
def test_golden_equals_a_fresh_model_run_and_the_scene_shows_what_it_is_named_for(name):
    g = golden_scene(name)
    s = scenes.scene(name, extra1=17, extra2=9, shuffle=True)
    for k in ("k1", "k2", "m12", "M21"):
        assert np.array_equal(g[k], s[k]), k
    r = model.reconstruct(g["k1"], g["k2"], g["m12"], g["M21"], bool(g["use_h"]), g["mask"], GOLD["K4"])
    for k in KEYS:
        assert model.same_bits(np.asarray(r[k]), g[k]), k
    cnt = np.sort(r["n_good"][:r["n_motion"]])[::-1]
    N = r["n_inliers"]
    if name.startswith("f"):  # one hypothesis takes every point, the others at most 5
        assert r["ok"] and r["n_motion"] == 4 and cnt[0] == N and cnt[1] <= 5 and r["best"] == int(np.argmax(r["n_good"]))
        assert r["parallax_deg"][r["best"]] > 1.0 + float(GOLD["parallax_bound"])
        # the winner is the true motion and the points are the scene's (t21 is a unit vector)
        assert np.abs(r["R21"] - s["R"]).max() < 1e-5
        # depth error z^2 d / (f b): z <= 10, f = 500, b = 0.3, disparity noise d up to 4 sigma sqrt(2) = 1.7 px
        assert np.abs(r["P3D"][g["m12"] >= 0] * np.linalg.norm(s["t"]) - s["X"]).max() < 100 * 1.7 / 150
    else:  # 8 hypotheses; accepted only when the runner-up stays under 0.75 of the best, 5 % clear of it
        assert r["n_motion"] == 8 and cnt[0] == N == 130
        assert abs(cnt[1] - 0.75 * cnt[0]) >= 0.05 * cnt[0]
        assert r["ok"] == (cnt[1] < 0.75 * cnt[0]) == (name == "h_accept")
    # every accept / reject decision holds when acosf moves by one ulp either way, within the recorded bound
    for v in (-1, 1):
        rv = model.reconstruct(g["k1"], g["k2"], g["m12"], g["M21"], bool(g["use_h"]), g["mask"], GOLD["K4"], acos_variant=v)
        assert rv["ok"] == r["ok"] and rv["best"] == r["best"]
        assert 4 * np.abs(rv["parallax_deg"].astype(np.float64) - r["parallax_deg"]).max() <= float(GOLD["parallax_bound"])


def test_counted_but_not_good_points_keep_their_vp3d_entry():
    """CheckRT semantics on a pure rotation: cosParallax >= 0.99998 everywhere, so the depth gates do
    not apply, every point is counted and has its vP3D entry, vbGood stays false and parallax is 0."""
    X = scenes.volume_points(60, 5)
    k1, k2, m12 = scenes.make_pair(X, scenes.R_TRUE, np.zeros(3), noise=0.0, seed=3, extra1=5)
    F = scenes.F_of(scenes.R_TRUE, np.array([0.3, 0.02, 0.03]))
    mask = np.ones(60, np.uint8)
    mask[10:20] = 0  # CheckRT walks all matches and skips the non-inliers
    r = model.reconstruct(k1, k2, m12, F, False, mask, scenes.K4)
    b = int(np.argmax(r["n_good"]))
    idx = np.flatnonzero(m12 >= 0)
    assert r["n_inliers"] == 50 and r["n_good"][b] == 50 and not r["ok"]
    # index min(50, 49) is the largest cosine, which may round above 1: acosf then gives NaN, as in the reference
    assert np.isnan(r["parallax_deg"][b]) or r["parallax_deg"][b] < 0.1
    assert not r["hyp_good"][b].any() and np.array_equal(np.flatnonzero(r["hyp_P3D"][b].any(1)), np.delete(idx, range(10, 20)))
    assert np.float64(r["cos_parallax"][b]) >= 0.99998 and not r["P3D"].any() and r["P3D"].shape == (65, 3)


def test_sanitized_model_program(tmp_path):
    """The model as a stand-alone program under AddressSanitizer and UBSan, on a golden pair."""
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge

    g = golden_scene("h_accept")
    exe = tmp_path / "initializer_reconstruct_model_san"
    subprocess.run(ge.INITIALIZER_RECONSTRUCT_MODEL_CMD(exe, ("-DINITIALIZER_RECONSTRUCT_MODEL_MAIN", "-g",
                                                              "-fsanitize=address,undefined",
                                                              "-fno-sanitize-recover=all")), check=True)
    n1 = len(g["k1"])
    mask = np.zeros(n1, np.uint8)
    mask[: len(g["mask"])] = g["mask"]
    path = tmp_path / "case.bin"
    path.write_bytes(np.array([n1, len(g["k2"]), 1], np.int32).tobytes() + GOLD["K4"].tobytes() + f32(1.0).tobytes() +
                     g["M21"].tobytes() + g["k1"].tobytes() + g["k2"].tobytes() + g["m12"].tobytes() + mask.tobytes())
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "status 0 ok 1 best 1 n_motion 8 N 130" in r.stdout and "ERROR" not in r.stderr, \
        r.stdout + r.stderr
