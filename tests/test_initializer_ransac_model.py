"""The CPU model of the Initializer's hypothesis generation (tests/initializer_ransac_model.py,
tests/native/initializer_ransac_model.cpp) proved on its own: the minimal sets against Python and a
replay of the reference's vector, ComputeH21 / ComputeF21 on cases worked by hand and against numpy
float64, and the golden file against a fresh run.  No GPU."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import initializer_model as check_model
import initializer_ransac_model as model
from orbslam_jpminipc_amd._native import KEYPOINT_DTYPE
from orbslam_jpminipc_amd.initializer import initializer_minimal_sets

ROOT = pathlib.Path(__file__).resolve().parents[1]
GOLD = ROOT / "tests" / "golden"
f32 = np.float32

# Measured maxima of the float32 model against numpy float64 on the 400 sets below (printed by the
# two tests; DESIGN.md §16 records them); each test's bound is 8 x its maximum.  They bound the
# model against mathematics, never the kernel against the model (that comparison is exact).
H_MAX_DEV, F_MAX_DEV = 5.19e-7, 1.79e-5


# ---- helpers shared with tests/test_gpu_initializer_ransac.py ----------------------------------

def kps_of(xy):
    k = np.zeros(len(xy), KEYPOINT_DTYPE)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["size"], k["angle"], k["class_id"] = 31.0, -1.0, -1
    return k


def two_view_scene(n_pts, seed, noise=0.5, planar_share=0.0):
    """n_pts points at depth 2-10 seen by two cameras (500 px focal length, baseline about 0.3, a
    small rotation), pixel noise `noise`: (n, 2) float64 image points of each view."""
    rng = np.random.default_rng(seed)
    Z = rng.uniform(2, 10, n_pts)
    npl = int(planar_share * n_pts)
    Z[:npl] = 6.0
    X = np.stack([rng.uniform(-0.3, 0.3, n_pts) * Z, rng.uniform(-0.22, 0.22, n_pts) * Z, Z], 1)
    a = 0.03
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([0.3, 0.02, 0.01])
    X2 = X @ R.T + t
    x1 = 500 * X[:, :2] / X[:, 2:] + [160, 120] + rng.normal(0, noise, (n_pts, 2))
    x2 = 500 * X2[:, :2] / X2[:, 2:] + [160, 120] + rng.normal(0, noise, (n_pts, 2))
    return x1, x2


def two_view_case(N, n1=None, n2=None, seed=0, planar_share=0.5):
    """A pair with N matches among n1 / n2 keypoints (holes of -1, frame-2 indices shuffled, the
    unmatched keypoints anywhere in the image so that Normalize sees them): half the scene on a
    plane, so that both a homography and a fundamental matrix find inliers."""
    rng = np.random.default_rng(77 * N + seed)
    n1 = n1 if n1 is not None else N + N // 3 + 2
    n2 = n2 if n2 is not None else N + 4
    x1, x2 = two_view_scene(N, 1000 + N + seed, planar_share=planar_share)
    k1 = (rng.random((n1, 2)) * [320, 240]).astype(f32)
    k2 = (rng.random((n2, 2)) * [320, 240]).astype(f32)
    m12 = np.full(n1, -1, np.int32)
    src = np.sort(rng.choice(n1, N, replace=False))
    dst = rng.choice(n2, N, replace=False)
    m12[src] = dst
    k1[src] = x1.astype(f32)
    k2[dst] = x2.astype(f32)
    return kps_of(k1), kps_of(k2), m12


def draws(n_hyp, seed):
    return np.random.default_rng(seed).integers(0, 1 << 31, (n_hyp, 8), dtype=np.int64).astype(np.int32)


def draw_for(position, size):
    """A rand() value whose RandomInt(0, size - 1) is `position`."""
    r = -(-(position << 31) // size)
    assert (r * size) >> 31 == position
    return r


def replay_sets(N, rand31):
    """Initializer.cc:80-95 with a Python list, the double expression of Random.cpp:47-50; also
    which sets drew a position that an earlier removal had written."""
    sets, moved = [], []
    for row in np.asarray(rand31, np.int64).reshape(-1, 8):
        avail, written, hit, s = list(range(N)), set(), False, []
        for r in row:
            randi = int((float(r) / (2147483647.0 + 1.0)) * len(avail))
            hit |= randi in written
            s.append(avail[randi])
            avail[randi] = avail[-1]
            written.add(randi)
            avail.pop()
        sets.append(s)
        moved.append(hit)
    return np.array(sets, np.int32), np.array(moved)


# ---- the sets ------------------------------------------------------------------------------------

def test_sets_python_cpp_and_replay_agree():
    for N, seed in ((8, 1), (9, 2), (100, 3), (8192, 4)):
        r = draws(64 if N < 8192 else 4, seed)
        want, _ = replay_sets(N, r)
        assert np.array_equal(model.minimal_sets(N, r), want)
        assert np.array_equal(initializer_minimal_sets(N, r), want)
        assert all(len(set(s)) == 8 and max(s) < N for s in want.tolist())


def test_sets_by_hand_a_moved_entry_is_drawn_again():
    # N = 8, every draw lands on position 0, which after the first removal holds the moved back()
    r = np.zeros((1, 8), np.int32)
    want = [[0, 7, 6, 5, 4, 3, 2, 1]]
    assert model.minimal_sets(8, r).tolist() == want and initializer_minimal_sets(8, r).tolist() == want
    # the last position every time: nothing moves
    r = np.array([[draw_for(7 - j, 8 - j) for j in range(8)]], np.int32)
    want = [[7, 6, 5, 4, 3, 2, 1, 0]]
    assert model.minimal_sets(8, r).tolist() == want and initializer_minimal_sets(8, r).tolist() == want
    # N = 10: position 2 (2; 9 moves in), 2 again (9; 8 moves in), 7 (the back itself), 2 again (8)
    r = np.array([[draw_for(2, 10), draw_for(2, 9), draw_for(7, 8), draw_for(2, 7), 0, 0, 0, 0]], np.int32)
    got = model.minimal_sets(10, r).tolist()[0]
    assert got[:4] == [2, 9, 7, 8] and got == initializer_minimal_sets(10, r).tolist()[0] == replay_sets(10, r)[0][0].tolist()
    # a sampler that removes by value (the Sim3Solver's quirk) would differ
    assert replay_sets(10, r)[1][0]


def test_shift_equals_the_double_expression():
    rng = np.random.default_rng(5)
    sizes = [1, 2, 3, 7, 8, 9, 100, 1000, 4095, 4096, 4097, 8191, 8192]
    for size in sizes:
        ks = set(range(0, min(size, 40))) | set(rng.integers(0, size, 40).tolist()) | {size - 1}
        rs = {0, (1 << 31) - 1}
        for k in ks:
            c = -(-(k << 31) // size)
            rs |= {c - 1, c, c + 1}
        for r in rs:
            if 0 <= r < 1 << 31:
                assert (r * size) >> 31 == int((float(r) / (2147483647.0 + 1.0)) * size), (r, size)


def test_refusals_of_the_model():
    with pytest.raises(ValueError):
        model.minimal_sets(7, np.zeros((1, 8), np.int32))
    with pytest.raises(ValueError):
        model.minimal_sets(8, np.full((1, 8), -1, np.int32))
    with pytest.raises(ValueError):
        initializer_minimal_sets(7, np.zeros((1, 8), np.int32))


# ---- worked by hand ------------------------------------------------------------------------------

def test_rng_signs():
    """cv::RNG(0x12345678): bit 8 of the first nine draws, the signs of the row ComputeF21's F is
    made from (when no earlier row was degenerate)."""
    state, want = 0x12345678, []
    for _ in range(9):
        state = (state & 0xFFFFFFFF) * 4164903690 + (state >> 32)
        want.append(1 if state & 256 else -1)
    x1, x2 = two_view_scene(8, 3, noise=0.0)
    _, _, _, sg = model.compute((x1 - 160) / 100, (x2 - 160) / 100)
    print("signs", sg.tolist())
    assert sg.tolist() == want == [-1, -1, 1, -1, -1, -1, -1, 1, 1]


def test_identical_first_two_correspondences_consume_draws():
    """Rows 0 and 1 of ComputeF21's matrix identical: the first rotation (c == s) leaves row 1
    exactly zero, nothing rotates it again, the sort puts it last among the 8 and the fill-in
    takes nine draws for it before the nine of the row F is made from."""
    x1, x2 = two_view_scene(8, 5, noise=0.0)
    p1, p2 = ((x1 - [160, 120]) / 100).astype(f32), ((x2 - [160, 120]) / 100).astype(f32)
    p1[1], p2[1] = p1[0], p2[0]
    _, Fn, Fpre, sg = model.compute(p1, p2)
    assert len(sg) == 18 and not np.isnan(Fn).any()
    h1, h2 = np.c_[p1.astype(np.float64), np.ones(8)], np.c_[p2.astype(np.float64), np.ones(8)]
    assert np.abs(np.einsum("ni,ij,nj->n", h2, Fpre.astype(np.float64), h1)).max() < 1e-4


def test_exact_homography():
    p1 = np.array([[0, 0], [1, 0], [0, 1], [1, 1], [2, 1], [1, 2], [-1, 1], [-2, -1]], f32)
    Ht = np.array([[2, 0, 1], [0, 2, -1], [0, 0, 1]], np.float64)
    q = np.c_[p1.astype(np.float64), np.ones(8)] @ Ht.T
    p2 = (q[:, :2] / q[:, 2:]).astype(f32)
    Hn, _, _, _ = model.compute(p1, p2)
    Hn = Hn.astype(np.float64) / Hn[2, 2]
    assert np.abs(Hn - Ht).max() < 1e-5, Hn
    # a projective one, exactly representable points
    Ht = np.array([[1, 0.5, 0], [0, 1, 0.25], [0.25, 0, 1]], np.float64)
    p1 = np.array([[0, 0], [4, 0], [0, 4], [4, 4], [-2, 4], [4, -2], [12, 4], [-2, -2]], f32)
    q = np.c_[p1.astype(np.float64), np.ones(8)] @ Ht.T
    p2 = (q[:, :2] / q[:, 2:]).astype(f32)
    assert np.array_equal(p2.astype(np.float64), q[:, :2] / q[:, 2:])
    Hn, _, _, _ = model.compute(p1, p2)
    Hn = Hn.astype(np.float64) / Hn[2, 2]
    assert np.abs(Hn - Ht).max() < 1e-4, Hn


def test_two_view_fundamental_is_rank_two_by_construction():
    x1, x2 = two_view_scene(8, 11, noise=0.0)
    p2 = ((x2 - [160, 120]) / 100).astype(f32)
    p1 = ((x1 - [160, 120]) / 100).astype(f32)
    _, Fn, Fpre, _ = model.compute(p1, p2)
    h1 = np.c_[p1.astype(np.float64), np.ones(8)]
    h2 = np.c_[p2.astype(np.float64), np.ones(8)]
    for F in (Fpre, Fn):
        res = np.abs(np.einsum("ni,ij,nj->n", h2, F.astype(np.float64), h1)).max()
        assert res < 1e-4, res
    # F = u * diag(w0, w1, 0) * vt of the model's own decomposition of Fpre, product by product
    w, u, vt = model.svd(Fpre)
    assert w[0] >= w[1] >= w[2] >= 0
    D = np.diag(np.array([w[0], w[1], 0], f32))
    assert model.mul3(model.mul3(u, D), vt).tobytes() == Fn.tobytes()
    assert abs(np.linalg.det(Fn.astype(np.float64))) < 1e-9
    s = np.linalg.svd(Fn.astype(np.float64), compute_uv=False)
    assert s[2] < 1e-7 * s[0]


def test_svd_reconstructs_and_sorts():
    rng = np.random.default_rng(9)
    for shape in ((16, 9), (8, 9), (3, 3)):
        A = rng.normal(0, 1, shape).astype(f32)
        w, u, vt = model.svd(A)
        assert np.all(np.diff(w) <= 0)
        assert np.allclose(w, np.linalg.svd(A.astype(np.float64), compute_uv=False), atol=1e-5)
        assert np.abs(vt.astype(np.float64) @ vt.T - np.eye(shape[1])).max() < 1e-5  # the filled-in row included
        if shape == (3, 3):
            assert np.abs(u.astype(np.float64) @ np.diag(w) @ vt - A).max() < 1e-5


def test_inv3():
    assert not model.inv3(np.array([[1, 2, 3], [2, 4, 6], [0, 1, 5]], f32)).any()  # det == 0: zeros
    assert not model.inv3(np.zeros((3, 3), f32)).any()
    assert np.array_equal(model.inv3(np.diag([2, 4, 8]).astype(f32)), np.diag([0.5, 0.25, 0.125]).astype(f32))
    S = np.array([[2, 0, 1], [0, 3, -1], [0, 0, 1]], f32)
    assert np.abs(model.inv3(S).astype(np.float64) @ S - np.eye(3)).max() < 1e-6
    assert np.isnan(model.inv3(np.full((3, 3), np.nan, f32))).all()


def test_normalize_and_degenerate_frames():
    k1, k2, m12 = two_view_case(20, seed=1)
    h = model.hypotheses(k1, k2, m12, rand31=draws(4, 1))
    x = check_model.xy(k1).astype(np.float64)
    mean = x.mean(0)
    dev = np.abs(x - mean).mean(0)
    want = np.array([[1 / dev[0], 0, -mean[0] / dev[0]], [0, 1 / dev[1], -mean[1] / dev[1]], [0, 0, 1]])
    assert np.allclose(h["T1"], want, rtol=1e-5)
    # fewer than 8 matches: nothing is generated
    m7 = m12.copy()
    m7[np.flatnonzero(m7 >= 0)[7:]] = -1
    h = model.hypotheses(k1, k2, m7, rand31=draws(4, 1))
    assert h["n_matches"] == 7 and not any(h[k].any() for k in model.HYP_KEYS) and not h["sets"].any()
    r = model.find(k1, k2, m7, draws(4, 1))
    assert r["best_h"] == r["best_f"] == -1 and r["best_score_h"] == 0 and np.isnan(r["RH"]) and not r["use_h"]
    assert np.isnan(r["H"]).all() and not r["inliers_h"].any()
    # zero deviation in x: sX is inf, the NaN flows on
    kz = k2.copy()
    kz["x"] = 100.0
    with np.errstate(all="ignore"):
        h = model.hypotheses(k1, kz, m12, rand31=draws(4, 1))
    assert np.isinf(h["T2"][0, 0]) and np.isnan(h["H21"]).any()


# ---- against numpy float64 -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene_sets():
    x1, x2 = two_view_scene(200, 2024)

    def norm(x):
        m = x.mean(0)
        return ((x - m) / np.abs(x - m).mean(0)).astype(f32)

    p1, p2 = norm(x1), norm(x2)
    rng = np.random.default_rng(6)
    out = []
    for _ in range(400):
        s = rng.choice(200, 8, replace=False)
        Hn, _, Fpre, _ = model.compute(p1[s], p2[s])
        out.append((p1[s].astype(np.float64), p2[s].astype(np.float64), Hn, Fpre))
    return out


def _align(v, ref):
    v = v.reshape(9).astype(np.float64)
    return v if v @ ref >= 0 else -v


def test_homography_against_numpy_float64(scene_sets):
    dev, skipped = 0.0, 0
    for a, b, Hn, _ in scene_sets:
        A = np.zeros((16, 9))
        for i in range(8):
            u1, v1, u2, v2 = a[i, 0], a[i, 1], b[i, 0], b[i, 1]
            A[2 * i] = [0, 0, 0, -u1, -v1, -1, v2 * u1, v2 * v1, v2]
            A[2 * i + 1] = [u1, v1, 1, 0, 0, 0, -u2 * u1, -u2 * v1, -u2]
        _, s, vt = np.linalg.svd(A)
        if (s[7] - s[8]) / s[0] < 1e-2:
            skipped += 1
            continue
        dev = max(dev, np.abs(_align(Hn, vt[8]) - vt[8]).max())
    print(f"H: max deviation {dev:.3e}, skipped {skipped} of 400")
    assert skipped <= 20
    assert dev <= 8 * H_MAX_DEV


def test_fundamental_against_numpy_float64(scene_sets):
    dev, skipped = 0.0, 0
    for a, b, _, Fpre in scene_sets:
        A = np.zeros((8, 9))
        for i in range(8):
            u1, v1, u2, v2 = a[i, 0], a[i, 1], b[i, 0], b[i, 1]
            A[i] = [u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1]
        _, s, vt = np.linalg.svd(A)
        if s[7] / s[0] < 1e-4:
            skipped += 1
            continue
        dev = max(dev, np.abs(_align(Fpre, vt[8]) - vt[8]).max())
    print(f"F: max deviation {dev:.3e}, skipped {skipped} of 400")
    assert skipped <= 20
    assert dev <= 8 * F_MAX_DEV


# ---- the golden file -------------------------------------------------------------------------------

def golden():
    from test_initializer_model import golden_inputs

    k1, k2, m12, _ = golden_inputs()
    return k1, k2, m12, dict(np.load(GOLD / "initializer_ransac_320x240.npz"))


def golden_as_result(g) -> dict:
    r = {k: g[k] for k in ("H21", "H12", "F21", "sets", "scores_h", "scores_f", "inliers_h", "inliers_f", "H", "F")}
    r.update(n_matches=int(g["n_matches"]), best_h=int(g["best_h"]), best_f=int(g["best_f"]),
             best_score_h=f32(g["best_score_h"]), best_score_f=f32(g["best_score_f"]), RH=f32(g["RH"]),
             use_h=bool(g["use_h"]))
    return r


def same_find(got, want):
    """Asserts that two find() results agree: floats bit for bit (NaN as "is NaN")."""
    check_model.same_result(got, want)
    for k in ("H21", "H12", "F21", "sets", "H", "F"):
        assert model.same_bits(np.asarray(got[k]).reshape(np.asarray(want[k]).shape), want[k]), k
    assert model.same_bits(f32(got["RH"]), f32(want["RH"])), (got["RH"], want["RH"])
    assert bool(got["use_h"]) == bool(want["use_h"])


def test_golden_equals_a_fresh_model_run():
    k1, k2, m12, g = golden()
    r = model.find(k1, k2, m12, g["rand31"], float(g["sigma"]))
    same_find(r, golden_as_result(g))
    assert g["rand31"].shape == (200, 8) and r["best_h"] >= 0 and r["best_f"] >= 0
    assert replay_sets(r["n_matches"], g["rand31"])[1].sum() >= 8


def test_sanitized_model_program(tmp_path):
    """The model as a stand-alone program under AddressSanitizer and UBSan, on the golden pair."""
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge

    k1, k2, m12, g = golden()
    exe = tmp_path / "initializer_ransac_model_san"
    subprocess.run(ge.INITIALIZER_RANSAC_MODEL_CMD(exe, ("-DINITIALIZER_RANSAC_MODEL_MAIN", "-g",
                                                         "-fsanitize=address,undefined",
                                                         "-fno-sanitize-recover=all")), check=True)
    path = tmp_path / "case.bin"
    path.write_bytes(np.array([len(k1), len(k2), 200], np.int32).tobytes() + check_model.xy(k1).tobytes() +
                     check_model.xy(k2).tobytes() + np.asarray(m12, np.int32).tobytes() + g["rand31"].tobytes())
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "status 0" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr
