"""The CPU model of the Sim3Solver hypotheses (tests/native/sim3_solver_model.cpp) on cases worked by
hand: the sampler with its removal quirk, cv::eigen's Jacobi, computeT against an independent
float64 Horn solution, the degenerate sets and the iterate bookkeeping.  No GPU."""
import numpy as np

import orbslam_jpminipc_amd as orb
import sim3_solver_model as s3
import solvers_model

f32 = np.float32
K = np.asarray(solvers_model.K_TUM, f32)


def r_for(randi, size):
    """A rand() value whose RandomInt(0, size - 1) is randi (the middle of its interval)."""
    return (randi * 2 ** 31 + 2 ** 30) // size


# ---- the sampler -------------------------------------------------------------------------------------
def test_sampler_n3_every_position():
    want = {(0, 0, 0): (0, 2, 2), (0, 1, 0): (0, 1, 2), (1, 0, 0): (1, 0, 2), (1, 1, 0): (1, 2, 0),
            (2, 0, 0): (2, 0, 1), (2, 1, 0): (2, 1, 0)}
    # worked by hand, e.g. (0, 0, 0): [0 1 2] draws 0, [0] = 2 -> [2 1 2]; position 0 draws 2,
    # [2] = [1] -> [2 1 1]; position 0 draws 2 again.  (1, 1, 0): draws 1, [1] = 2 -> [0 2 2]; position
    # 1 draws 2, [2] = [1] = 2; position 0 draws 0.
    for randi, idx in want.items():
        r = [[r_for(randi[0], 3), r_for(randi[1], 2), r_for(randi[2], 1)]]
        assert tuple(s3.sets(3, r)[0]) == idx, randi
        assert tuple(orb.sim3_minimal_sets(3, r)[0]) == idx, randi
    # the third draw is forced: any value maps to position 0
    assert tuple(s3.sets(3, [[0, 0, 2 ** 31 - 1]])[0]) == (0, 2, 2)


def test_sampler_n5_repeated_index_and_fixed_variant():
    r = 751619276  # 0.35 * 2^31: position 1 of 5, of 4 and of 3
    assert [(r * d) >> 31 for d in (5, 4, 3)] == [1, 1, 1]
    # [0 1 2 3 4] draws 1, [1] = 4 -> [0 4 2 3 4]; position 1 draws 4, [4] = [3] -> [0 4 2 3 3];
    # position 1 draws 4 again
    assert s3.sets(5, [[r, r, r]]).tolist() == [[1, 4, 4]]
    assert orb.sim3_minimal_sets(5, [[r, r, r]]).tolist() == [[1, 4, 4]]
    # removing by position: [0 4 2 3], [0 3 2]: the third draw is 3
    assert s3.sets(5, [[r, r, r]], s3.FIXED_SAMPLER).tolist() == [[1, 4, 3]]
    assert orb.sim3_minimal_sets(5, [[r, r, r]], fixed=True).tolist() == [[1, 4, 3]]


def test_sampler_python_restatement_equals_model():
    rng = np.random.default_rng(5)
    for N in (3, 4, 5, 63, 64, 65, 200, 8192):
        r = rng.integers(0, 2 ** 31, (500, 3))
        r[0], r[1] = 0, 2 ** 31 - 1
        a, b = s3.sets(N, r), orb.sim3_minimal_sets(N, r)
        assert np.array_equal(a, b) and a.min() >= 0 and a.max() < N
        assert np.array_equal(s3.sets(N, r, s3.FIXED_SAMPLER), orb.sim3_minimal_sets(N, r, fixed=True))


def test_random_int_shift_equals_the_double_expression():
    rng = np.random.default_rng(6)
    rs = [0, 1, 2 ** 31 - 1, 2 ** 30] + rng.integers(0, 2 ** 31, 2000).tolist()
    for d in (1, 2, 3, 8191, 8192):
        for r in rs:
            assert s3.random_int(r, d) == (r * d) >> 31, (r, d)


# ---- cv::eigen ---------------------------------------------------------------------------------------
def test_jacobi_diagonal_is_sorted_with_its_rows():
    W, V = s3.jacobi(np.diag(f32([2, -1, 7, 3])))
    assert W.tolist() == [7, 3, 2, -1]
    assert np.array_equal(V, np.eye(4, dtype=f32)[[2, 3, 0, 1]])


def test_jacobi_block_matrix():
    A = np.zeros((4, 4), f32)
    A[:2, :2] = [[2, 1], [1, 2]]      # eigenpairs 3: (1, 1)/sqrt2, 1: (1, -1)/sqrt2
    A[2:, 2:] = [[5, 2], [2, 5]]      # 7: (1, 1)/sqrt2, 3: (1, -1)/sqrt2
    W, V = s3.jacobi(A)
    assert np.allclose(W, [7, 3, 3, 1], atol=1e-6)
    h = np.sqrt(0.5)
    assert np.allclose(np.abs(V[0]), [0, 0, h, h], atol=1e-6) and V[0, 2] * V[0, 3] > 0
    assert np.allclose(np.abs(V[3]), [h, h, 0, 0], atol=1e-6) and V[3, 0] * V[3, 1] < 0


def test_jacobi_random_symmetric():
    rng = np.random.default_rng(7)
    for _ in range(200):
        B = rng.normal(0, 1, (4, 4))
        A = ((B + B.T) / 2).astype(f32)
        W, V = s3.jacobi(A)
        assert np.all(np.diff(W) <= 0)
        Vd, Ad = V.astype(np.float64), A.astype(np.float64)
        scale = np.abs(Ad).max()
        assert np.abs(Vd @ Vd.T - np.eye(4)).max() < 2e-6
        assert np.abs(Vd @ Ad @ Vd.T - np.diag(W.astype(np.float64))).max() < 4e-6 * scale
        assert np.allclose(W, np.linalg.eigvalsh(Ad)[::-1], atol=4e-6 * scale)


# ---- computeT against float64 ------------------------------------------------------------------------
# The largest float32-against-float64 deviation this test measures on its kept sets (seed 11, 400
# sets), and the bound at 8 x that.
MEASURED = {"R": 3.01e-6, "t": 3.10e-5, "s": 1.25e-7}
BOUND = {k: 8 * v for k, v in MEASURED.items()}


def test_compute_t_against_numpy_float64(capsys):
    c = s3.cloud(200, seed=1, scale=1.7, angle=0.4, noise=0.01)
    rng = np.random.default_rng(11)
    sets = s3.sets(200, rng.integers(0, 2 ** 31, (400, 3)))
    m = s3.compute(c["x3dc1"], c["x3dc2"], sets)
    dev = {"R": 0.0, "t": 0.0, "s": 0.0}
    left_out = 0
    for h, st in enumerate(sets):
        R, t, s, gap = s3.horn_f64(c["x3dc1"][st].T, c["x3dc2"][st].T)
        if not gap >= 1e-2:
            left_out += 1
            continue
        got = m["sim3"][h].astype(np.float64)
        dev["R"] = max(dev["R"], np.abs(got[:9].reshape(3, 3) - R).max())
        dev["t"] = max(dev["t"], np.abs(got[9:12] - t).max())
        dev["s"] = max(dev["s"], abs(got[12] - s) / s)
        sR, tt = got[12] * got[:9].reshape(3, 3), got[9:12]
        assert np.allclose(m["T12"][h], np.hstack([sR, tt[:, None]]), atol=1e-5)
        assert np.allclose(m["T21"][h], np.hstack([sR.T / got[12] ** 2, (-(sR.T / got[12] ** 2) @ tt)[:, None]]), atol=1e-4)
    with capsys.disabled():
        print(f"\ncomputeT f32 vs f64: left out {left_out}/400, max deviation {dev}, bound {BOUND}")
    assert left_out <= 20, "at most 5 % of the sets may be left out as ill-conditioned"
    for k in dev:
        assert dev[k] <= BOUND[k], (k, dev[k], BOUND[k])
    # and the similarity itself is recovered by the well-conditioned sets
    assert abs(np.median(m["sim3"][:, 12]) - 1.7) < 0.05


# ---- degenerate sets ---------------------------------------------------------------------------------
def test_exact_scale_and_translation_is_nan_and_scores_nothing():
    x2 = f32([[1, 2, 4], [2, -4, 1], [-3, 2, -5], [0.5, 0.25, 8]])
    x1 = 2 * x2 + f32([1, 2, 4])
    m = s3.compute(x1, x2, [[0, 1, 2]])
    assert m["quat"][0].tolist() == [1, 0, 0, 0], "N's first row is exactly zero off the diagonal"
    assert np.isnan(m["T12"]).all() and np.isnan(m["T21"]).all() and np.isnan(m["sim3"][0, :12]).all()
    s2 = np.ones(4, f32)
    r = s3.iterate(x1, x2, s2, s2, K, K, None, 3, sets_=[[0, 1, 2]])
    assert r["counts"].tolist() == [0] and r["first_accept"] == -1


def test_repeated_index_is_deterministic():
    c = s3.cloud(50, seed=3)
    sets = [[1, 4, 4], [7, 7, 7], [0, 0, 9]]
    a, b = s3.compute(c["x3dc1"], c["x3dc2"], sets), s3.compute(c["x3dc1"], c["x3dc2"], sets)
    for k in ("T12", "T21", "sim3", "quat"):
        assert a[k].tobytes() == b[k].tobytes()
    assert np.isnan(a["sim3"][1]).any(), "three times one point: den = 0"


# ---- iterate -----------------------------------------------------------------------------------------
def test_too_few_correspondences_is_no_more():
    c = s3.cloud(5, seed=4)
    sol = s3.Solver(c["x3dc1"], c["x3dc2"], c["sigma2_1"], c["sigma2_2"], K, K, np.arange(5), 9, np.zeros((10, 3)),
                    min_inliers=6)
    T, no_more, vb, n = sol.iterate(5)
    assert T is None and no_more and not vb.any() and n == 0 and sol.iterations == 0
    r = s3.iterate(c["x3dc1"], c["x3dc2"], c["sigma2_1"], c["sigma2_2"], K, K, np.zeros((4, 3), np.int64), 6)
    assert not r["counts"].any() and r["first_accept"] == -1 and not r["sets"].any() and not r["T12"].any()


def test_two_calls_equal_one_long_call_and_the_last_maximum_wins():
    c = s3.cloud(120, seed=5, outliers=0.3)
    a = (c["x3dc1"], c["x3dc2"], c["sigma2_1"], c["sigma2_2"], K, K)
    rng = np.random.default_rng(12)
    r = rng.integers(0, 2 ** 31, (60, 3))
    r[41] = r[17]  # the same set twice: the same count
    one = s3.iterate(*a, r, 119)  # min_inliers so high that nothing is accepted
    assert one["first_accept"] == -1 and one["counts"].max() > 6
    h1 = s3.iterate(*a, r[:25], 119)
    best = int(h1["counts"][h1["best_at"][-1]])
    h2 = s3.iterate(*a, r[25:], 119, best)
    assert np.array_equal(np.concatenate([h1["counts"], h2["counts"]]), one["counts"])
    at2 = np.where(h2["best_at"] >= 0, h2["best_at"] + 25, h1["best_at"][-1])
    assert np.array_equal(np.concatenate([h1["best_at"], at2]), one["best_at"])
    # first_accept carried: with a bound below the best count the long call and the two calls stop
    # at the same iteration
    lo = int(np.sort(one["counts"])[-3])
    long_first = s3.iterate(*a, r, lo - 1)["first_accept"]
    f1 = s3.iterate(*a, r[:5], lo - 1)
    if f1["first_accept"] < 0:
        f2 = s3.iterate(*a, r[5:], lo - 1, int(f1["counts"][f1["best_at"][-1]]))
        assert f2["first_accept"] + 5 == long_first
    else:
        assert f1["first_accept"] == long_first
    # the last maximum wins: identical sets give identical counts, the later one holds the best
    rr = np.repeat(r[17:18], 6, 0)
    same = s3.iterate(*a, rr, 119)
    assert len(set(same["counts"])) == 1 and same["best_at"].tolist() == list(range(6))


def test_solver_block_calls_equal_find():
    c = s3.cloud(150, seed=6, outliers=0.3)
    rng = np.random.default_rng(13)
    r = rng.integers(0, 2 ** 31, (300, 3))
    mk = lambda: s3.Solver(c["x3dc1"], c["x3dc2"], c["sigma2_1"], c["sigma2_2"], K, K, np.arange(150) * 2, 300, r,  # noqa: E731
                           min_inliers=60)
    a, b = mk(), mk()
    Tb, _, vbb, nb = b.iterate(b.max_its)
    T, no_more = None, False
    while T is None and not no_more:
        T, no_more, vb, n = a.iterate(5)
    assert Tb is not None and T.tobytes() == Tb.tobytes() and np.array_equal(vb, vbb) and n == nb
    assert a.iterations == b.iterations and n > 60
