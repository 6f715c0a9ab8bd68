"""GPU matchers on the adversarial scenes of tests/adversarial_scenes.py: dependency chains as
deep as the query list, pairs exactly on every acceptance threshold, and the size edges of the
host BoW path.  Every result is compared element for element with the CPU oracle and with the
expectation known by construction (count and mapping), so no test passes on two empty results.

Which resolver a test reaches (csrc/orb_match.hip, csrc/orb_sfi.hip):
  test_fix_*            k_resolve_fix, chains of more than one and more than two 1024-thread
                        strides with short candidate lists, 200 links with truncated lists
  test_resolve_*        k_resolve: BoW on the generic path, SearchForTriangulation, and the grid
                        matchers once takenBy + queries exceed the fixed point's LDS
  test_sfi_*            k_match_init: fixed point (one pair, <= 1024 level-0 keypoints), the
                        large-capacity body (> 1024), the 8-wave speculated pass (256 pairs)
  test_ratio_tables     every matcher's accept rule on and around its float / integer cuts
  test_bow_size_edges   the first sizes past the batched BoW kernel and under k_resolve's limit
tests/test_adversarial_scenes_oracle.py proves the same expectations against the oracle on the
CPU."""
import numpy as np
import pytest

import orbslam_jpminipc_amd as orb
from orbslam_jpminipc_amd._native import ORB_ENOTSUP, OrbError
from orbslam_jpminipc_amd.views import FeatureVector, View
from oracle_lib import OracleMatcher, search_for_initialization
import adversarial_scenes as A
import scenes as S

pytestmark = pytest.mark.gpu

W, H = A.W, A.H
RATIOS = (0.6, 0.75, 0.8, 0.9)


def rng_of(*key):
    return np.random.default_rng([11, *[int(k) if k is not None else 99991 for k in key]])


def both(nnratio=0.9, checkOri=False):
    return orb.ORBmatcher(nnratio, checkOri), OracleMatcher(nnratio, checkOri)


def same(a, b, expect=None):
    """GPU result a == oracle result b (count and every element) == the analytic expectation."""
    na, oa = a
    nb, ob = b
    assert na == nb, (na, nb)
    np.testing.assert_array_equal(oa, ob)
    if expect is not None:
        np.testing.assert_array_equal(oa, expect)
        assert na == (expect >= 0).sum()
    return na


def expect_grid(C, mode, ori):
    return C.by_target_ori if ori and mode in A.ORI_MODES else C.by_target


FIX_CASES = [("window", "A"), ("window", "B"), ("local", "A"), ("f2f", "A"), ("motion", "B"), ("reloc", "B"),
             ("sim3", "B")]


# ---- (a) k_resolve_fix ------------------------------------------------------------------------
@pytest.mark.parametrize("n,layout,mid", [(1100, "short", 1029), (2100, "short", 2051), (200, "long", 137)])
@pytest.mark.parametrize("mode,kind", FIX_CASES)
def test_fix_chain(mode, kind, n, layout, mid):
    """One iteration of the fixed point per link.  broken = 0 (kind A: nothing matches) and a
    break past the last 1024-thread stride (kind A: nothing after it matches; kind B: every
    later link shifts by one), so a resolver that stopped early or dropped the cross-query
    state differs in every link after the break."""
    for lead, broken in ((0, None), (3, 0), (7, mid)):
        C = A.chain_scene(rng_of(1, n, lead, broken), n, kind, layout, lead, broken)
        assert C.count == (n if broken is None else broken if kind == "A" else n - 1)
        for ori in (False, True):
            g, o = both(0.9, ori)
            same(A.run_grid(g, mode, C), A.run_grid(o, mode, C), expect_grid(C, mode, ori))


@pytest.mark.parametrize("mode", ["local", "f2f"])
def test_fix_chain_taken_head(mode):
    """T[0] taken before the call: query 0 has nothing left, query 1 sees T[0] taken as if
    query 0 had matched it, links 1 .. n-1 match."""
    C = A.chain_scene(rng_of(2), 1100, "A", take_first=True)
    g, o = both()
    assert same(A.run_grid(g, mode, C, C.taken0), A.run_grid(o, mode, C, C.taken0), C.by_target) == 1099


# ---- (b) k_resolve ----------------------------------------------------------------------------
BOW_VARIANTS = [(0, None), (3, None), (7, None), (3, 0), (7, 77)]


def _bow_both(C, fv1, fv2, nnratio, ori, off_q=0, off_t=0, Q=None, T=None, uq=None):
    """KF-F and KF-KF on GPU and oracle; the chain's rows sit at off_q / off_t of Q / T."""
    Q, T = C.Q if Q is None else Q, C.T if T is None else T
    uq = C.usable if uq is None else uq
    g, o = both(nnratio, ori)
    by_t = C.by_target_ori if ori else C.by_target
    n1, out = g.SearchByBoW_KF_F(Q, uq, fv1, T, fv2)
    same((n1, out), o.SearchByBoW_KF_F(Q, uq, fv1, T, fv2))
    np.testing.assert_array_equal(out[off_t : off_t + C.n], np.where(by_t >= 0, by_t + off_q, -1))
    n2, out = g.SearchByBoW_KF_KF(Q, uq, fv1, T, None, fv2)
    same((n2, out), o.SearchByBoW_KF_KF(Q, uq, fv1, T, None, fv2))
    by_q = C.by_query(ori)
    np.testing.assert_array_equal(out[off_q : off_q + C.Q.n], np.where(by_q >= 0, by_q + off_t, -1))
    return n1, n2


@pytest.mark.parametrize("lead,broken", BOW_VARIANTS)
def test_resolve_bow_chain_duplicate_feature(lead, broken):
    """A FeatureVector that lists one feature twice goes to the generic resolver: a 200-link
    chain (three 64-query chunks plus a tail) in one node, from every alignment of the
    8-query speculation groups."""
    C = A.chain_scene(rng_of(3, lead, broken), 200, "A", "short", lead, broken)
    fv1, fv2 = A.chain_bow(C, duplicate=True)
    for nnratio in (0.9, 0.75):
        for ori in (False, True):
            n1, n2 = _bow_both(C, fv1, fv2, nnratio, ori)
            assert n1 == n2 == (C.count_ori if ori else C.count)
    assert C.count == (200 if broken is None else broken)


@pytest.mark.parametrize("lead,broken", [(0, None), (7, 77)])
def test_resolve_bow_chain_in_8200_features(lead, broken):
    """The same chain as one node of frames with 8 200 features (past the batched kernel's
    8 192): the generic path with unique vectors."""
    rng = rng_of(4, lead, broken)
    C = A.chain_scene(rng, 200, "A", "short", lead, broken)
    V1, f1, V2, f2 = A.big_bow_pair(rng, 8200 - C.Q.n, 8000)
    Q = View(np.concatenate([V1.kps, C.Q.kps]), np.vstack([V1.desc, C.Q.desc]), (0, W, 0, H))
    T = A.target_view(np.concatenate([V2.kps, C.T.kps]), np.vstack([V2.desc, C.T.desc]))
    assert Q.n == 8200
    node = int(f1.nodes[len(f1.nodes) // 2]) + 1  # (between the fillers' nodes)
    assert node not in f1.nodes and node not in f2.nodes

    def merged(fv, feats):
        d = {int(x): fv.features[fv.offsets[k] : fv.offsets[k + 1]].tolist() for k, x in enumerate(fv.nodes)}
        d[node] = feats
        return FeatureVector.from_dict(d)

    fv1 = merged(f1, list(range(V1.n, V1.n + C.Q.n)))
    fv2 = merged(f2, list(range(V2.n, V2.n + C.n)))
    uq = np.concatenate([np.ones(V1.n, np.uint8), C.usable])
    n1, n2 = _bow_both(C, fv1, fv2, 0.9, False, V1.n, V2.n, Q, T, uq)
    assert n1 > C.count and n2 > C.count


@pytest.mark.parametrize("lead,broken", BOW_VARIANTS)
def test_resolve_triangulation_chain(lead, broken):
    """SearchForTriangulation over a kind-B chain (A.triangulation_scene: every keypoint on one
    image row and F12 a translation along x, so each link's epipolar distance is exactly 0).
    Its walk takes the first unmatched candidate within 2 * bestDist; a break shifts every later
    link by one."""
    V1, h1, fv1, V2, fv2, F12, exp, exp_o = A.triangulation_scene(rng_of(5, lead, broken), 200, lead, broken)
    h2 = np.zeros(V2.n, np.uint8)
    for ori, e in ((False, exp), (True, exp_o)):
        g, o = both(0.6, ori)
        n = same(g.SearchForTriangulation(V1, h1, fv1, V2, h2, fv2, F12),
                 o.SearchForTriangulation(V1, h1, fv1, V2, h2, fv2, F12), e)
        assert n >= 170


def embedded(rng, C, n_t, n_q, at):
    """Chain scene C inside frames of n_t targets and n_q queries: the chain's targets first,
    its queries at rows at .. ; the fillers (clustered copies of filler targets, ~20 bits
    flipped) live below y = 120, out of every chain window."""
    nt, nq = n_t - C.n, n_q - C.Q.n
    tk = A.kps_at(rng.uniform(20, W - 20, nt), rng.uniform(120, H - 20, nt))
    td = S.descriptors(rng, nt)
    src = rng.integers(0, nt, nq)
    qk = A.kps_at(tk["x"][src] + rng.normal(0, 2, nq), np.maximum(tk["y"][src] + rng.normal(0, 2, nq), 110.0))
    qd = td[src] ^ A._pack(rng.random((nq, 256)) < 0.08)
    Q = View(np.concatenate([qk[:at], C.Q.kps, qk[at:]]), np.vstack([qd[:at], C.Q.desc, qd[at:]]), (0, W, 0, H))
    T = A.target_view(np.concatenate([C.T.kps, tk]), np.vstack([C.T.desc, td]))
    usable = np.concatenate([np.ones(at, np.uint8), C.usable, np.ones(nq - at, np.uint8)])
    none = np.full(n_t, -1, np.int32)
    return A.Chain(C.kind, C.n, C.lead, C.broken, C.window, Q, T, usable, np.zeros(n_t, np.uint8), none, none)


@pytest.mark.parametrize("mode,kind", [("local", "A"), ("f2f", "A"), ("window", "A"), ("motion", "B"), ("reloc", "B"),
                                       ("sim3", "B")])
def test_resolve_grid_chain_past_fixed_point_lds(mode, kind):
    """11 800 targets and 16 384 queries (the most a query frame may hold): takenBy (8 B per
    target) + the rescan list (4 B per query) exceed the fixed point's 150 KB while k_resolve's
    13 B per target still fit, so the grid matchers take the speculated sequential pass: a
    200-link chain starting at query row 8 003 + 3, unbroken and broken."""
    for broken in (None, 77):
        rng = rng_of(6, broken)
        C = A.chain_scene(rng, 200, kind, "short", 3, broken)
        E = embedded(rng, C, 11800, 16384, 8003)
        assert 2 * E.T.n * 4 + E.Q.n * 4 + 16 > 150 * 1024 >= 13 * E.T.n + 16
        g, o = both()
        n, out = A.run_grid(g, mode, E)
        same((n, out), A.run_grid(o, mode, E))
        np.testing.assert_array_equal(out[: C.n], np.where(C.by_target >= 0, C.by_target + 8003, -1))
        assert n > C.count


# ---- (c) k_match_init -------------------------------------------------------------------------
def sfi_two_calls(k1, d1, k2, d2, expect, nnratio=0.9, checkOri=False, window=A.SHORT_WINDOW):
    """Both calls of the initialiser's pattern: the second reads the vbPrevMatched the first
    wrote (the matched F2 positions); the chain's result is the same from there."""
    F1, F2 = orb.Frame(k1, d1, W, H), orb.Frame(k2, d2, W, H)
    matcher = orb.ORBmatcher(nnratio, checkOri)
    prev = np.ascontiguousarray(np.stack([k1["x"], k1["y"]], 1).astype(np.float32))
    prev_o = prev.copy()
    for _ in range(2):
        m12 = []
        n = matcher.SearchForInitialization(F1, F2, prev, m12, window)
        no, m12o = search_for_initialization(k1, d1, k2, d2, W, H, prev_o, nnratio, checkOri, window)
        same((n, np.array(m12, np.int32)), (no, m12o), expect)
        assert prev.tobytes() == prev_o.tobytes()
    return n


@pytest.mark.parametrize("n", [1000, 1500])
def test_sfi_chain_host(n):
    """One pair on the host entry point: 1 000 level-0 keypoints take k_match_init's fixed
    point, 1 500 exceed nmax = 1024 and take the large-capacity body."""
    for lead, broken in ((0, None), (3, 0), (7, n - 139)):
        C = A.chain_scene(rng_of(7, n, lead, broken), n, "A", "short", lead, broken, disabled_octave=1)
        for ori in (False, True):
            cnt = sfi_two_calls(C.Q.kps, C.Q.desc, C.T.kps, C.T.desc, C.by_query(ori), 0.9, ori)
            assert cnt == (C.count_ori if ori else C.count)
        assert C.count == (n if broken is None else broken)


def test_sfi_chain_after_acceptor_overflow():
    """Five copies of query 0 ahead of the chain: with query 0 itself six queries accept T[0]
    in the fixed point's first iteration, more than a slot's acceptor list holds, so the pass
    hands over to the sequential one in the middle of a chained scene.  The first copy keeps
    T[0] (a later equal distance does not steal it), query 0 stays unmatched, and query 1 finds
    T[0] matched at 20 <= 22, so links 1 .. n-1 match."""
    n = 600
    C = A.chain_scene(rng_of(8), n, "A", "short", 0, None, disabled_octave=1)
    k1 = np.concatenate([np.repeat(C.Q.kps[:1], 5), C.Q.kps])
    d1 = np.vstack([np.repeat(C.Q.desc[:1], 5, 0), C.Q.desc])
    exp = np.full(n + 5, -1, np.int32)
    exp[0] = 0
    exp[6:] = np.arange(1, n)
    assert sfi_two_calls(k1, d1, C.T.kps, C.T.desc, exp) == n


def test_sfi_chain_batch_256_pairs():
    """256 pairs of capacity 256 in one launch (the 8-wave speculated pass), each with its own
    200-link chain: lead p % 8, every third pair broken at its own link."""
    import torch

    P, cap, n = 256, 256, 200
    kps = np.zeros((2 * P, cap, 28), np.uint8)
    desc = np.zeros((2 * P, cap, 32), np.uint8)
    cnt = np.zeros(2 * P, np.int32)
    chains = []
    for p in range(P):
        broken = (37 * p) % n if p % 3 == 0 else None
        C = A.chain_scene(rng_of(9, p), n, "A", "short", p % 8, broken, disabled_octave=1)
        chains.append(C)
        for f, V in ((2 * p, C.Q), (2 * p + 1, C.T)):
            kps[f, : V.n] = np.frombuffer(np.ascontiguousarray(V.kps).tobytes(), np.uint8).reshape(V.n, 28)
            desc[f, : V.n] = V.desc
            cnt[f] = V.n
    f1 = torch.arange(0, 2 * P, 2, dtype=torch.int32, device="cuda")
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    d_kps, d_desc, d_cnt = t(kps), t(desc), t(cnt)
    for ori in (False, True):
        prev = np.zeros((P, cap, 2), np.float32)
        for p, C in enumerate(chains):
            prev[p, : C.Q.n, 0], prev[p, : C.Q.n, 1] = C.Q.kps["x"], C.Q.kps["y"]
        d_prev = t(prev)
        prev_o = prev.copy()
        for call in range(2):
            m12, nm = orb.ORBmatcher(0.9, ori).search_for_initialization_batch_device(
                d_kps, d_desc, d_cnt, f1, f1 + 1, W, H, A.SHORT_WINDOW, d_prev_xy=d_prev)
            torch.cuda.synchronize()
            m12, nm, prev_g = m12.cpu().numpy(), nm.cpu().numpy(), d_prev.cpu().numpy()
            total = 0
            for p, C in enumerate(chains):
                po = np.ascontiguousarray(prev_o[p, : C.Q.n])
                no, mo = search_for_initialization(C.Q.kps, C.Q.desc, C.T.kps, C.T.desc, W, H, po, 0.9, ori,
                                                   A.SHORT_WINDOW)
                prev_o[p, : C.Q.n] = po
                same((nm[p], m12[p, : C.Q.n]), (no, mo), C.by_query(ori))
                assert prev_g[p, : C.Q.n].tobytes() == po.tobytes(), (p, call)
                total += no
            assert total > 100 * P


# ---- (d) ratio and threshold tables -------------------------------------------------------------
@pytest.mark.parametrize("nnratio", RATIOS)
def test_ratio_tables(nnratio):
    """Isolated queries with best / second-best candidates at exact distances (d1, d2) for
    d1 = floor(r d2) - 1, floor(r d2), ceil(r d2), d2 = 2 .. 83, and lone candidates at
    TH_LOW, TH_HIGH and ORBdist = 64, each +- 1, through every matcher: accepted exactly where a
    float32 evaluation of the matcher's rule accepts (`<` against `<=`, the order of the
    product, single precision)."""
    Tb = A.ratio_table(rng_of(10, int(100 * nnratio)), nnratio)
    assert Tb.exact_ties(nnratio) >= 8
    g, o = both(nnratio, False)
    dup = FeatureVector.from_dict({**{int(x): [k] for k, x in enumerate(Tb.fvq.nodes)}, 10**6: [0]})
    for fvq in (Tb.fvq, dup):  # the node-parallel kernel, then the generic resolver
        cnt, by_t, by_q = Tb.expect("bow_kf_f", nnratio)
        assert same(g.SearchByBoW_KF_F(Tb.Q, None, fvq, Tb.T, Tb.fvt), o.SearchByBoW_KF_F(Tb.Q, None, fvq, Tb.T, Tb.fvt),
                    by_t) == cnt > 50
        cnt, by_t, by_q = Tb.expect("bow_kf_kf", nnratio)
        assert same(g.SearchByBoW_KF_KF(Tb.Q, None, fvq, Tb.T, None, Tb.fvt),
                    o.SearchByBoW_KF_KF(Tb.Q, None, fvq, Tb.T, None, Tb.fvt), by_q) == cnt > 50
    C = A.table_chain(Tb)
    for mode in A.GRID_MODES:
        cnt, by_t, _ = Tb.expect(mode, nnratio, 64 if mode == "reloc" else 100)
        assert same(A.run_grid(g, mode, C, orbdist=64), A.run_grid(o, mode, C, orbdist=64), by_t) == cnt > 50
    for name in ("fuse", "triang", "sim3_pair"):  # by query, best distance cut at TH_LOW
        cnt, _, by_q = Tb.expect(name, nnratio)
        assert same(A.run_table_by_query(g, name, Tb), A.run_table_by_query(o, name, Tb), by_q) == cnt > 50
    cnt, _, by_q = Tb.expect("sfi", nnratio)
    assert sfi_two_calls(Tb.Q.kps, Tb.Q.desc, Tb.T.kps, Tb.T.desc, by_q, nnratio, False, Tb.window) == cnt > 50


# ---- (f) size edges of the host BoW path --------------------------------------------------------
@pytest.mark.parametrize("n", [8193, 11800])
def test_bow_size_edges(n):
    """8 193 features: the first size past the batched kernel; 11 800: just under what
    k_resolve's 13 B per target admit (11 814).  KF-F, KF-KF and (8 193) SearchForTriangulation."""
    V1, fv1, V2, fv2 = A.big_bow_pair(rng_of(12, n), n, n)
    u1 = (np.arange(n) % 7 != 3).astype(np.uint8)
    for nnratio, ori in ((0.75, True), (0.9, False)):
        g, o = both(nnratio, ori)
        assert same(g.SearchByBoW_KF_F(V1, u1, fv1, V2, fv2), o.SearchByBoW_KF_F(V1, u1, fv1, V2, fv2)) > n // 10
        assert same(g.SearchByBoW_KF_KF(V1, u1, fv1, V2, None, fv2),
                    o.SearchByBoW_KF_KF(V1, u1, fv1, V2, None, fv2)) > n // 10
    if n == 8193:
        F12 = A.F12_ROWS  # epipolar lines y2 = y1
        for V in (V1, V2):  # six image rows: about one candidate in six lies on the query's line
            V.kps["y"] = np.rint(V.kps["y"] / 80) * 80 + 20
        h = np.zeros(n, np.uint8)
        g, o = both(0.6, True)
        assert same(g.SearchForTriangulation(V1, h, fv1, V2, h, fv2, F12),
                    o.SearchForTriangulation(V1, h, fv1, V2, h, fv2, F12)) > n // 20


@pytest.mark.parametrize("kf_kf", [False, True])
def test_bow_16384_features_exact_or_refused(kf_kf):
    """Past k_resolve's LDS limit the call must be refused on the host (ORB_ENOTSUP, nothing
    launched) or be exact; a wrong answer is a failure."""
    n = 16384
    V1, fv1, V2, fv2 = A.big_bow_pair(rng_of(13), n, n)
    g, o = both(0.75, True)
    try:
        r = g.SearchByBoW_KF_KF(V1, None, fv1, V2, None, fv2) if kf_kf else g.SearchByBoW_KF_F(V1, None, fv1, V2, fv2)
    except OrbError as e:
        assert e.code == ORB_ENOTSUP, e
        return
    ro = o.SearchByBoW_KF_KF(V1, None, fv1, V2, None, fv2) if kf_kf else o.SearchByBoW_KF_F(V1, None, fv1, V2, fv2)
    assert same(r, ro) > n // 10
