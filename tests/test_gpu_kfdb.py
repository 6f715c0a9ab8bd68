"""GPU parity of the KeyFrameDatabase and the L1 BoW score (csrc/orb_kfdb.hip) against the
plain-Python model of the reference (tests/kfdb_model.py, proven on its own in
tests/test_kfdb_model.py): doubles, floats, counts and id order bit for bit.

The device database and the model are driven in lockstep (Lockstep below): every query compares
the candidates and, through orb_debug_kfdb_last_query, the per-keyframe common-word count, first
shared word, scored flag and double score, so a wrong count, a wrong score and a wrong order
fail in different places."""
import ctypes

import numpy as np
import pytest

import orbslam_jpminipc_amd as orb
from orbslam_jpminipc_amd import _native
import kfdb_cases as C
from kfdb_model import ModelDatabase, bow_items, l1_score

pytestmark = pytest.mark.gpu

U = C.U
_vocs = {}


def flat_vocabulary(n_words: int, scoring: int = 0):
    """n_words leaves under the root: only the word count and the scoring type matter here."""
    key = (n_words, scoring)
    if key not in _vocs:
        _vocs[key] = orb.ORBVocabulary.from_arrays(10, 1, scoring, 0, np.zeros(n_words, np.int32),
                                                   np.ones(n_words, np.uint8), np.zeros((n_words, 32), np.uint8),
                                                   np.ones(n_words, np.float64))
    return _vocs[key]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def check_table(dev, model, q=0, connected=()):
    """Debug table of the device's query q against the model's last query."""
    if not model.last and len(model) == 0:
        return
    t = dev.debug_last_query(q)
    for s in range(len(t["common"])):
        kid = dev._id[s]
        row = model.last.get(kid)
        if row is None:
            assert t["scored"][s] == 0, ("scored", kid)
            if kid not in connected:  # the scan counts connected keyframes too; the list leaves them out
                assert t["common"][s] == 0, ("common", kid, t["common"][s])
            continue
        common, first, scored, score = row
        assert t["common"][s] == common, ("common", kid, t["common"][s], common)
        assert t["first"][s] == first, ("first", kid, t["first"][s], first)
        assert bits(t["score"][s]) == bits(score), ("score", kid, t["score"][s], score)
        assert t["scored"][s] == int(scored), ("scored", kid)
        assert t["seq"][s] == model.kfs[kid].seq, ("seq", kid)


class Lockstep:
    """The device database and the model, given the same calls; a query returns the device's
    answer after comparing it with the model's."""

    def __init__(self, n_words=C.N_WORDS, max_keyframes=512, max_entries=None):
        self.dev = orb.KeyFrameDatabase(flat_vocabulary(n_words), max_keyframes, max_entries)
        self.model = ModelDatabase()

    def add(self, kf_id, bow):
        self.dev.add(kf_id, bow)
        self.model.add(kf_id, bow)

    def erase(self, kf_id):
        self.dev.erase(kf_id)
        self.model.erase(kf_id)

    def clear(self):
        self.dev.clear()
        self.model.clear()

    def set_covisible(self, kf_id, nb):
        self.dev.set_covisible(kf_id, nb)
        self.model.set_covisible(kf_id, nb)

    def DetectRelocalisationCandidates(self, bow):
        expect = self.model.DetectRelocalisationCandidates(bow)
        got = self.dev.DetectRelocalisationCandidates(bow)
        if expect or self.model.last:
            check_table(self.dev, self.model)
        assert got == expect, ("reloc", got, expect)
        assert len(self.dev) == len(self.model)
        return got

    def DetectLoopCandidates(self, bow, connected_ids=(), min_score=0.0):
        expect = self.model.DetectLoopCandidates(bow, connected_ids, min_score)
        got = self.dev.DetectLoopCandidates(bow, connected_ids, min_score)
        if expect or self.model.last:
            check_table(self.dev, self.model, connected=set(connected_ids))
        assert got == expect, ("loop", got, expect)
        return got


# ---- score ------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 63, 64, 65, 1000, 8192)


def _score_frames():
    """Per length n: a random vector, its copy, a disjoint one (other words), an interleaved one
    (every second word shared, the others in between) and one sharing only the last word; values
    10^-12 .. 1 so that the order of the additions shows in the sum."""
    rng = np.random.default_rng(77)
    frames = []
    val = lambda n: 10.0 ** rng.uniform(-12, 0, n)  # noqa: E731
    for n in LENGTHS:
        w = np.sort(rng.choice(4 * n + 4, n, replace=False)).astype(np.uint32) * 4
        frames.append((w, val(n)))
        frames.append((w.copy(), frames[-1][1].copy()))
        frames.append((w + 1, val(n)))
        iw = w.copy()
        iw[1::2] += 2
        frames.append((iw, val(n)))
        lw = w + 3
        if n:
            lw[-1] = w[-1]
        frames.append((lw, val(n)))
    return frames


def test_score_pairs_bit_exact_and_order_sensitive():
    import torch

    frames = _score_frames()
    B, cap = len(frames), 8192
    bw = np.zeros((B, cap), np.uint32)
    bv = np.zeros((B, cap), np.float64)
    bn = np.array([len(w) for w, _ in frames], np.int32)
    for f, (w, v) in enumerate(frames):
        bw[f, : len(w)] = w
        bv[f, : len(w)] = v
    pairs = [(5 * g + a, 5 * g + b) for g in range(len(LENGTHS)) for a in range(5) for b in range(5)]
    pairs += [(5 * ga + a, 5 * gb + b) for ga, gb, a, b in ((6, 5, 0, 0), (5, 6, 0, 3), (6, 4, 3, 0), (2, 6, 0, 0),
                                                            (4, 3, 0, 3), (1, 6, 0, 0), (6, 0, 0, 0), (0, 0, 0, 0))]
    items = [bow_items(f) for f in frames]
    expect = np.array([l1_score(items[a], items[b]) for a, b in pairs])
    reverse = np.array([l1_score(items[a], items[b], reverse=True) for a, b in pairs])
    # without this the comparison below would prove nothing about the order of the additions
    assert (bits(expect) != bits(reverse)).sum() >= 10
    voc = flat_vocabulary(C.N_WORDS)
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    got = voc.score_pairs_device(t(bw.view(np.int32)), t(bv), t(bn), t(np.array([a for a, _ in pairs], np.int32)),
                                 t(np.array([b for _, b in pairs], np.int32)))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    bad = np.flatnonzero(bits(got) != bits(expect))
    assert bad.size == 0, [(pairs[i], got[i], expect[i]) for i in bad[:5]]
    assert (expect > 0).sum() > 20 and (expect == 0).sum() > 5
    # the host entry point: the same doubles
    for p in (3, 30, 80, 130, 170, len(pairs) - 6):
        a, b = pairs[p]
        assert bits(voc.score(frames[a], frames[b])) == bits(expect[p])
    assert voc.score({1: 0.5, 7: 0.5}, {7: 0.25, 9: 0.75}) == 0.25


# ---- random databases -----------------------------------------------------------------------------
def _random_bow(rng, n_words, n):
    w = np.sort(rng.choice(n_words, min(n, n_words), replace=False)).astype(np.uint32)
    v = rng.random(len(w)) + 1e-3
    return w, v / v.sum()


def _perturbed(rng, bow, n_words, keep):
    """A query near a keyframe: `keep` of its words (re-weighted) plus some others."""
    w, v = bow
    sel = rng.random(len(w)) < keep
    sel[0] = True
    extra = rng.choice(n_words, max(1, len(w) // 4), replace=False).astype(np.uint32)
    d = {int(a): float(b) for a, b in zip(extra, rng.random(len(extra)) + 1e-3)}
    d.update({int(a): float(b) * float(rng.uniform(0.5, 1.5)) for a, b in zip(w[sel], v[sel])})
    keys = sorted(d)
    vals = np.array([d[k] for k in keys])
    return np.array(keys, np.uint32), vals / vals.sum()


@pytest.mark.parametrize("n_words", [1000, 100000])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 300])
def test_random_database(N, n_words):
    rng = np.random.default_rng([N, n_words])
    db = Lockstep(n_words, max_keyframes=512, max_entries=N * 500)
    ids = rng.permutation(1000)[:N].tolist()
    bows = {}
    for k in ids:
        bows[k] = _random_bow(rng, n_words, int(rng.integers(1, 501)))
        db.add(k, bows[k])
    for k in ids:
        nb = rng.choice(ids + [5000, 5001], min(len(ids) + 2, int(rng.integers(0, 11))), replace=False).tolist()
        db.set_covisible(k, nb)
    nonempty = 0
    for r in range(3):
        near = bows[ids[int(rng.integers(0, N))]]
        q = _perturbed(rng, near, n_words, 0.7)
        nonempty += len(db.DetectRelocalisationCandidates(q)) > 0
        conn = rng.choice(ids, min(N, 3), replace=False).tolist() if r else []
        ms = [0.0, 0.01, 0.05][r]
        db.DetectLoopCandidates(q, conn, ms)
        q = _random_bow(rng, n_words, int(rng.integers(1, 501)))
        db.DetectRelocalisationCandidates(q)  # the stored scores of the queries before count here
        db.DetectLoopCandidates(q, conn, 0.0)
    assert nonempty == 3
    for k in ids[::3]:
        db.erase(k)
    db.DetectRelocalisationCandidates(_perturbed(rng, bows[ids[1 % N]], n_words, 0.9))


# ---- cases known by construction -----------------------------------------------------------------
@pytest.mark.parametrize("M", range(1, 41))
def test_min_common_boundary(M):
    C.case_min_common(Lockstep(), M)


@pytest.mark.parametrize("name", list(C.CASES))
def test_case(name):
    C.CASES[name](Lockstep())


# ---- the pool --------------------------------------------------------------------------------------
def test_pool_churn_compaction_and_range():
    rng = np.random.default_rng(9)
    db = Lockstep(max_keyframes=64, max_entries=1000)
    mk = lambda n: _random_bow(rng, C.N_WORDS, n)  # noqa: E731
    q = _random_bow(rng, C.N_WORDS, 400)
    live = {}
    for k in range(5):
        live[k] = mk(200)
        db.add(k, live[k])          # the tail is at 1000 = max_entries
    db.DetectRelocalisationCandidates(q)
    nxt = 5
    for victim in (1, 0, 4, 3, 2):   # every add below finds no room at the tail: compaction
        db.erase(victim)
        live.pop(victim)
        with pytest.raises(orb.OrbError) as e:  # 800 live + 201 do not fit
            db.dev.add(99, mk(201))
        assert e.value.code == _native.ORB_ERANGE and "max_entries" in str(e.value)
        for part in (120, 80):       # 800 live + 200 fit exactly, after compaction
            live[nxt] = mk(part)
            db.add(nxt, live[nxt])
            nxt += 1
        assert len(db.dev) == len(live)
        db.DetectRelocalisationCandidates(q)
        db.DetectLoopCandidates(q, [2], 0.0)
        with pytest.raises(orb.OrbError) as e:  # full
            db.dev.add(98, mk(1))
        assert e.value.code == _native.ORB_ERANGE
    db.add(50, ([], []))             # an empty BowVector is a keyframe that shares nothing
    assert db.DetectRelocalisationCandidates(q) and 50 not in db.DetectRelocalisationCandidates(q)
    db.clear()
    assert len(db.dev) == 0
    assert db.DetectRelocalisationCandidates(q) == []
    db.add(7, mk(1000))
    assert db.DetectRelocalisationCandidates(q) == [7]


# ---- the batch entry point -----------------------------------------------------------------------
def _pack_queries(queries, cap):
    import torch

    Q = len(queries)
    bw = np.zeros((Q, cap), np.uint32)
    bv = np.zeros((Q, cap), np.float64)
    bn = np.zeros(Q, np.int32)
    for i, q in enumerate(queries):
        w, v = orb.vocabulary.bow_arrays(q)
        bw[i, : len(w)] = w
        bv[i, : len(w)] = v
        bn[i] = len(w)
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    return t(bw.view(np.int32)), t(bv), t(bn)


def _stale_db(extra):
    """case_neighbour_stale's keyframes plus random ones."""
    rng = np.random.default_rng(31)
    db = Lockstep(max_keyframes=128)
    C._ab(db)
    db.add(C.N, {0: U, 100: 1024 * U})
    for k in range(extra):
        db.add(200 + k, _random_bow(rng, C.N_WORDS, int(rng.integers(1, 300))))
        db.set_covisible(200 + k, [C.A, 200 + (k * 7) % extra, C.N])
    return db, rng


@pytest.mark.parametrize("Q", [1, 2, 17])
def test_batch_equals_single_calls(Q):
    import torch

    db, rng = _stale_db(40)
    single, _ = _stale_db(40)
    if Q == 1:
        queries = [C.Q2]
    elif Q == 2:
        queries = [C.Q1, C.Q2]  # query 1 needs the score that query 0 stores for N
    else:
        queries = [_random_bow(rng, C.N_WORDS, int(rng.integers(1, 400))) for _ in range(Q)]
        queries[3], queries[9], queries[12], queries[16] = C.Q2, C.Q1, {}, C.Q2
    d_w, d_v, d_n = _pack_queries(queries, 400)
    slots, n_out = db.dev.detect_relocalisation_candidates_batch_device(d_w, d_v, d_n, out_cap=64)
    torch.cuda.synchronize()
    slots, n_out = slots.cpu().numpy(), n_out.cpu().numpy()
    results = []
    for i, q in enumerate(queries):
        expect = db.model.DetectRelocalisationCandidates(q)
        got = db.dev.ids_of(slots[i, : n_out[i]])
        assert got == expect, (i, got, expect)
        check_table(db.dev, db.model, q=i)
        assert single.dev.DetectRelocalisationCandidates(q) == got
        if len(orb.vocabulary.bow_arrays(q)[0]):
            a, b = db.dev.debug_last_query(i), single.dev.debug_last_query(0)
            for key in a:
                assert a[key].tobytes() == b[key].tobytes(), (i, key)
        results.append(got)
    if Q == 2:
        assert results == [[C.N], [C.N]]
    if Q == 17:
        assert results[3] == [C.B] and results[16] == [C.N] and results[12] == []
    # a single call after the batch sees the batch's state (N keeps its 900 U when Q1 was in the batch)
    assert db.DetectRelocalisationCandidates(C.Q2) == ([C.B] if Q == 1 else [C.N])
    # a short output row: the true count, and only out_cap ids written
    if Q == 17:
        rows = [i for i in range(Q) if n_out[i] >= 2]
        assert rows
        fresh, _ = _stale_db(40)
        s2, n2 = fresh.dev.detect_relocalisation_candidates_batch_device(d_w, d_v, d_n, out_cap=1)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(n2.cpu().numpy(), n_out)
        np.testing.assert_array_equal(s2.cpu().numpy()[:, 0][n_out > 0], slots[:, 0][n_out > 0])


def test_device_calls_order_the_next_call_without_a_synchronise():
    """add_batch_device and the batch query on the default stream, each followed at once, with
    no synchronise of the caller's, by a host call on the same handle: the handle itself orders
    them.  A big batch (Q = 64, 300 keyframes) keeps the device busy while the host call arrives;
    then a still larger Q, which regrows the query scratch under the same condition."""
    import torch

    rng = np.random.default_rng(53)
    N, nw = 300, 100000  # a sparse vocabulary: the scan's work is the same, the model's is small
    bows = [_random_bow(rng, nw, int(rng.integers(100, 501))) for _ in range(N)]
    d_w, d_v, d_n = _pack_queries(bows, 500)
    db = orb.KeyFrameDatabase(flat_vocabulary(nw), 512, N * 500)
    model = ModelDatabase()
    db.add_batch_device(list(range(N)), d_w, d_v, d_n)
    for k in range(N):
        model.add(k, bows[k])
    q0 = _perturbed(rng, bows[7], nw, 0.8)
    assert db.DetectRelocalisationCandidates(q0) == model.DetectRelocalisationCandidates(q0)  # after the add
    check_table(db, model)
    for k in range(0, N, 3):
        nb = [(k * 7 + j) % N for j in range(1, 6)]
        db.set_covisible(k, nb)
        model.set_covisible(k, nb)
    for Q in (64, 96):
        queries = [_perturbed(rng, bows[int(rng.integers(0, N))], nw, 0.6) for _ in range(Q)]
        q_w, q_v, q_n = _pack_queries(queries, 700)
        slots, n_out = db.detect_relocalisation_candidates_batch_device(q_w, q_v, q_n, out_cap=16)
        q1 = _perturbed(rng, bows[11], nw, 0.8)
        got = db.DetectRelocalisationCandidates(q1)  # no torch synchronise in between
        expect = [model.DetectRelocalisationCandidates(q) for q in queries]
        assert got == model.DetectRelocalisationCandidates(q1)
        check_table(db, model)
        torch.cuda.synchronize()
        slots, n_out = slots.cpu().numpy(), n_out.cpu().numpy()
        assert [db.ids_of(slots[i, : min(16, n_out[i])]) for i in range(Q)] == [e[:16] for e in expect]
        assert n_out.tolist() == [len(e) for e in expect]
        db.erase(int(Q))  # a host call that changes the slots, again right after device work
        model.erase(int(Q))
        slots, n_out = db.detect_relocalisation_candidates_batch_device(q_w, q_v, q_n, out_cap=16)
        if Q == 96:
            db.clear()
        torch.cuda.synchronize()
        expect = [model.DetectRelocalisationCandidates(q) for q in queries]
        assert n_out.cpu().numpy().tolist() == [len(e) for e in expect]
    assert len(db) == 0


def test_queries_longer_than_the_lds_stage():
    """Queries of 2048 words are staged in LDS, of 2049 and 6000 searched in HBM; keyframes of 1,
    64, 65 and 300 words (1, 1, 2 and more 64-entry groups).  Host calls and one batch whose row
    capacity is 8192, against the model."""
    import torch

    rng = np.random.default_rng(61)
    nw = 100000
    db = Lockstep(nw, max_keyframes=64, max_entries=40000)
    single = orb.KeyFrameDatabase(flat_vocabulary(nw), 64, 40000)
    big = _random_bow(rng, nw, 6000)
    for k, n in enumerate((1, 64, 65, 300, 2048, 2049, 6000)):
        w = np.sort(rng.choice(big[0], n, replace=False))
        v = rng.random(n) + 1e-3
        db.add(k, (w, v / v.sum()))
        single.add(k, (w, v / v.sum()))
        db.set_covisible(k, [(k + 1) % 7, (k + 3) % 7])
        single.set_covisible(k, [(k + 1) % 7, (k + 3) % 7])
    queries = [(big[0][:n].copy(), big[1][:n] / big[1][:n].sum()) for n in (2048, 2049, 6000, 1, 8192 - 6000)]
    queries[4] = _random_bow(rng, nw, 8192)
    d_w, d_v, d_n = _pack_queries(queries, 8192)
    slots, n_out = single.detect_relocalisation_candidates_batch_device(d_w, d_v, d_n, out_cap=8)
    torch.cuda.synchronize()
    slots, n_out = slots.cpu().numpy(), n_out.cpu().numpy()
    for i, q in enumerate(queries):
        got = db.DetectRelocalisationCandidates(q)
        assert single.ids_of(slots[i, : n_out[i]]) == got, i
        check_table(single, db.model, q=i)
        db.DetectLoopCandidates(q, [3], 0.0)
    assert n_out[:3].min() >= 1


# ---- extract-side chain ---------------------------------------------------------------------------
def test_transform_add_query_match_chain():
    """random vocabulary -> transform_batch_device (32 frames x 200 descriptors) -> add_batch_device
    (24 keyframes) -> batch relocalisation query (all 32 frames) -> batched SearchByBoW(KF, F) on
    the returned candidates.  The model is fed the BowVectors read back from the device."""
    import torch

    import scenes as S
    from oracle_lib import OracleMatcher
    from orbslam_jpminipc_amd.views import FeatureVector, View
    from vocab_util import random_vocabulary

    rng = np.random.default_rng(41)
    B, NKF, n = 32, 24, 200
    base = [S.view(rng, n) for _ in range(4)]
    views = [View(base[b % 4].kps.copy(), S.perturb(rng, base[b % 4].desc, 12), (0, S.W, 0, S.H)) for b in range(B)]
    kps = np.zeros((B, n, 28), np.uint8)
    desc = np.zeros((B, n, 32), np.uint8)
    for b, v in enumerate(views):
        kps[b] = np.frombuffer(np.ascontiguousarray(v.kps).tobytes(), np.uint8).reshape(n, 28)
        desc[b] = v.desc
    d_kps, d_desc = torch.from_numpy(kps).cuda(), torch.from_numpy(desc).cuda()
    d_cnt = torch.full((B,), n, dtype=torch.int32, device="cuda")
    voc = orb.ORBVocabulary.from_arrays(8, 3, 0, 0, *random_vocabulary(8, 3, seed=3))
    fv = voc.transform_batch_device(d_desc, d_cnt, 1)
    db = orb.KeyFrameDatabase(voc, 64, 64 * n)
    kf_ids = [1000 + 3 * b for b in range(NKF)]
    db.add_batch_device(kf_ids, fv["bow_words"], fv["bow_values"], fv["bow_n"])
    for b in range(NKF):
        db.set_covisible(kf_ids[b], [kf_ids[(b + 4) % NKF], kf_ids[(b + 1) % NKF]])
    slots, n_out = db.detect_relocalisation_candidates_batch_device(fv["bow_words"], fv["bow_values"], fv["bow_n"], 32)
    torch.cuda.synchronize()
    assert len(db) == NKF
    bw, bv, bn = (fv[k].cpu().numpy() for k in ("bow_words", "bow_values", "bow_n"))
    bows = [(bw[b, : bn[b]].view(np.uint32), bv[b, : bn[b]]) for b in range(B)]
    model = ModelDatabase()
    for b in range(NKF):
        model.add(kf_ids[b], bows[b])
        model.set_covisible(kf_ids[b], [kf_ids[(b + 4) % NKF], kf_ids[(b + 1) % NKF]])
    slots, n_out = slots.cpu().numpy(), n_out.cpu().numpy()
    pa, pb = [], []
    for b in range(B):
        expect = model.DetectRelocalisationCandidates(bows[b])
        assert db.ids_of(slots[b, : n_out[b]]) == expect and expect, b
        check_table(db, model, q=b)
        for s in slots[b, : n_out[b]]:
            pa.append(int(s))  # slot = frame index of the batch: the ids were added in frame order
            pb.append(b)
    assert set(pa) <= set(range(NKF)) and len(pa) >= B
    # the pairwise scores of LoopClosing.cc:138-150 on the same device vectors
    t = lambda a: torch.tensor(a, dtype=torch.int32, device="cuda")  # noqa: E731
    sc = voc.score_pairs_device(fv["bow_words"], fv["bow_values"], fv["bow_n"], t(pb), t(pa))
    m, nm = orb.ORBmatcher(0.75, True).search_by_bow_batch_device(False, d_kps, d_desc, d_cnt, fv, t(pa), t(pb))
    torch.cuda.synchronize()
    sc, m, nm = sc.cpu().numpy(), m.cpu().numpy(), nm.cpu().numpy()
    assert bits(sc).tolist() == bits([l1_score(bow_items(bows[b]), bow_items(bows[a])) for a, b in zip(pa, pb)]).tolist()
    nodes, off, feat, fvn = (fv[k].cpu().numpy() for k in ("fv_nodes", "fv_offsets", "fv_features", "fv_n"))
    fvs = [FeatureVector(nodes[b, : fvn[b]].view(np.uint32), off[b, : fvn[b] + 1], feat[b, : off[b, fvn[b]]])
           for b in range(B)]
    o = OracleMatcher(0.75, True)
    for p in range(0, len(pa), max(1, len(pa) // 8)):
        no, mo = o.SearchByBoW_KF_F(views[pa[p]], None, fvs[pa[p]], views[pb[p]], fvs[pb[p]])
        assert nm[p] == no
        np.testing.assert_array_equal(m[p, :n], mo)
    assert nm.max() > 20


# ---- errors ------------------------------------------------------------------------------------------
def _raises(code, text, fn):
    with pytest.raises(orb.OrbError) as e:
        fn()
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_errors():
    import torch

    voc = flat_vocabulary(100000)
    l2 = flat_vocabulary(1000, scoring=1)
    _raises(_native.ORB_EINVAL, "L1_NORM", lambda: orb.KeyFrameDatabase(l2, 16, 100))
    _raises(_native.ORB_EINVAL, "L1_NORM", lambda: l2.score({1: 1.0}, {1: 1.0}))
    z = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    _raises(_native.ORB_EINVAL, "L1_NORM", lambda: l2.score_pairs_device(
        z, torch.zeros((2, 4), dtype=torch.float64, device="cuda"), z[:, 0], z[:, 0], z[:, 0]))
    db = orb.KeyFrameDatabase(voc, 16, 20000)
    _raises(_native.ORB_EINVAL, "ascending", lambda: db.add(0, ([3, 2], [0.5, 0.5])))
    _raises(_native.ORB_EINVAL, "ascending", lambda: db.add(0, ([3, 3], [0.5, 0.5])))
    _raises(_native.ORB_EINVAL, "word id 100000", lambda: db.add(0, ([3, 100000], [0.5, 0.5])))
    _raises(_native.ORB_EINVAL, "ascending", lambda: db.DetectRelocalisationCandidates(([3, 2], [0.5, 0.5])))
    _raises(_native.ORB_ENOTSUP, "8192", lambda: db.add(0, (np.arange(8193), np.ones(8193))))
    assert len(db) == 0
    db.add(0, {5: 1.0})
    big = np.full(8192, 2.0 ** -13)
    big[5] = 1.0
    db.add(1, (np.arange(8192), big))
    _raises(_native.ORB_EINVAL, "already live", lambda: db.add(0, {6: 1.0}))
    w, v = np.array([5], np.uint32), np.array([1.0])
    lib = orb.hip_lib()
    for bad in (16, -1):
        _raises(_native.ORB_EINVAL, "out of range", lambda: _native.check(
            lib.orb_kfdb_add(db._h, bad, _native.ptr(w), _native.ptr(v), 1)))
    _raises(_native.ORB_EINVAL, "out of range", lambda: _native.check(
        lib.orb_kfdb_set_covisible(db._h, 0, _native.ptr(np.array([16], np.int32)), 1)))
    _raises(_native.ORB_EINVAL, "[0, 10]", lambda: db.set_covisible(0, list(range(11))))
    assert len(db) == 2
    # a too-small out_cap: ORB_ERANGE and the count needed, nothing truncated silently
    out = np.full(4, -7, np.int32)
    n = ctypes.c_int(-1)
    q = np.array([5], np.uint32)
    _raises(_native.ORB_ERANGE, "out_cap", lambda: _native.check(lib.orb_kfdb_detect_relocalisation_candidates(
        db._h, _native.ptr(q), _native.ptr(v), 1, _native.ptr(out), 1, ctypes.byref(n))))
    assert n.value == 2 and (out == -7).all()
    _raises(_native.ORB_ERANGE, "out_cap", lambda: _native.check(lib.orb_kfdb_detect_loop_candidates(
        db._h, _native.ptr(q), _native.ptr(v), 1, None, 0, 0.0, _native.ptr(out), 1, ctypes.byref(n))))
    assert n.value == 2
    assert db.DetectRelocalisationCandidates({5: 1.0}) == [0, 1]
    db.erase(3)  # not live: a no-op
    db.erase(0)
    assert db.DetectRelocalisationCandidates({5: 1.0}) == [1] and len(db) == 1
