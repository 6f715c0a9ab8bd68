"""The vocabulary oracle (oracle/orb_oracle_voc.cpp) and the Python models (vocab_util.PyVocabulary,
kfdb_model.l1_score) against what the reference's own DBoW2 returned, as recorded in
tests/golden/ref_dbow2_* (tests/ref_dbow2_fixture.py; scripts/gen_ref_dbow2_golden.py).

Only test_fixtures_are_what_the_reference_returns needs the compiled reference
(oracle/_ref/dbow2_ref_*): it reruns the driver on the fixtures' inputs and requires the
committed bytes.  Everything else runs from the fixtures alone.

Every comparison is exact: words, nodes and feature lists as integers, doubles by their bits.
The recorded reference is the contracted build (the reference compiles DBoW2 -O3 -march=native);
test_only_the_l2_norm_contracts covers what the plain build gave.
"""
import ctypes

import numpy as np
import pytest

import orbslam_jpminipc_amd as orb
import ref_dbow2_fixture as rf
from kfdb_model import l1_score
from oracle_lib import _p, lib
from orbslam_jpminipc_amd import _native
from vocab_util import OracleVocabulary, PyVocabulary, hamming_matrix


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64).tolist()


def _check_oracle_case(ov, c):
    bw, bv, fn, fo, ff = ov.transform(c.feats, c.levelsup)
    assert bw.tolist() == c.bow_words.tolist(), c.label
    assert bits(bv) == bits(c.bow_vals), c.label
    assert fn.tolist() == c.fv_nodes.tolist(), c.label
    assert fo.tolist() == c.fv_offsets.tolist(), c.label
    assert ff.tolist() == c.fv_feats.tolist(), c.label
    for i, f in enumerate(c.feats):
        w, wt, nid = ov.transform_one(f, c.levelsup)
        assert (w, bits([wt]), nid) == (int(c.feat_word[i]), bits([c.feat_weight[i]]), int(c.feat_nid[i])), (c.label, i)


# ---- the fixtures themselves --------------------------------------------------------------------
def test_fixtures_are_what_the_reference_returns():
    """Rerun the reference's DBoW2 on the fixtures' inputs: the committed outputs, byte for byte."""
    if not rf.binaries_present():
        pytest.skip("oracle/_ref/dbow2_ref_* are not built: build() makes them only where the reference tree is present")
    for name in rf.VOCABS:
        fx = rf.vocabulary_fixture(name)
        out = rf.record_vocabulary(fx.k, fx.L, *fx.arrays, fx.ws, fx.frames, fx.lvls)
        for key in rf.OUT_KEYS:
            assert out[key].dtype == fx.z[key].dtype and out[key].tobytes() == fx.z[key].tobytes(), (name, key)
    fx = rf.vocabulary_fixture("v1")
    text, rs = rf.record_resave(fx.k, fx.L, *fx.arrays, fx.frames, fx.lvls)
    assert text == rf.RESAVED.read_bytes()
    for key in rf.OUT_KEYS:
        assert rs[key].dtype == fx.z["rs_" + key].dtype and rs[key].tobytes() == fx.z["rs_" + key].tobytes(), key
    bows, _, pairs, scores, _ = rf.score_fixture()
    assert rf.record_scores(bows, pairs).tobytes() == scores.tobytes()
    dpairs, dist = rf.distance_fixture()
    assert rf.record_distances(dpairs).tobytes() == dist.tobytes()


@pytest.mark.parametrize("name", rf.VOCABS)
def test_fixture_stays_where_the_reference_is_defined(name):
    """Every leaf at depth L (no `nid` left unwritten: the driver's 0xFFFFFFFF never comes back),
    a tie at every level and stop-word features present (the meta data and the weights say so)."""
    fx = rf.vocabulary_fixture(name)
    parent, leaf, _, weight = fx.arrays
    depth = np.zeros(len(parent) + 1, np.int64)
    for i, p in enumerate(parent):
        depth[i + 1] = depth[p] + 1
    nchild = np.bincount(parent, minlength=len(parent) + 1)
    assert (depth[1:][leaf > 0] == fx.L).all() and ((nchild[1:] == 0) == (leaf > 0)).all()
    assert fx.lvls == [0, 1, fx.L - 1, fx.L, fx.L + 2]
    assert [len(f) for f in fx.frames[:6]] == [0, 1, 63, 64, 65, 300]
    assert rf.UNWRITTEN not in fx.z["feat_nid"].tolist()
    stop = fx.frame("stop")
    for c in fx.cases():
        assert len(c.feat_word) == len(c.feats)
        if c.fi == stop:
            assert len(c.feats) > 0 and len(c.bow_words) == 0 and len(c.fv_nodes) == 0 and (c.feat_weight == 0).all()
        if c.levelsup >= fx.L:
            assert (c.feat_nid == 0).all()  # nid level <= 0: the root
    assert any((c.feat_weight == 0).any() and (c.feat_weight > 0).any() for c in fx.cases(0))


# ---- the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rf.VOCABS)
def test_oracle_transform_is_the_reference_s(name, tmp_path):
    """load_text (the file the reference loaded), create, transform and transform_one."""
    fx = rf.vocabulary_fixture(name)
    for wi, (weighting, scoring) in enumerate(fx.ws):
        path = tmp_path / f"voc_{wi}.txt"
        rf.write_vocabulary_text(path, fx.k, fx.L, scoring, weighting, *fx.arrays)
        loaded = OracleVocabulary.load_text(path)
        created = OracleVocabulary.create(fx.k, fx.L, scoring, weighting, *fx.arrays)
        want = [fx.k, fx.L, scoring, weighting, len(fx.arrays[0]) + 1, int(fx.arrays[1].sum())]
        assert loaded.info().tolist() == want and created.info().tolist() == want
        for c in fx.cases(wi):
            _check_oracle_case(loaded, c)
            _check_oracle_case(created, c)


def test_only_the_l2_norm_contracts():
    """The oracle's header claims that of the whole path only BowVector::normalize's L2
    `norm += v * v` contracts under the reference's -O3 -march=native.  The two reference builds
    (contraction off / fast) agree byte for byte except in L2-normalised values (the generator and
    the fixture check assert it of every array); the fixtures hold BowVectors in which they do
    differ, and there the oracle gives the contracted build's values, not the plain build's."""
    differing = 0
    for name in rf.VOCABS:
        fx = rf.vocabulary_fixture(name)
        for wi, (weighting, scoring) in enumerate(fx.ws):
            ov = OracleVocabulary.create(fx.k, fx.L, scoring, weighting, *fx.arrays)
            for c in fx.cases(wi):
                if scoring != rf.L2_NORM:
                    assert not c.plain_differs, c.label
                if c.plain_differs and c.li == 0:
                    differing += 1
                    assert len(c.plain_bow_vals) == len(c.bow_vals) and bits(c.plain_bow_vals) != bits(c.bow_vals)
                    got = ov.transform(c.feats, c.levelsup)[1]
                    assert bits(got) == bits(c.bow_vals) and bits(got) != bits(c.plain_bow_vals), c.label
    assert differing >= 1


def test_oracle_loads_the_file_the_reference_saved(tmp_path):
    """saveToTextFile's own output for V1 (six-digit weights, double spaces, a trailing newline),
    loaded as it is and with the newline stripped: both transform as the reference did after
    loading the stripped file, its defined half (the raw file gives the reference a ghost node)."""
    fx = rf.vocabulary_fixture("v1")
    text = rf.RESAVED.read_bytes()
    assert text.endswith(b"\n") and not text.endswith(b"\n\n") and text.startswith(b"4 4  0 0\n")
    (tmp_path / "stripped.txt").write_bytes(text[:-1])
    raw, stripped = OracleVocabulary.load_text(rf.RESAVED), OracleVocabulary.load_text(tmp_path / "stripped.txt")
    want = [fx.k, fx.L, 0, 0, len(fx.arrays[0]) + 1, int(fx.arrays[1].sum())]
    assert raw.info().tolist() == want and stripped.info().tolist() == want
    rounded = False
    for c in fx.resave_cases():
        _check_oracle_case(raw, c)
        _check_oracle_case(stripped, c)
        exact = fx.out.case(c.fi, fx.ws.index((0, 0)), c.li)
        rounded |= bits(exact.feat_weight) != bits(c.feat_weight)
    assert rounded  # the six-digit weights are not the exact ones: the file was really reparsed


def test_product_loader_parses_the_reference_s_file(tmp_path):
    """orb_vocabulary_load_text on the same two files.  Its header parse (the double space) runs
    before the device is looked up, so without a device it ends in ORB_EDEVICE, never in
    ORB_EINVAL; with one, the tree has the reference's counts."""
    fx = rf.vocabulary_fixture("v1")
    (tmp_path / "stripped.txt").write_bytes(rf.RESAVED.read_bytes()[:-1])
    L = orb.hip_lib()
    for path in (rf.RESAVED, tmp_path / "stripped.txt"):
        h = ctypes.c_void_p()
        st = L.orb_vocabulary_load_text(str(path).encode(), 0, ctypes.byref(h))
        assert st in (_native.ORB_OK, _native.ORB_EDEVICE), (st, L.orb_last_error())
        if st == _native.ORB_OK:
            info = np.zeros(7, np.int32)
            assert L.orb_vocabulary_info(h, _p(info)) == 0
            assert info.tolist() == [fx.k, fx.L, 0, 0, len(fx.arrays[0]) + 1, int(fx.arrays[1].sum()), fx.L]
            L.orb_vocabulary_destroy(h)


# ---- the Python models --------------------------------------------------------------------------
class _MemoPyVocabulary(PyVocabulary):
    """PyVocabulary with its descents remembered: transform1 depends on the tree, the feature and
    levelsup only, and the cases repeat each of them for every weighting/scoring pair."""

    def __init__(self, memo, *a):
        super().__init__(*a)
        self.memo = memo

    def transform1(self, f, levelsup):
        key = (bytes(f), levelsup)
        if key not in self.memo:
            self.memo[key] = super().transform1(f, levelsup)
        return self.memo[key]


@pytest.mark.parametrize("name", rf.VOCABS)
def test_python_restatement_is_the_reference_s(name):
    fx = rf.vocabulary_fixture(name)
    memo = {}
    for wi, (weighting, scoring) in enumerate(fx.ws):
        pv = _MemoPyVocabulary(memo, fx.k, fx.L, scoring, weighting, *fx.arrays)
        for c in fx.cases(wi):
            bow, fv = pv.transform(c.feats, c.levelsup)
            assert list(bow.keys()) == c.bow_words.tolist(), c.label
            assert bits(list(bow.values())) == bits(c.bow_vals), c.label
            assert list(fv.keys()) == c.fv_nodes.tolist() and list(fv.values()) == c.fv_lists, c.label
            for i, f in enumerate(c.feats):
                w, wt, nid = pv.transform1(f, c.levelsup)
                assert (w, bits([wt]), nid) == (int(c.feat_word[i]), bits([c.feat_weight[i]]), int(c.feat_nid[i]))


def test_l1_score_model_is_the_reference_s():
    """kfdb_model.l1_score over every ordered pair of the score set, by bits: the empty vector,
    one word, 300 features, identical pairs, and disjoint pairs, whose score is -0.0."""
    bows, labels, pairs, scores, meta = rf.score_fixture()
    assert len(pairs) == len(bows) ** 2
    items = [list(zip(w.tolist(), v.tolist())) for w, v in bows]
    for (a, b), s in zip(pairs.tolist(), scores):
        assert bits([l1_score(items[a], items[b])]) == bits([s]), (labels[a], labels[b])
    minus_zero = bits([-0.0])
    for x, y in meta["disjoint"]:
        a, b = labels.index(x), labels.index(y)
        assert len(bows[a][0]) and len(bows[b][0]) and not set(bows[a][0].tolist()) & set(bows[b][0].tolist())
        assert bits([scores[a * len(bows) + b]]) == minus_zero and bits([scores[b * len(bows) + a]]) == minus_zero
    assert any(len(w) == 0 for w, _ in bows) and any(len(w) == 1 for w, _ in bows)
    assert all(scores[a * len(bows) + a] > 0.99 for a in range(len(bows)) if len(bows[a][0]))  # identical pairs


def test_descriptor_distance_is_forb_distance():
    dpairs, dist = rf.distance_fixture()
    assert len(dpairs) == 66 and 0 in dist and 256 in dist
    O, H = lib(), orb.hip_lib()
    for (a, b), d in zip(dpairs, dist.tolist()):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert O.oracle_descriptor_distance(_p(a), _p(b)) == d
        assert H.orb_descriptor_distance(_p(a), _p(b)) == d  # host code: no device needed
        assert int(hamming_matrix(a[None], b[None])[0, 0]) == d
