"""GPU parity of the vocabulary path (csrc/orb_voc.hip), the BoW score (csrc/orb_kfdb.hip) and the
descriptor distance against what the reference's own DBoW2 returned, as recorded in
tests/golden/ref_dbow2_* (tests/ref_dbow2_fixture.py).  Nothing here reads the CPU oracle or the
compiled reference: the fixtures and the product only.

Four vocabularies (k, L = 4, 4 trained on real descriptors with every weighting x scoring;
17, 2 dense; 20, 2 and 10, 3 sparse and tie-heavy), frames of 0, 1, 63, 64, 65 and 300 features
plus a frame of stop-word features only, levelsup 0, 1, L - 1, L and L + 2.  Every comparison is
exact: integers as integers, doubles by their bits.
"""
import numpy as np
import pytest

import orbslam_jpminipc_amd as orb
import ref_dbow2_fixture as rf

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64).tolist()


def _vocabulary(fx, wi, how, tmp_path):
    weighting, scoring = fx.ws[wi]
    if how == "create":
        gv = orb.ORBVocabulary.from_arrays(fx.k, fx.L, scoring, weighting, *fx.arrays)
    else:
        path = tmp_path / f"voc_{wi}.txt"
        rf.write_vocabulary_text(path, fx.k, fx.L, scoring, weighting, *fx.arrays)
        gv = orb.ORBVocabulary()
        assert gv.loadFromTextFile(str(path)), gv.last_error
    assert (gv.k, gv.L, gv.scoring, gv.weighting, gv.n_nodes, gv.n_words, gv.height) == (
        fx.k, fx.L, scoring, weighting, len(fx.arrays[0]) + 1, int(fx.arrays[1].sum()), fx.L)
    return gv


def _check_host_transform(gv, c):
    bow, fv = gv.transform(c.feats, c.levelsup)
    assert list(bow.keys()) == c.bow_words.tolist(), c.label
    assert bits(list(bow.values())) == bits(c.bow_vals), c.label
    assert fv.nodes.tolist() == c.fv_nodes.tolist() and fv.offsets.tolist() == c.fv_offsets.tolist(), c.label
    assert fv.features.tolist() == c.fv_feats.tolist(), c.label


def _check_features_device(gv, c, d_feats):
    import torch

    w, wt, nd = gv.transform_features_device(d_feats, c.levelsup)
    torch.cuda.synchronize()
    assert w.cpu().numpy().view(np.uint32).tolist() == c.feat_word.tolist(), c.label
    assert bits(wt.cpu().numpy()) == bits(c.feat_weight), c.label
    assert nd.cpu().numpy().view(np.uint32).tolist() == c.feat_nid.tolist(), c.label


@pytest.mark.parametrize("how", ["create", "load_text"])
@pytest.mark.parametrize("name", rf.VOCABS)
def test_transform_is_the_reference_s(name, how, tmp_path):
    """orb_vocabulary_create / _load_text, then orb_vocabulary_transform and
    orb_vocabulary_transform_features_device on every recorded case."""
    import torch

    fx = rf.vocabulary_fixture(name)
    d_frames = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in fx.frames]
    for wi in range(len(fx.ws)):
        gv = _vocabulary(fx, wi, how, tmp_path)
        for c in fx.cases(wi):
            _check_host_transform(gv, c)
            _check_features_device(gv, c, d_frames[c.fi])
        gv.close()


@pytest.mark.parametrize("name", rf.VOCABS)
def test_transform_batch_is_the_reference_s(name):
    """orb_vocabulary_transform_batch_device: the frames of 0, 1, 63, 64, 65 and 300 features
    (and the stop-word frame) in one batch, for every weighting/scoring pair and levelsup."""
    import torch

    fx = rf.vocabulary_fixture(name)
    sel = [fx.frame(n) for n in ("n0", "n1", "n63", "n64", "n65", "n300", "stop")]
    B, cap = len(sel), 300
    D = np.zeros((B, cap, 32), np.uint8)
    counts = np.array([len(fx.frames[f]) for f in sel], np.int32)
    assert counts.tolist()[:6] == [0, 1, 63, 64, 65, 300]
    for b, f in enumerate(sel):
        D[b, :counts[b]] = fx.frames[f]
    d_D, d_counts = torch.from_numpy(D).cuda(), torch.from_numpy(counts).cuda()
    for wi in range(len(fx.ws)):
        gv = orb.ORBVocabulary.from_arrays(fx.k, fx.L, fx.ws[wi][1], fx.ws[wi][0], *fx.arrays)
        for li, levelsup in enumerate(fx.lvls):
            out = gv.transform_batch_device(d_D, d_counts, levelsup)
            torch.cuda.synchronize()
            o = {k: v.cpu().numpy() for k, v in out.items()}
            for b, f in enumerate(sel):
                c = fx.out.case(f, wi, li)
                label = f"{name} frame={fx.frame_names[f]} ws={fx.ws[wi]} lu={levelsup}"
                n, nb, nf = int(counts[b]), int(o["bow_n"][b]), int(o["fv_n"][b])
                assert o["feat_word"][b, :n].view(np.uint32).tolist() == c.feat_word.tolist(), label
                assert bits(o["feat_weight"][b, :n]) == bits(c.feat_weight), label
                assert o["feat_node"][b, :n].view(np.uint32).tolist() == c.feat_nid.tolist(), label
                assert o["bow_words"][b, :nb].view(np.uint32).tolist() == c.bow_words.tolist(), label
                assert bits(o["bow_values"][b, :nb]) == bits(c.bow_vals), label
                assert o["fv_nodes"][b, :nf].view(np.uint32).tolist() == c.fv_nodes.tolist(), label
                assert o["fv_offsets"][b, :nf + 1].tolist() == c.fv_offsets.tolist(), label
                assert o["fv_features"][b, :len(c.fv_feats)].tolist() == c.fv_feats.tolist(), label
        gv.close()


def test_resaved_file_loads_as_the_reference_loaded_it(tmp_path):
    """The file the reference's saveToTextFile wrote for V1, as it is (trailing newline) and
    stripped: both transform as the reference did after loading the stripped file."""
    fx = rf.vocabulary_fixture("v1")
    (tmp_path / "stripped.txt").write_bytes(rf.RESAVED.read_bytes()[:-1])
    for path in (rf.RESAVED, tmp_path / "stripped.txt"):
        gv = orb.ORBVocabulary()
        assert gv.loadFromTextFile(str(path)), gv.last_error
        assert (gv.k, gv.L, gv.scoring, gv.weighting, gv.n_nodes, gv.n_words) == (
            fx.k, fx.L, 0, 0, len(fx.arrays[0]) + 1, int(fx.arrays[1].sum()))
        for c in fx.resave_cases():
            _check_host_transform(gv, c)
        gv.close()


def test_score_is_the_reference_s():
    """orb_vocabulary_score and orb_vocabulary_score_pairs_device over every ordered pair of the
    score set (empty, one word, 300 features, identical and disjoint pairs), by bits: the disjoint
    pairs' -0.0 included."""
    import torch

    bows, labels, pairs, scores, meta = rf.score_fixture()
    fx = rf.vocabulary_fixture("v4")
    gv = orb.ORBVocabulary.from_arrays(fx.k, fx.L, 0, 0, *fx.arrays)
    assert max(int(w.max()) for w, _ in bows if len(w)) < gv.n_words
    a, b = labels.index(meta["disjoint"][1][0]), labels.index(meta["disjoint"][1][1])
    assert bits([scores[a * len(bows) + b]]) == bits([-0.0])
    for (x, y), s in zip(pairs.tolist(), scores):
        assert bits([gv.score(bows[x], bows[y])]) == bits([s]), (labels[x], labels[y])
    B, cap = len(bows), max(len(w) for w, _ in bows)
    bw, bv = np.zeros((B, cap), np.uint32), np.zeros((B, cap), np.float64)
    bn = np.array([len(w) for w, _ in bows], np.int32)
    for f, (w, v) in enumerate(bows):
        bw[f, :len(w)], bv[f, :len(w)] = w, v
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    got = gv.score_pairs_device(t(bw.view(np.int32)), t(bv), t(bn), t(pairs[:, 0].astype(np.int32)),
                                t(pairs[:, 1].astype(np.int32)))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    bad = [(labels[x], labels[y], g, s) for (x, y), g, s in zip(pairs.tolist(), got, scores) if bits([g]) != bits([s])]
    assert not bad, bad[:5]


def test_descriptor_distance_is_forb_distance():
    dpairs, dist = rf.distance_fixture()
    for (a, b), d in zip(dpairs, dist.tolist()):
        assert orb.ORBmatcher.DescriptorDistance(np.ascontiguousarray(a), np.ascontiguousarray(b)) == d
