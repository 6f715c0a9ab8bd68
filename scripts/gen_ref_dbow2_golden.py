#!/usr/bin/env python3
"""Writes tests/golden/ref_dbow2_{v1,v2,v3,v4,score,distance}.npz and ref_dbow2_v1_resaved.txt:
what the reference's own DBoW2, compiled into oracle/_ref/dbow2_ref_{fma,plain} by
__graft_entry__.build_ref_dbow2(), returns for four vocabularies (tests/ref_dbow2_fixture.py
describes the files).  Needs the reference tree; the tests read the fixtures alone.

Inputs stay where the reference is defined: the vocabulary text has no trailing newline (its
loader would make a ghost node of it) and every leaf sits at depth L (a shallower leaf leaves
`nid` unwritten); vocabularies come from tests/vocab_util.py, not from the reference's create(),
which reads a released cv::Mat when a k-means iteration leaves a cluster empty.
No case is dropped for these reasons: the script asserts both properties of every vocabulary it
writes.

Before a fixture is written the script also asserts what the tests rely on: a descent with an
equal-distance tie at every tree level, a feature on a stop word, a frame of stop-word features
only (an empty BowVector from a non-empty frame), for the score set a disjoint pair of non-empty
vectors, and no `nid` left unwritten.
"""
import json
import pathlib
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import ref_dbow2_fixture as rf  # noqa: E402
from vocab_util import build_vocabulary, hamming_matrix, random_vocabulary  # noqa: E402

GOLD = ROOT / "tests" / "golden"
ALL_WS = [(w, s) for s in range(6) for w in range(4)]  # (weighting, scoring)
FEW_WS = [(0, 0), (3, 1)]  # (TF_IDF, L1_NORM), (BINARY, L2_NORM)
COUNTS = [0, 1, 63, 64, 65, 300]


def depths(parent):
    d = np.zeros(len(parent) + 1, np.int32)
    for i, p in enumerate(parent):
        d[i + 1] = d[p] + 1
    return d


def assert_defined(k, L, parent, is_leaf):
    """Every leaf at depth L, every inner node with children: where the reference is defined."""
    n = len(parent)
    nchild = np.bincount(parent, minlength=n + 1)
    d = depths(parent)
    assert nchild.max() <= k and nchild[0] >= 1
    for i in range(n):
        assert bool(is_leaf[i]) == (nchild[i + 1] == 0), ("leaf flag and children disagree", i + 1)
        assert not is_leaf[i] or d[i + 1] == L, ("leaf above depth L", i + 1, d[i + 1])
    assert all(parent[i] <= i for i in range(n))


def sparse_rows(rng, n, bits):
    out = np.zeros((n, 32), np.uint8)
    for i in range(n):
        for b in rng.choice(256, size=bits, replace=False):
            out[i, b // 8] |= np.uint8(1 << (b % 8))
    return out


def stop_some_words(arrays, seed, frac=0.15):
    """random_vocabulary has no stop words: zero the weight of a seeded share of the leaves."""
    parent, leaf, desc, weight = arrays
    rng = np.random.default_rng(seed)
    weight = weight.copy()
    weight[(leaf > 0) & (rng.random(len(leaf)) < frac)] = 0.0
    return parent, leaf, desc, weight


def reference_words(k, L, arrays, pool):
    """(word, weight) of every pool feature, from the reference itself."""
    with tempfile.TemporaryDirectory() as tmp:
        voc = pathlib.Path(tmp) / "voc.txt"
        rf.write_vocabulary_text(voc, k, L, 0, 0, *arrays)
        r = rf.run_transform(rf.BINARIES[0], voc, [pool], [0], tmp)[0, 0]
    return r["feat_word"], r["feat_weight"]


def tie_levels(arrays, pool, words):
    """Per feature, the levels (1-based) at which the reference's own path had another child at
    the minimum distance."""
    parent, leaf, desc, _ = arrays
    leaves = np.nonzero(leaf)[0] + 1  # word id -> node id
    kids = {}
    for i, p in enumerate(parent):
        kids.setdefault(int(p), []).append(i + 1)
    out = []
    for f, w in zip(pool, words):
        node, path = int(leaves[w]), []
        while node != 0:
            path.append(node)
            node = int(parent[node - 1])
        path.reverse()
        lv = set()
        for level, node in enumerate(path, 1):
            sib = kids[int(parent[node - 1])]
            d = hamming_matrix(f[None], desc[np.array(sib) - 1])[0]
            assert d[sib.index(node)] == d.min()
            if (d == d.min()).sum() >= 2:
                lv.add(level)
        out.append(lv)
    return out


def choose_frames(L, pool, words, weights, ties):
    """Frames of 0, 1, 63, 64, 65 and 300 features, a frame of stop-word features only, and the
    300-feature frame's kept features split by word parity (a disjoint pair of BowVectors).
    Features with a tie at each level and stop-word features are moved to the front of the pool,
    so they fall into the small frames."""
    first = [int(np.nonzero(weights > 0)[0][0])]
    for level in range(1, L + 1):
        hit = [i for i, t in enumerate(ties) if level in t]
        assert hit, f"no tie at level {level} in the pool"
        first += hit[:3]
    stops = [int(i) for i in np.nonzero(weights == 0)[0]]
    assert len(stops) >= 3, "fewer than three pool features on stop words"
    first += stops[:3]
    seen, order = set(), []
    for i in first + list(range(len(pool))):
        if i not in seen:
            seen.add(i)
            order.append(i)
    assert len(order) >= sum(COUNTS)
    frames, names, at = [], [], 0
    for n in COUNTS:
        frames.append(order[at:at + n])
        names.append(f"n{n}")
        at += n
    frames.append(stops[:5])
    names.append("stop")
    big = frames[COUNTS.index(300)]
    frames.append([i for i in big if weights[i] > 0 and words[i] % 2 == 0])
    names.append("even")
    frames.append([i for i in big if weights[i] > 0 and words[i] % 2 == 1])
    names.append("odd")
    assert len(frames[-1]) > 5 and len(frames[-2]) > 5
    used = sorted({i for fr in frames[:len(COUNTS)] for i in fr})
    for level in range(1, L + 1):
        assert any(level in ties[i] for i in used), f"no tie at level {level} in the frames"
    assert any(weights[i] == 0 for i in used)
    return frames, names


def make_v1():
    """k = 4, L = 4 over the oracle's descriptors of a 320x240 synthetic frame, stop_frac 0.2;
    the first seed whose tree is complete."""
    import orbslam_jpminipc_amd as orb
    from oracle_lib import Oracle

    ora = Oracle(2000, 1.2, 8, 1, 20)
    imgs = orb.synth_stream(320, 240, stream=30, first=0, count=3)
    train = ora.extract(imgs[0])[1]
    pool = np.concatenate([ora.extract(imgs[1])[1], ora.extract(imgs[2])[1]])
    for seed in range(400):
        arrays = build_vocabulary(train, k=4, L=4, seed=seed, stop_frac=0.2)
        try:
            assert_defined(4, 4, arrays[0], arrays[1])
        except AssertionError:
            continue
        return arrays, pool, {"source": "build_vocabulary(oracle descriptors of synth_stream(320, 240, stream=30) "
                                        "frame 0, nfeatures 2000, k=4, L=4, stop_frac=0.2)", "seed": seed,
                              "train": len(train)}
    raise SystemExit("no seed gives a complete k=4, L=4 tree")


def make_random(k, L, bits, seed):
    arrays = stop_some_words(random_vocabulary(k, L, seed=seed, bits=bits), seed + 1000)
    rng = np.random.default_rng(seed + 2000)
    n = 1500
    pool = rng.integers(0, 256, size=(n, 32), dtype=np.uint8) if bits >= 256 else sparse_rows(rng, n, bits)
    return arrays, pool, {"source": f"random_vocabulary(k={k}, L={L}, bits={bits}) with 15% of the leaf weights "
                                    "zeroed; features drawn like the nodes", "seed": seed}


def write_vocabulary_fixture(name, k, L, arrays, pool, ws, meta, resave=False):
    assert_defined(k, L, arrays[0], arrays[1])
    words, weights = reference_words(k, L, arrays, pool)
    ties = tie_levels(arrays, pool, words)
    rows, names = choose_frames(L, pool, words, weights, ties)
    used = sorted({i for fr in rows for i in fr})  # the feature table: every pool row that a frame uses
    frame_rows = np.array([used.index(i) for fr in rows for i in fr], np.int32)
    frames = [pool[np.array(fr, np.int64)].reshape(-1, 32) for fr in rows]
    lvls = rf.levelsups(L)
    out = rf.record_vocabulary(k, L, *arrays, ws, frames, lvls)
    assert rf.UNWRITTEN not in out["feat_nid"], "the reference left a nid unwritten"
    fx_meta = dict(meta, frames=names, n_cases=len(frames) * len(ws) * len(lvls),
                   l2_bow_vectors=len(frames) * sum(1 for _, s in ws if s == rf.L2_NORM),
                   l2_bow_vectors_where_plain_differs=int(out["plain_differs"].sum()))
    data = dict(k=np.int32(k), L=np.int32(L), parent=arrays[0].astype(np.int32), is_leaf=arrays[1].astype(np.uint8),
                desc=arrays[2].astype(np.uint8), weight=arrays[3].astype(np.float64), ws=np.array(ws, np.int32),
                feats=pool[np.array(used, np.int64)].astype(np.uint8), frame_rows=frame_rows,
                counts=np.array([len(f) for f in frames], np.int32),
                levelsups=np.array(lvls, np.int32), **out)
    if resave:
        text, rs = rf.record_resave(k, L, *arrays, frames, lvls)
        rf.RESAVED.write_bytes(text)
        data.update({"rs_" + key: v for key, v in rs.items()})
    # the stop frame: not empty, yet an empty BowVector in every case
    si = names.index("stop")
    assert len(frames[si]) > 0 and not out["bow_n"][si * len(ws):(si + 1) * len(ws)].any()
    data["meta"] = np.array(json.dumps(fx_meta))
    np.savez_compressed(GOLD / f"ref_dbow2_{name}.npz", **data)
    print(name, fx_meta, (GOLD / f"ref_dbow2_{name}.npz").stat().st_size, "bytes")
    return fx_meta["l2_bow_vectors_where_plain_differs"]


def write_score_fixture():
    v1, v4 = rf.vocabulary_fixture("v1"), rf.vocabulary_fixture("v4")
    bows, labels = [], []
    for fx, names in ((v1, ["n0", "n1", "n63", "n300", "stop", "even", "odd"]), (v4, ["n1", "n300", "even", "odd"])):
        wi = fx.ws.index((0, 0))
        for nm in names:
            c = next(c for c in fx.cases(wi) if c.fi == fx.frame(nm) and c.li == 0)
            bows.append((c.bow_words.copy(), c.bow_vals.copy()))
            labels.append(f"{fx.name}:{nm}")
    assert len(bows[labels.index("v1:n0")][0]) == 0 and len(bows[labels.index("v1:stop")][0]) == 0
    assert len(bows[labels.index("v1:n1")][0]) == 1 and len(bows[labels.index("v4:n1")][0]) == 1
    for v in ("v1", "v4"):
        a, b = bows[labels.index(v + ":even")][0], bows[labels.index(v + ":odd")][0]
        assert len(a) > 3 and len(b) > 3 and not set(a.tolist()) & set(b.tolist())
        assert a.min() < b.max() and b.min() < a.max()  # interleaved: both lower_bound branches run
    pairs = np.array([(a, b) for a in range(len(bows)) for b in range(len(bows))], np.int32)
    scores = rf.record_scores(bows, pairs)
    d = scores[len(bows) * labels.index("v4:even") + labels.index("v4:odd")]
    assert d == 0.0 and np.signbit(d), "the disjoint pair does not score -0.0"
    meta = {"labels": labels, "scoring": "L1_NORM", "disjoint": [["v1:even", "v1:odd"], ["v4:even", "v4:odd"]]}
    np.savez_compressed(GOLD / "ref_dbow2_score.npz", bow_n=np.array([len(w) for w, _ in bows], np.int32),
                        bow_words=np.concatenate([w for w, _ in bows]).astype(np.uint32),
                        bow_vals=np.concatenate([v for _, v in bows]).astype(np.float64), pairs=pairs, scores=scores,
                        meta=np.array(json.dumps(meta)))
    print("score", len(bows), "vectors", len(pairs), "pairs", (GOLD / "ref_dbow2_score.npz").stat().st_size, "bytes")


def write_distance_fixture():
    rng = np.random.default_rng(99)
    a = rng.integers(0, 256, size=(66, 32), dtype=np.uint8)
    b = rng.integers(0, 256, size=(66, 32), dtype=np.uint8)
    b[64] = a[64]  # identical
    b[65] = ~a[65]  # complementary
    pairs = np.stack([a, b], 1)
    dist = rf.record_distances(pairs)
    assert dist[64] == 0 and dist[65] == 256
    np.savez_compressed(GOLD / "ref_dbow2_distance.npz", pairs=pairs, dist=dist.astype(np.int32))
    print("distance", len(pairs), "pairs", (GOLD / "ref_dbow2_distance.npz").stat().st_size, "bytes")


def main():
    if not rf.binaries_present():
        raise SystemExit("oracle/_ref/dbow2_ref_* are missing: run __graft_entry__.build() with the reference tree")
    arrays, pool, meta = make_v1()
    differing = write_vocabulary_fixture("v1", 4, 4, arrays, pool, ALL_WS, meta, resave=True)
    for name, (k, L, bits, seed) in (("v2", (17, 2, 256, 17)), ("v3", (20, 2, 16, 20)), ("v4", (10, 3, 24, 10))):
        arrays, pool, meta = make_random(k, L, bits, seed)
        differing += write_vocabulary_fixture(name, k, L, arrays, pool, FEW_WS, meta)
    # the oracle's claim that the L2 norm's `norm += v * v` contracts needs a case that shows it
    assert differing > 0, "no L2 BowVector in which the plain build differs from the contracted one"
    print("L2 BowVectors in which the plain build differs from the contracted one:", differing)
    write_score_fixture()
    write_distance_fixture()


if __name__ == "__main__":
    main()
