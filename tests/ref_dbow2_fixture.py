"""TEST INFRASTRUCTURE: the fixtures recorded from the reference's own DBoW2
(tests/golden/ref_dbow2_*.npz, written by scripts/gen_ref_dbow2_golden.py) and the code that
records them through the driver binaries oracle/_ref/dbow2_ref_{plain,fma}
(oracle/ref_dbow2/dbow2_ref.cpp).

A vocabulary fixture holds the tree (parent, leaf flag, descriptors, f64 weights), the
(weighting, scoring) pairs it was loaded with, the frames' descriptors, the levelsups, and for
every case (frame, weighting/scoring, levelsup) what the reference returned: BowVector,
FeatureVector, and the single-feature overload's (word, weight, nid).  The recorded reference is
`dbow2_ref_fma` (the reference builds DBoW2 -O3 -march=native); where `dbow2_ref_plain` gave other
BowVector values the case is flagged in `plain_differs` and the plain values are kept too.
The reference's BowVector does not depend on levelsup and its FeatureVector and single-feature
results do not depend on the weighting/scoring pair; that is asserted of every case while
recording, and each is then stored once (BowVectors per (frame, pair), the rest per (frame,
levelsup)).  Frames are lists of rows of one feature table.

The other files: ref_dbow2_score.npz (BowVectors taken from the V1 and V4 fixtures, every ordered
pair, voc.score under L1_NORM), ref_dbow2_distance.npz (FORB::distance of 66 descriptor pairs)
and ref_dbow2_v1_resaved.txt (saveToTextFile's own output for V1, committed as written).

`record_*` is the single place that talks to the binaries: the generator calls it to write the
fixtures and the fixture check calls it again to compare, so both see the same bytes.
"""
from __future__ import annotations

import json
import pathlib
import subprocess
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
REF_DIR = ROOT / "oracle" / "_ref"
BINARIES = ("dbow2_ref_fma", "dbow2_ref_plain")  # the first is the recorded reference
VOCABS = ("v1", "v2", "v3", "v4")
RESAVED = GOLD / "ref_dbow2_v1_resaved.txt"
L2_NORM = 1
UNWRITTEN = 0xFFFFFFFF  # the driver's nid before each single-feature call

OUT_KEYS = ("bow_n", "bow_words", "bow_vals", "fv_n", "fv_nodes", "fv_cnt", "fv_feats", "feat_n", "feat_word",
            "feat_weight", "feat_nid", "plain_differs", "plain_bow_vals")


def binaries_present() -> bool:
    return all((REF_DIR / b).exists() for b in BINARIES)


def levelsups(L: int):
    return [0, 1, L - 1, L, L + 2]


def write_vocabulary_text(path, k, L, scoring, weighting, parent, is_leaf, desc, weight) -> None:
    """The product's writer (exact %.17g weights), without the trailing newline that the
    reference's loader turns into a ghost node."""
    from orbslam_jpminipc_amd.vocabulary import write_text

    write_text(path, k, L, scoring, weighting, parent, is_leaf, desc, weight)
    text = pathlib.Path(path).read_text()
    assert text.endswith("\n") and not text.endswith("\n\n")
    pathlib.Path(path).write_text(text[:-1])


def _run(binary, *args):
    r = subprocess.run([str(REF_DIR / binary), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{binary} {args[0]} failed ({r.returncode}): {r.stdout}")


class _Reader:
    def __init__(self, path):
        self.buf = pathlib.Path(path).read_bytes()
        self.pos = 0

    def take(self, dtype, n):
        dt = np.dtype(dtype)
        out = np.frombuffer(self.buf, dt, n, self.pos).copy()
        self.pos += n * dt.itemsize
        return out

    def u32(self):
        return int(self.take("<u4", 1)[0])

    def done(self):
        return self.pos == len(self.buf)


def run_transform(binary, voc_path, frames, lvls, tmp):
    """{(frame index, levelsup index): record dict} from one `load+transform` run."""
    tmp = pathlib.Path(tmp)
    desc = np.concatenate([np.asarray(f, np.uint8).reshape(-1, 32) for f in frames]) if frames else np.zeros((0, 32))
    (tmp / "desc.bin").write_bytes(np.ascontiguousarray(desc, np.uint8).tobytes())
    _run(binary, "load+transform", voc_path, tmp / "desc.bin", ",".join(str(len(f)) for f in frames),
         ",".join(map(str, lvls)), tmp / "out.bin")
    rd = _Reader(tmp / "out.bin")
    out = {}
    for fi in range(len(frames)):
        for li in range(len(lvls)):
            r = {}
            nb = rd.u32()
            r["bow_words"], r["bow_vals"] = rd.take("<u4", nb), rd.take("<f8", nb)
            nf = rd.u32()
            r["fv_nodes"], r["fv_cnt"] = rd.take("<u4", nf), rd.take("<u4", nf)
            r["fv_feats"] = rd.take("<u4", int(r["fv_cnt"].sum()))
            n = rd.u32()
            assert n == len(frames[fi])
            r["feat_word"], r["feat_weight"], r["feat_nid"] = rd.take("<u4", n), rd.take("<f8", n), rd.take("<u4", n)
            out[fi, li] = r
    assert rd.done()
    return out


def case_order(n_frames, n_ws, n_lvls):
    """Storage order of the cases: frame, then weighting/scoring, then levelsup."""
    return [(f, w, l) for f in range(n_frames) for w in range(n_ws) for l in range(n_lvls)]


def _same(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


BOW_KEYS = ("bow_words", "bow_vals")
LVL_KEYS = ("fv_nodes", "fv_cnt", "fv_feats", "feat_word", "feat_weight", "feat_nid")


def _pack(n_frames, n_ws, n_lvls, ref, plain, scoring_of):
    """Per-case records {(frame, ws, levelsup): ...} of the two binaries -> the arrays a fixture
    stores.  The reference's BowVector does not depend on levelsup, and its FeatureVector and
    single-feature results do not depend on the weighting/scoring pair: both are asserted here,
    for every case, and each is then stored once (BowVectors per (frame, ws), the rest per
    (frame, levelsup)).  Between the two binaries all but L2-normalised values must be
    byte-equal."""
    for c in case_order(n_frames, n_ws, n_lvls):
        f, w, l = c
        for k in BOW_KEYS + LVL_KEYS:
            if k != "bow_vals":
                assert _same(ref[c][k], plain[c][k]), ("the two reference builds differ in", k, c)
        for k in BOW_KEYS:
            assert _same(ref[c][k], ref[f, w, 0][k]), ("BowVector depends on levelsup", c)
            assert _same(plain[c][k], plain[f, w, 0][k]), ("BowVector depends on levelsup", c)
        for k in LVL_KEYS:
            assert _same(ref[c][k], ref[f, 0, l][k]), (k, "depends on weighting/scoring", c)
    cat = {k: [] for k in BOW_KEYS + LVL_KEYS}
    bow_n, fv_n, feat_n, differs, plain_vals = [], [], [], [], []
    for f in range(n_frames):
        for w in range(n_ws):
            r, p = ref[f, w, 0], plain[f, w, 0]
            d = not _same(r["bow_vals"], p["bow_vals"])
            assert not d or scoring_of(w) == L2_NORM, ("the two reference builds differ outside L2", f, w)
            differs.append(d)
            if d:
                plain_vals.append(p["bow_vals"])
            for k in BOW_KEYS:
                cat[k].append(r[k])
            bow_n.append(len(r["bow_words"]))
        for l in range(n_lvls):
            r = ref[f, 0, l]
            for k in LVL_KEYS:
                cat[k].append(r[k])
            fv_n.append(len(r["fv_nodes"]))
            feat_n.append(len(r["feat_word"]))
    out = {}
    for k, v in cat.items():
        out[k] = np.concatenate(v).astype(np.float64 if k in ("bow_vals", "feat_weight") else np.uint32)
    out["bow_n"], out["fv_n"], out["feat_n"] = (np.array(x, np.int32) for x in (bow_n, fv_n, feat_n))
    out["plain_differs"] = np.array(differs, np.uint8)
    out["plain_bow_vals"] = np.concatenate(plain_vals) if plain_vals else np.zeros(0, np.float64)
    return out


def record_vocabulary(k, L, parent, is_leaf, desc, weight, ws, frames, lvls):
    """The output arrays (OUT_KEYS) of one vocabulary fixture, from both binaries."""
    assert binaries_present()
    res = {b: {} for b in BINARIES}
    with tempfile.TemporaryDirectory() as tmp:
        voc = pathlib.Path(tmp) / "voc.txt"
        for wi, (weighting, scoring) in enumerate(ws):
            write_vocabulary_text(voc, k, L, int(scoring), int(weighting), parent, is_leaf, desc, weight)
            for b in BINARIES:
                for (fi, li), r in run_transform(b, voc, frames, lvls, tmp).items():
                    res[b][fi, wi, li] = r
    return _pack(len(frames), len(ws), len(lvls), res[BINARIES[0]], res[BINARIES[1]], lambda w: int(ws[w][1]))


def record_resave(k, L, parent, is_leaf, desc, weight, frames, lvls):
    """(text the reference's saveToTextFile writes for the (TF_IDF, L1_NORM) vocabulary, output
    arrays of the reference's transform after loading that text without its last newline)."""
    assert binaries_present()
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        write_vocabulary_text(tmp / "voc.txt", k, L, 0, 0, parent, is_leaf, desc, weight)
        texts = []
        for b in BINARIES:
            _run(b, "resave", tmp / "voc.txt", tmp / f"{b}.txt")
            texts.append((tmp / f"{b}.txt").read_bytes())
        assert texts[0] == texts[1], "the two reference builds save different text"
        text = texts[0]
        assert text.endswith(b"\n") and not text.endswith(b"\n\n")
        (tmp / "stripped.txt").write_bytes(text[:-1])
        res = []
        for b in BINARIES:
            res.append({(fi, 0, li): r for (fi, li), r in run_transform(b, tmp / "stripped.txt", frames, lvls,
                                                                         tmp).items()})
    return text, _pack(len(frames), 1, len(lvls), res[0], res[1], lambda w: 0)


def record_scores(bows, pairs):
    """f64 voc.score(bows[a], bows[b]) per pair under L1_NORM; the two binaries must agree."""
    assert binaries_present()
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        # a one-word vocabulary: score() only consults the scoring object
        write_vocabulary_text(tmp / "voc.txt", 2, 1, 0, 0, [0, 0], [1, 1], np.zeros((2, 32), np.uint8), [1.0, 1.0])
        blob = [np.array([len(bows)], "<u4").tobytes()]
        for w, v in bows:
            blob += [np.array([len(w)], "<u4").tobytes(), np.asarray(w, "<u4").tobytes(), np.asarray(v, "<f8").tobytes()]
        (tmp / "bows.bin").write_bytes(b"".join(blob))
        (tmp / "pairs.bin").write_bytes(np.array([len(pairs)], "<u4").tobytes()
                                        + np.asarray(pairs, "<u4").reshape(-1, 2).tobytes())
        out = []
        for b in BINARIES:
            _run(b, "score", tmp / "voc.txt", tmp / "bows.bin", tmp / "pairs.bin", tmp / "out.bin")
            out.append(np.frombuffer((tmp / "out.bin").read_bytes(), "<f8").copy())
    assert len(out[0]) == len(pairs) and _same(out[0], out[1]), "the two reference builds score differently"
    return out[0]


def record_distances(pairs):
    """i32 FORB::distance per (a, b) row of `pairs` (N, 2, 32)."""
    assert binaries_present()
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        (tmp / "pairs.bin").write_bytes(np.ascontiguousarray(pairs, np.uint8).tobytes())
        out = []
        for b in BINARIES:
            _run(b, "distance", tmp / "pairs.bin", tmp / "out.bin")
            out.append(np.frombuffer((tmp / "out.bin").read_bytes(), "<i4").copy())
    assert len(out[0]) == len(pairs) and _same(out[0], out[1])
    return out[0]


# ---- reading a fixture ------------------------------------------------------------------------
class Case:
    """One recorded transform: inputs and the reference's outputs."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def fv_offsets(self):
        return np.concatenate([[0], np.cumsum(self.fv_cnt)]).astype(np.int32)

    @property
    def fv_lists(self):
        o = self.fv_offsets
        return [self.fv_feats[o[i]:o[i + 1]].tolist() for i in range(len(self.fv_nodes))]


class Outputs:
    """The packed output arrays: BowVectors per (frame, ws), the rest per (frame, levelsup)."""

    def __init__(self, z, n_ws, n_lvls, prefix=""):
        self.a = {k: z[prefix + k] for k in OUT_KEYS}
        self.n_ws, self.n_lvls = n_ws, n_lvls
        a = self.a
        self.bow_off = np.concatenate([[0], np.cumsum(a["bow_n"])])
        self.fv_off = np.concatenate([[0], np.cumsum(a["fv_n"])])
        self.feat_off = np.concatenate([[0], np.cumsum(a["feat_n"])])
        self.ff_off = np.concatenate([[0], np.cumsum(a["fv_cnt"].astype(np.int64))])[self.fv_off]
        self.plain_off = np.concatenate([[0], np.cumsum(np.where(a["plain_differs"] > 0, a["bow_n"], 0))])

    def case(self, f, w, l, **kw):
        a = self.a
        cb, cl = f * self.n_ws + w, f * self.n_lvls + l
        b0, b1 = self.bow_off[cb], self.bow_off[cb + 1]
        f0, f1 = self.fv_off[cl], self.fv_off[cl + 1]
        g0, g1 = self.ff_off[cl], self.ff_off[cl + 1]
        e0, e1 = self.feat_off[cl], self.feat_off[cl + 1]
        differs = bool(a["plain_differs"][cb])
        return Case(bow_words=a["bow_words"][b0:b1], bow_vals=a["bow_vals"][b0:b1], fv_nodes=a["fv_nodes"][f0:f1],
                    fv_cnt=a["fv_cnt"][f0:f1], fv_feats=a["fv_feats"][g0:g1], feat_word=a["feat_word"][e0:e1],
                    feat_weight=a["feat_weight"][e0:e1], feat_nid=a["feat_nid"][e0:e1], plain_differs=differs,
                    plain_bow_vals=(a["plain_bow_vals"][self.plain_off[cb]:self.plain_off[cb + 1]] if differs
                                    else a["bow_vals"][b0:b1]), fi=f, wi=w, li=l, **kw)


class VocabularyFixture:
    def __init__(self, name):
        self.name = name
        z = np.load(GOLD / f"ref_dbow2_{name}.npz")
        self.z = z
        self.k, self.L = int(z["k"]), int(z["L"])
        self.arrays = (z["parent"], z["is_leaf"], z["desc"], z["weight"])
        self.ws = [tuple(map(int, x)) for x in z["ws"]]  # (weighting, scoring)
        self.lvls = [int(x) for x in z["levelsups"]]
        self.meta = json.loads(str(z["meta"]))
        self.frame_names = self.meta["frames"]
        # frames are rows of one feature table: frame i = feats[frame_rows[off[i]:off[i + 1]]]
        off = np.concatenate([[0], np.cumsum(z["counts"])])
        self.frames = [np.ascontiguousarray(z["feats"][z["frame_rows"][off[i]:off[i + 1]]]).reshape(-1, 32)
                       for i in range(len(z["counts"]))]
        self.out = Outputs(z, len(self.ws), len(self.lvls))
        self.resave = Outputs(z, 1, len(self.lvls), "rs_") if "rs_bow_n" in z.files else None

    def frame(self, name):
        return self.frame_names.index(name)

    def cases(self, wi=None):
        """Every recorded case (of one weighting/scoring pair when `wi` is given)."""
        for f, w, l in case_order(len(self.frames), len(self.ws), len(self.lvls)):
            if wi is None or w == wi:
                yield self.out.case(f, w, l, feats=self.frames[f], levelsup=self.lvls[l], weighting=self.ws[w][0],
                                    scoring=self.ws[w][1],
                                    label=f"{self.name} frame={self.frame_names[f]} ws={self.ws[w]} lu={self.lvls[l]}")

    def resave_cases(self):
        for f, _, l in case_order(len(self.frames), 1, len(self.lvls)):
            yield self.resave.case(f, 0, l, feats=self.frames[f], levelsup=self.lvls[l], weighting=0, scoring=0,
                                   label=f"{self.name} resaved frame={self.frame_names[f]} lu={self.lvls[l]}")


_LOADED = {}


def vocabulary_fixture(name) -> VocabularyFixture:
    if name not in _LOADED:
        _LOADED[name] = VocabularyFixture(name)
    return _LOADED[name]


def score_fixture():
    """(bows [(words, values)], labels, pairs (P, 2), scores (P,) f64, meta)."""
    z = np.load(GOLD / "ref_dbow2_score.npz")
    off = np.concatenate([[0], np.cumsum(z["bow_n"])])
    bows = [(z["bow_words"][off[i]:off[i + 1]], z["bow_vals"][off[i]:off[i + 1]]) for i in range(len(z["bow_n"]))]
    meta = json.loads(str(z["meta"]))
    return bows, meta["labels"], z["pairs"], z["scores"], meta


def distance_fixture():
    """(pairs (N, 2, 32) uint8, FORB::distance (N,) int32)."""
    z = np.load(GOLD / "ref_dbow2_distance.npz")
    return z["pairs"], z["dist"]
