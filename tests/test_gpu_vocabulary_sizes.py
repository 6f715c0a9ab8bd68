"""k_voc_bow (csrc/orb_voc.hip) at every size step of its sort and at capacity.

The kernel sorts P = max(256, next power of two >= n) keys in 16 P bytes of LDS; every other
vocabulary test feeds it at most ~1000 features (P <= 1024).  Here: both sides of every step of
P up to the capacity of 8192 features (P = 8192: 128 KB of dynamic LDS, above the 64 KB a kernel
gets without hipFuncAttributeMaxDynamicSharedMemorySize), runs of equal words that span every
thread's chunk, the batch entry point with a full frame, an empty frame and a capacity that is
no power of two, what the kernels leave unwritten, and the refusal one feature past capacity.
Everything is bit-exact against the CPU oracle (oracle/orb_oracle_voc.cpp), as in
tests/test_gpu_vocabulary.py, whose comparisons are reused unchanged."""
import numpy as np
import pytest

import orbslam_jpminipc_amd as orb
from orbslam_jpminipc_amd._native import ORB_ENOTSUP
from orbslam_jpminipc_amd.vocabulary import BINARY, DOT_PRODUCT, IDF, L1_NORM, L2_NORM, TF, TF_IDF
from oracle_lib import Oracle
from test_gpu_vocabulary import _same_features, _same_transform, _vocab
from vocab_util import OracleVocabulary, build_vocabulary, random_vocabulary

CAPACITY = 8192  # VOC_MAX_FEATURES
SIZES = [1024, 1025, 2048, 2049, 4096, 4097, 8191, 8192]  # both sides of every step of P, and the capacity
VOCAB_FRAMES = 3  # frames whose descriptors build the vocabulary; the features come from the frames after them
SENTINEL = 0xA5

_CACHE = {}


def _real():
    """(vocabulary arrays, features): real ORB descriptors of 640x480 synthetic frames.  The
    first VOCAB_FRAMES frames build the k = 10, L = 4 tree, the following ones are concatenated
    until there are more than CAPACITY feature rows."""
    if "real" not in _CACHE:
        ora = Oracle(1000, 1.2, 8, 1, 20)
        frames = orb.synth_stream(640, 480, stream=44, first=0, count=VOCAB_FRAMES + 16)
        train = np.concatenate([ora.extract(f)[1] for f in frames[:VOCAB_FRAMES]])
        feats, rows = [], 0
        for f in frames[VOCAB_FRAMES:]:
            feats.append(ora.extract(f)[1])
            rows += len(feats[-1])
            if rows > CAPACITY:
                break
        arrays = build_vocabulary(train, k=10, L=4, seed=21, stop_frac=0.1)
        feats = np.ascontiguousarray(np.concatenate(feats))
        # the last feature of every tested size counts (a stop word there would let a transform that
        # loses its last key pass): where it is a stop word, swap it with a row past the capacity
        ov = OracleVocabulary.create(10, 4, L1_NORM, TF_IDF, *arrays)
        spare = (j for j in range(CAPACITY, len(feats)) if ov.transform_one(feats[j], 0)[1] > 0.0)
        for n in SIZES:
            if not ov.transform_one(feats[n - 1], 0)[1] > 0.0:
                j = next(spare)
                feats[[n - 1, j]] = feats[[j, n - 1]]
        _CACHE["real"] = (arrays, feats)
    return _CACHE["real"]


def _identical(n):
    """n copies of one real feature that lands in a word of positive weight."""
    arrays, feats = _real()
    ov = OracleVocabulary.create(10, 4, L1_NORM, TF, *arrays)
    row = next(f for f in feats if ov.transform_one(f, 0)[1] > 0.0)
    return np.ascontiguousarray(np.repeat(row[None, :], n, axis=0))


def _two_word_case(n):
    return random_vocabulary(2, 1, seed=5), np.random.default_rng(n).integers(0, 256, size=(n, 32), dtype=np.uint8)


def _zero_weight_arrays():
    parent, leaf, desc, weight = _real()[0]
    return parent, leaf, desc, np.zeros_like(weight)


# ---- CPU: the inputs are what the GPU tests below take them to be ----------------------------
def test_inputs_real_descriptors():
    arrays, feats = _real()
    assert len(feats) > CAPACITY and feats.dtype == np.uint8 and feats.shape[1] == 32
    ov = OracleVocabulary.create(10, 4, L1_NORM, TF_IDF, *arrays)
    bw, bv, fn, fo, ff = ov.transform(feats[:CAPACITY], 4)
    # many words with several features each, and stop words (weight 0) among the features
    assert 100 < len(bw) < fo[-1] < CAPACITY and len(fn) == 1 and ff.tolist() == sorted(ff.tolist())
    assert all(ov.transform_one(feats[n - 1], 4)[1] > 0.0 for n in SIZES)  # every size's last feature counts
    for n in SIZES:  # ... so the transform of n features differs from that of n - 1
        assert ov.transform(feats[:n], 4)[4].tolist() != ov.transform(feats[:n - 1], 4)[4].tolist()
    bw0, _, fn0, fo0, _ = ov.transform(feats[:CAPACITY], 0)
    assert bw0.tolist() == bw.tolist() and len(fn0) > 100 and fo0[-1] == fo[-1]


@pytest.mark.parametrize("n", [CAPACITY, 4097])
def test_inputs_degenerate(n):
    arrays, _ = _real()
    # one word, one node: under TF without normalisation the value is n equal weights summed in order
    d = _identical(n)
    ov = OracleVocabulary.create(10, 4, DOT_PRODUCT, TF, *arrays)
    w = ov.transform_one(d[0], 0)[1]
    bw, bv, fn, fo, ff = ov.transform(d, 0)
    s = 0.0
    for _ in range(n):
        s += w
    assert len(bw) == 1 and bv.tolist() == [s] and len(fn) == 1 and fo.tolist() == [0, n]
    assert ff.tolist() == list(range(n))
    # two words: two runs of about n / 2; with levelsup >= L one node (the root) holds every feature
    arrays2, feats2 = _two_word_case(n)
    ov2 = OracleVocabulary.create(2, 1, DOT_PRODUCT, TF, *arrays2)
    bw, bv, fn, fo, ff = ov2.transform(feats2, 1)
    assert bw.tolist() == [0, 1] and fn.tolist() == [0] and fo.tolist() == [0, n] and ff.tolist() == list(range(n))
    fn, fo = ov2.transform(feats2, 0)[2:4]
    assert fn.tolist() == [1, 2] and n // 4 < fo[1] < 3 * n // 4 and fo[2] == n
    # every word a stop word: nothing comes back
    ov0 = OracleVocabulary.create(10, 4, L1_NORM, TF_IDF, *_zero_weight_arrays())
    bw, bv, fn, fo, ff = ov0.transform(_real()[1][:n], 4)
    assert len(bw) == 0 and len(fn) == 0 and fo.tolist() == [0] and len(ff) == 0


# ---- GPU: the host transform ------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("weighting,scoring", [(TF_IDF, L1_NORM), (TF, L2_NORM), (IDF, DOT_PRODUCT),
                                               (BINARY, L1_NORM)])
def test_transform_at_every_sort_size(weighting, scoring):
    arrays, feats = _real()
    gv, ov = _vocab(10, 4, scoring, weighting, arrays)
    for levelsup in (0, 4):
        for n in SIZES:
            _same_transform(gv, ov, feats[:n], levelsup)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [CAPACITY, 4097])
def test_transform_one_run_through_every_chunk(n):
    """All features identical: one word and one node, a single run of equal keys through all 256
    thread chunks of run_heads; under TF the thread that owns the head sums n weights in order."""
    arrays, _ = _real()
    d = _identical(n)
    for weighting, scoring in ((TF, DOT_PRODUCT), (TF_IDF, L2_NORM), (BINARY, L1_NORM)):
        gv, ov = _vocab(10, 4, scoring, weighting, arrays)
        for levelsup in (0, 4):
            _same_transform(gv, ov, d, levelsup)
        bow, fv = gv.transform(d, 0)
        assert len(bow) == 1 and fv.offsets.tolist() == [0, n] and fv.features.tolist() == list(range(n))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [CAPACITY, 4097])
def test_transform_two_words(n):
    """A two-word tree: two runs of about n / 2 keys, and (levelsup = 1) one FeatureVector node,
    the root, that holds every feature."""
    arrays, feats = _two_word_case(n)
    for weighting, scoring in ((TF, DOT_PRODUCT), (TF_IDF, L1_NORM)):
        gv, ov = _vocab(2, 1, scoring, weighting, arrays)
        for levelsup in (0, 1):
            _same_transform(gv, ov, feats, levelsup)
        bow, fv = gv.transform(feats, 1)
        assert list(bow) == [0, 1] and fv.nodes.tolist() == [0] and fv.offsets.tolist() == [0, n]
    _same_features(gv, ov, feats[:300], 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [CAPACITY, 4097])
def test_transform_every_word_a_stop_word(n):
    gv, ov = _vocab(10, 4, L1_NORM, TF_IDF, _zero_weight_arrays())
    feats = _real()[1][:n]
    _same_transform(gv, ov, feats, 4)
    bow, fv = gv.transform(feats, 4)
    assert bow == {} and len(fv.nodes) == 0 and fv.offsets.tolist() == [0] and len(fv.features) == 0


# ---- GPU: the batch entry point ----------------------------------------------------------------
def _sentinel_outputs(B, cap):
    """transform_batch_device's output tensors with every byte set to SENTINEL."""
    import torch

    def full(shape, dtype):
        size = torch.empty((), dtype=dtype).element_size()
        return torch.full(shape[:-1] + (shape[-1] * size,), SENTINEL, dtype=torch.uint8, device="cuda").view(dtype)

    i32, f64 = torch.int32, torch.float64
    return {"feat_word": full((B, cap), i32), "feat_weight": full((B, cap), f64), "feat_node": full((B, cap), i32),
            "bow_words": full((B, cap), i32), "bow_values": full((B, cap), f64), "bow_n": full((B,), i32),
            "fv_nodes": full((B, cap), i32), "fv_offsets": full((B, cap + 1), i32),
            "fv_features": full((B, cap), i32), "fv_n": full((B,), i32)}


def _untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize("cap,counts", [(8192, [8192, 0, 4097]), (2049, [2049, 1, 2048, 0])])
def test_batch_device_full_frames_and_unwritten_rows(cap, counts):
    """Frames at capacity, empty frames and a capacity that is no power of two, every frame against
    the oracle.  Both kernels write only what they produce: feat_* rows past counts[b], bow_* rows
    past bow_n[b], fv_nodes past fv_n[b], fv_offsets past entry fv_n[b] and fv_features past
    fv_offsets[b, fv_n[b]] keep the bytes the caller put there (k_voc_descend skips rows past the
    count; k_voc_bow stores only heads of runs and valid keys: no exception to this was found)."""
    import torch

    arrays, feats = _real()
    gv, ov = _vocab(10, 4, L1_NORM, TF_IDF, arrays)
    B = len(counts)
    D = np.full((B, cap, 32), 0xCD, np.uint8)  # rows past the count hold no descriptor of the frame
    start = 0
    for b, n in enumerate(counts):  # different descriptors per frame
        start = start if start + n <= len(feats) else 0
        D[b, :n] = feats[start:start + n]
        start += n
    out = _sentinel_outputs(B, cap)
    ret = gv.transform_batch_device(torch.from_numpy(D).cuda(), torch.tensor(counts, dtype=torch.int32, device="cuda"),
                                    4, out=out)
    torch.cuda.synchronize()
    assert ret is out
    o = {k: v.cpu().numpy() for k, v in out.items()}
    for b, n in enumerate(counts):
        bw, bv, fn, fo, ff = ov.transform(D[b, :n], 4)
        nb, nf = int(o["bow_n"][b]), int(o["fv_n"][b])
        assert (nb, nf) == (len(bw), len(fn)), b
        assert o["bow_words"][b, :nb].view(np.uint32).tolist() == bw.tolist()
        assert o["bow_values"][b, :nb].view(np.uint64).tolist() == bv.view(np.uint64).tolist()
        assert o["fv_nodes"][b, :nf].view(np.uint32).tolist() == fn.tolist()
        assert o["fv_offsets"][b, :nf + 1].tolist() == fo.tolist()
        assert o["fv_features"][b, :fo[-1]].tolist() == ff.tolist()
        per = [ov.transform_one(f, 4) for f in D[b, :n]]
        assert o["feat_word"][b, :n].view(np.uint32).tolist() == [p[0] for p in per]
        assert o["feat_weight"][b, :n].tolist() == [p[1] for p in per]
        assert o["feat_node"][b, :n].view(np.uint32).tolist() == [p[2] for p in per]
        for name, first in (("feat_word", n), ("feat_weight", n), ("feat_node", n), ("bow_words", nb),
                            ("bow_values", nb), ("fv_nodes", nf), ("fv_offsets", nf + 1), ("fv_features", fo[-1])):
            assert _untouched(o[name][b, first:]), (name, b)


# ---- GPU: one feature past capacity -------------------------------------------------------------
@pytest.mark.gpu
def test_refusal_past_capacity():
    import torch

    arrays, feats = _real()
    gv, ov = _vocab(10, 4, L1_NORM, TF_IDF, arrays)
    assert len(feats) > CAPACITY
    with pytest.raises(orb.OrbError) as e:
        gv.transform(feats[:CAPACITY + 1], 4)
    assert e.value.code == ORB_ENOTSUP
    _same_transform(gv, ov, feats[:1500], 4)
    cap = CAPACITY + 1
    D = torch.zeros((1, cap, 32), dtype=torch.uint8, device="cuda")
    out = _sentinel_outputs(1, cap)
    with pytest.raises(orb.OrbError) as e:
        gv.transform_batch_device(D, torch.tensor([5], dtype=torch.int32, device="cuda"), 4, out=out)
    assert e.value.code == ORB_ENOTSUP
    torch.cuda.synchronize()
    assert all(_untouched(v.cpu().numpy()) for v in out.values())
    _same_transform(gv, ov, feats[:CAPACITY], 4)
    _same_transform(gv, ov, feats[100:900], 0)
