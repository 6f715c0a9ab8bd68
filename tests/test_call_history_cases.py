"""CPU guard of tests/call_history.py: every frame the call-history sequences use is in its density
class, measured with the oracle, and the recorded seeds are what the walk over the generators takes.

Without this the GPU sequences could pass for the wrong reason: a "sparse" frame that is as dense as
the one before it leaves no stale entry for a missing reset to pick up.
"""
import numpy as np
import pytest

import call_history as C

GEOMETRIES = [(C.W, C.H)] + C.SMALL_SIZES


def _totals(cls, w, h):
    """(8, levels): corners per level of the class's eight frames."""
    return np.array([[int(c.sum()) for c in C.cell_counts(cls, i, w, h)] for i in range(C.PER_CLASS)])


@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_recorded_seeds_are_the_walk(w, h):
    for cls in C.CLASSES:
        assert C.walk(cls, w, h) == C.TAKEN[(w, h)][cls], cls
        assert len(set(C.TAKEN[(w, h)][cls])) == C.PER_CLASS


@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_class_conditions(w, h):
    keeps, fpl = C.KEEPS[(w, h)], C.features_per_level()
    tot = {cls: _totals(cls, w, h) for cls in C.CLASSES}
    print({cls: tot[cls].tolist() for cls in C.CLASSES})
    assert (tot["flat"] == 0).all()
    for cls in ("noise", "stream", "lowtex"):
        assert (tot[cls] > 0).all(), cls
    for l in keeps["over_quota"]:
        assert (tot["noise"][:, l] > fpl[l]).all(), f"noise within the quota at level {l}"
    for i in range(C.PER_CLASS):
        cc = C.cell_counts("lowtex", i, w, h)
        for l in keeps["rerun"]:
            assert ((cc[l] >= 1) & (cc[l] <= 3)).any(), f"lowtex {i}: no cell with 1 .. 3 corners at level {l}"
        for l in keeps["empty"]:
            assert (cc[l] == 0).any(), f"lowtex {i}: no empty cell at level {l}"
    # the order holds between any frame of the denser class and any frame of the sparser one, so
    # whichever frames of two classes follow each other in a sequence, the later call is the sparser
    for (dense, sparse), levels in keeps["order"].items():
        for l in levels:
            assert tot[dense][:, l].min() > tot[sparse][:, l].max(), (dense, sparse, l)


def test_workhorse_keeps_every_condition():
    """323 x 243 is the geometry the issue's ladder is stated for: the whole chain, at every level."""
    k = C.KEEPS[(C.W, C.H)]
    every = tuple(range(C.NLEVELS))
    assert k["over_quota"] == k["rerun"] == k["empty"] == every
    assert k["order"] == {("noise", "stream"): every, ("stream", "lowtex"): every}


def test_frames_of_a_batch_differ():
    for w, h in GEOMETRIES:
        for cls in ("noise", "stream", "lowtex"):
            imgs = [C.frame(cls, i, w, h).tobytes() for i in range(C.PER_CLASS)]
            assert len(set(imgs)) == C.PER_CLASS, (cls, w, h)
    # flat frames differ in their grey value only, if at all; the mixed batch holds every class twice
    assert sorted(c for c, _ in C.MIXED) == sorted(2 * list(C.CLASSES))
    assert sorted(i for _, i in C.MIXED) == list(range(C.PER_CLASS))


def test_harris_keeps_the_counts():
    """HARRIS_SCORE changes the responses, not which corners a cell holds: the ladder serves both."""
    import orbslam_jpminipc_amd as orb

    for cls in ("noise", "lowtex"):
        C.oracle(orb.HARRIS_SCORE).extract(C.frame(cls, 0))
        for l in range(C.NLEVELS):
            assert np.array_equal(C.oracle(orb.HARRIS_SCORE).cell_counts(l), C.cell_counts(cls, 0)[l])


def test_matcher_frames_are_a_ladder():
    """The inputs of tests/test_gpu_matcher_history.py: dense > sparse > empty = 0 keypoints, and the dense
    and the sparse pair do match (SearchForInitialization by the oracle), so a call that follows a denser
    one has fewer queries, fewer targets and fewer matches than the arena last held."""
    from oracle_lib import search_for_initialization

    F = {name: get() for name, get in C.MATCHER_FRAMES.items()}
    n = {name: len(k) for name, (k, _) in F.items()}
    print(n)
    assert min(n["n0"], n["n0p"], n["n1"], n["n1p"]) > 2 * max(n["l0"], n["l0p"], n["l1"], n["l1p"])
    assert min(n["l0"], n["l0p"], n["l1"], n["l1p"]) > 100 and n["e0"] == n["e1"] == 0
    got = {}
    for a, b in (("n0", "n0p"), ("n1", "n1p"), ("l0", "l0p"), ("l1", "l1p")):
        (k1, d1), (k2, d2) = F[a], F[b]
        prev = np.ascontiguousarray(np.stack([k1["x"], k1["y"]], 1).astype(np.float32))
        got[a] = search_for_initialization(k1, d1, k2, d2, C.W, C.H, prev, 0.9, True, 100)[0]
    print(got)
    assert min(got["l0"], got["l1"]) >= 10 and min(got["n0"], got["n1"]) > 5 * max(got["l0"], got["l1"])
