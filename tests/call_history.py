"""TEST INFRASTRUCTURE: the frame ladder of the call-history tests.

A long-lived handle keeps state between calls ("State that outlives a call").  The tests
that drive one handle through a history of calls make stale state from real earlier calls, never
from arbitrary bytes: a dense frame first, then a sparser one of the same geometry, so that whatever
a call fails to reset holds a plausible, in-range leftover of the denser call.  That only works if
the frames really are ordered by density at every pyramid level, which is what this module
guarantees and tests/test_call_history_cases.py checks on the CPU.

Four content classes, eight frames each, from the package's own generators:

  noise   synth_special(SYN_NOISE)    more corners than mnFeaturesPerLevel at every level
  stream  synth_stream                an ordinary scene
  lowtex  synth_special(SYN_LOWTEX)   few corners: at every level a cell that FAST(20) leaves with
                                      <= 3 corners and the FAST(7) re-run with 1 .. 3, and an empty cell
  flat    synth_special(SYN_FLAT)     no corner anywhere

"Corners" are the oracle's per-cell counts (oracle_cell_counts: what a cell holds after the re-run
rule of ORBextractor.cc:609-614, before any retainBest), summed per level.

The workhorse geometry is tests/extractor_edge_frames.py's 323 x 243 (291 detection columns: more
than one k_fast tile; three scalar-tail blur columns) with nfeatures 1000, scale 1.2, 4 levels,
FAST threshold 20; 161 x 121 and 96 x 57 serve the size changes with the same constructor
arguments.  At those two sizes the generators give another order of the classes and noise does not
fill every level's quota, so KEEPS names, per geometry, which conditions hold there.

A class walks its generator's seeds (stream: frame numbers) upwards from its start value and takes
the first eight that meet the class condition, moving on at most MAX_MOVES times per class and
geometry; TAKEN records what was taken, and the CPU guard checks that the walk still ends there.
"""
from __future__ import annotations

import numpy as np

import orbslam_jpminipc_amd as orb
from oracle_lib import Oracle

W, H = 323, 243
SMALL_SIZES = [(161, 121), (96, 57)]
NF, SCALE, NLEVELS, TH = 1000, 1.2, 4, 20
CLASSES = ("noise", "stream", "lowtex", "flat")
PER_CLASS = 8
MAX_MOVES = 20
STREAM = 17                                         # synth_stream's stream number
START = {"noise": 5, "stream": 0, "lowtex": 5, "flat": 5}
_KIND = {"noise": orb.SYN_NOISE, "lowtex": orb.SYN_LOWTEX, "flat": orb.SYN_FLAT}

# what the walk took (seeds; frame numbers for `stream`), per geometry
_FIRST8 = [5, 6, 7, 8, 9, 10, 11, 12]
TAKEN = {
    (323, 243): {"noise": _FIRST8, "stream": [0, 1, 2, 3, 4, 5, 6, 7], "lowtex": _FIRST8, "flat": _FIRST8},
    # (lowtex seed 9 has no empty cell at level 1)
    (161, 121): {"noise": _FIRST8, "stream": [0, 1, 2, 3, 4, 5, 6, 7], "lowtex": [5, 6, 7, 8, 10, 11, 12, 13],
                 "flat": _FIRST8},
    (96, 57): {"noise": _FIRST8, "stream": [0, 1, 2, 3, 4, 5, 6, 7], "lowtex": _FIRST8, "flat": _FIRST8},
}
_ALL = (0, 1, 2, 3)
# The conditions each geometry keeps.  over_quota: levels on which every noise frame has more corners
# than mnFeaturesPerLevel; rerun / empty: levels on which every lowtex frame has a cell with 1 .. 3
# corners / an empty cell; order: (denser, sparser) -> levels on which every frame of the denser class
# has more corners than every frame of the sparser one.  Every frame of noise, stream and lowtex has a
# corner at every level and no flat frame has one, at every geometry.
# At the small sizes the generators' crops change the order: the scene of synth_stream is sparser than
# SYN_LOWTEX's texture there, and noise no longer fills the quota of 1000 features.
KEEPS = {
    (323, 243): {"over_quota": _ALL, "rerun": _ALL, "empty": _ALL,
                 "order": {("noise", "stream"): _ALL, ("stream", "lowtex"): _ALL}},
    (161, 121): {"over_quota": (0, 1, 2), "rerun": _ALL, "empty": _ALL,
                 "order": {("noise", "stream"): _ALL, ("noise", "lowtex"): _ALL}},
    (96, 57): {"over_quota": (), "rerun": _ALL, "empty": _ALL,
               "order": {("noise", "stream"): _ALL, ("lowtex", "stream"): _ALL, ("noise", "lowtex"): (0, 1, 2)}},
}


def generate(cls, seed, w=W, h=H):
    """The class's frame of one seed (stream: frame number), read only."""
    if cls == "stream":
        img = orb.synth_stream(w, h, stream=STREAM, first=seed, count=1)[0]
    else:
        img = orb.synth_special(_KIND[cls], w, h, seed=seed)
    img.setflags(write=False)
    return img


_images, _counts, _oracles, _extracted = {}, {}, {}, {}


def oracle(score=orb.FAST_SCORE):
    """The oracle extractor of the ladder's constructor arguments (scoreType as the product names it)."""
    if score not in _oracles:
        _oracles[score] = Oracle(NF, SCALE, NLEVELS, 1 if score == orb.FAST_SCORE else 0, TH)
    return _oracles[score]


def features_per_level():
    return oracle().level_info()[0]


def cell_counts_of(img):
    """Per level, the oracle's per-cell corner counts (rows x cols) of an image."""
    ora = oracle()
    ora.extract(img)
    return [ora.cell_counts(l).copy() for l in range(NLEVELS)]


def meets(cls, counts, keeps):
    """The class's own condition on per-level cell counts, under a geometry's KEEPS entry."""
    tot = [int(c.sum()) for c in counts]
    if cls == "flat":
        return all(t == 0 for t in tot)
    if not all(t > 0 for t in tot):
        return False
    if cls == "noise":
        fpl = features_per_level()
        return all(tot[l] > fpl[l] for l in keeps["over_quota"])
    if cls == "lowtex":
        return (all(((counts[l] >= 1) & (counts[l] <= 3)).any() for l in keeps["rerun"])
                and all((counts[l] == 0).any() for l in keeps["empty"]))
    return True


def walk(cls, w=W, h=H):
    """The first PER_CLASS seeds from START[cls] upwards that meet the class condition (what TAKEN
    records); raises once more than MAX_MOVES seeds were passed over."""
    taken, seed, moves = [], START[cls], 0
    while len(taken) < PER_CLASS:
        if meets(cls, cell_counts_of(generate(cls, seed, w, h)), KEEPS[(w, h)]):
            taken.append(seed)
        else:
            moves += 1
            if moves > MAX_MOVES:
                raise AssertionError(f"{cls} at {w} x {h}: more than {MAX_MOVES} seeds passed over")
        seed += 1
    return taken


def frame(cls, i, w=W, h=H):
    """Frame i (0 .. 7) of a class at a geometry, built once and shared (read only)."""
    key = (cls, i, w, h)
    if key not in _images:
        _images[key] = generate(cls, TAKEN[(w, h)][cls][i], w, h)
    return _images[key]


def cell_counts(cls, i, w=W, h=H):
    key = (cls, i, w, h)
    if key not in _counts:
        _counts[key] = cell_counts_of(frame(cls, i, w, h))
    return _counts[key]


def expected(cls, i, score=orb.FAST_SCORE, w=W, h=H):
    """The oracle's (keypoints, descriptors) of a ladder frame, computed once per score type."""
    key = (cls, i, w, h, score)
    if key not in _extracted:
        _extracted[key] = oracle(score).extract(frame(cls, i, w, h))
    return _extracted[key]


# ---- partner frames for the matchers -------------------------------------------------------------
# Two frames of one class share nothing (different seeds), so no matcher would accept a pair between
# them.  The partner of a frame is the frame moved by (3, 2) pixels (the far edges wrap round) at 15/16
# of its contrast: most keypoints reappear 3.6 px away with a descriptor a few bits off, inside every
# window the matcher tests use, and the partner is no denser than the frame (fresh noise on every pixel
# would add corners at the re-run's threshold of 7 to a low-texture frame).
PARTNER_SHIFT = (3, 2)


def partner_image(cls, i, w=W, h=H):
    key = (cls, i, w, h, "partner")
    if key not in _images:
        moved = np.roll(frame(cls, i, w, h), (PARTNER_SHIFT[1], PARTNER_SHIFT[0]), axis=(0, 1)).astype(np.int32)
        img = ((moved * 15 + 8) // 16 + 8).astype(np.uint8)
        img.setflags(write=False)
        _images[key] = img
    return _images[key]


def expected_partner(cls, i, score=orb.FAST_SCORE, w=W, h=H):
    key = (cls, i, w, h, score, "partner")
    if key not in _extracted:
        _extracted[key] = oracle(score).extract(partner_image(cls, i, w, h))
    return _extracted[key]


# the frames of tests/test_gpu_matcher_history.py: name -> (keypoints, descriptors) by the oracle
MATCHER_FRAMES = {
    "n0": lambda: expected("noise", 0), "n0p": lambda: expected_partner("noise", 0),
    "n1": lambda: expected("noise", 1), "n1p": lambda: expected_partner("noise", 1),
    "l0": lambda: expected("lowtex", 0), "l0p": lambda: expected_partner("lowtex", 0),
    "l1": lambda: expected("lowtex", 1), "l1p": lambda: expected_partner("lowtex", 1),
    "e0": lambda: expected("flat", 0), "e1": lambda: expected("flat", 1),
}


# ---- the batches the sequences use: lists of (class, index) ----------------------------------
def batch(cls, n=PER_CLASS):
    return [(cls, i) for i in range(n)]


MIXED = [("noise", 0), ("flat", 1), ("lowtex", 2), ("stream", 3), ("flat", 4), ("noise", 5), ("lowtex", 6), ("stream", 7)]


def images(items, w=W, h=H):
    return np.stack([frame(c, i, w, h) for c, i in items])
