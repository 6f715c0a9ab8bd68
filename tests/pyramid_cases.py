"""TEST INFRASTRUCTURE: the geometries of the pyramid-builder sweep and what they must cover.

tests/test_pyramid_cases.py proves the coverage conditions on the CPU (level sizes come from the
oracle's ComputePyramid); tests/test_gpu_pyramid_geometry.py runs every case through every
builder.  The `expect` of a case (stream plan, no plan, refused) and its K0 are what
orb_extractor geometry building answered on an MI355X; the GPU test asserts them, so a geometry
that loses its plan fails instead of skipping.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from oracle_lib import Oracle

PLAN, NO_PLAN, REFUSED = "plan", "no plan", "refused"

# expect: PLAN / NO_PLAN / REFUSED; k0: level-0 rows per round of the plan (None: no plan);
# why: the reason of a NO_PLAN, or the error text of a REFUSED
Case = namedtuple("Case", "name W H nf sf nl expect k0 why", defaults=(PLAN, None, ""))


def _c(W, H, nf, sf, nl, expect=PLAN, k0=None, why=""):
    return Case(f"{W}x{H}_nf{nf}_sf{sf}_L{nl}", W, H, nf, sf, nl, expect, k0, why)


# ---- width sweep: every level width takes all 16 residues mod 16 -------------------------------
WIDTH_SWEEP = [_c(W, 57, 300, 1.2, 4, PLAN, 32) for W in range(64, 128)]
# ---- height sweep: level heights 33 (both mirror stores on one row) .. 50 and more -------------
HEIGHT_SWEEP = [_c(96, H, 300, 1.2, 4, PLAN, 32) for H in range(57, 90)]
# ---- level counts: L <= 14 has a plan (one wave per level at 13 and 14), 15 and 16 have none ----
TOO_MANY_LEVELS = "more levels than builder waves (L > PS_THREADS / 64 - PS_LOADERS = 14)"
LEVEL_COUNTS = [
    _c(80, 60, 300, 1.2, 2, PLAN, 32),
    _c(80, 60, 300, 1.2, 3, PLAN, 32),
    _c(330, 250, 1000, 1.2, 8, PLAN, 32),
    _c(130, 120, 600, 1.1, 13, PLAN, 32),
    _c(120, 116, 600, 1.1, 14, PLAN, 32),
    _c(140, 134, 700, 1.1, 15, NO_PLAN, None, TOO_MANY_LEVELS),
    _c(160, 150, 800, 1.1, 16, NO_PLAN, None, TOO_MANY_LEVELS),
]
# ---- scale factors: exact levels from every builder, or refused when the geometry is built -----
SCALE_FACTORS = [
    _c(100, 80, 300, 1.05, 4, PLAN, 32),
    _c(100, 80, 300, 1.33, 3, PLAN, 32),
    _c(120, 90, 300, 1.5, 3, PLAN, 32),
    _c(160, 120, 300, 1.7, 3, PLAN, 32),
    _c(200, 150, 300, 1.9, 3, PLAN, 32),
    _c(300, 200, 300, 1.99, 3, PLAN, 32),
    _c(300, 200, 300, 2.5, 2, PLAN, 32),
    _c(300, 200, 300, 3.0, 2, PLAN, 32),
]
# ---- wide, short frames: the K0 ladder {32, 24, 16, 12, 8, 6, 4, 2} and per-round decode -------
WIDE_SHORT = [
    _c(600, 100, 400, 1.2, 3, PLAN, 24),
    _c(1000, 150, 600, 1.2, 3, PLAN, 16),
    _c(1300, 200, 800, 1.2, 3, PLAN, 12),
    _c(2040, 300, 1500, 1.2, 3, PLAN, 8),
    _c(2700, 300, 800, 1.2, 3, PLAN, 6),
    _c(4000, 300, 1000, 1.2, 3, PLAN, 2),
    # six levels of a wide frame want more than the 14 builder waves: some levels decode per round
    _c(1000, 150, 400, 1.2, 6, PLAN, 8),
]
# ---- input alignment x partial last unit (load_unit16) -----------------------------------------
ALIGN_WIDTHS = [_c(64 + r, 57, 300, 1.2, 4, PLAN, 32) for r in range(16)]
ALIGN_LAYOUTS = [(0, 0), (1, 3), (4, 12), (16, 16), (15, 1)]  # (byte offset, extra row stride)

GROUPS = {"width": WIDTH_SWEEP, "height": HEIGHT_SWEEP, "levels": LEVEL_COUNTS, "scale": SCALE_FACTORS,
          "wide": WIDE_SHORT}
ALL_CASES = list(dict.fromkeys(c for g in GROUPS.values() for c in g))  # (96 x 57 is in both sweeps)

# the fused tail depends on level sizes only: a subset of the sweeps and the level-count cases
TAIL_CASES = WIDTH_SWEEP[::4] + HEIGHT_SWEEP[::4] + LEVEL_COUNTS
# the automatic path at B = 256: every case without a plan that creates, and three with one
AUTO_PLAN_CASES = [WIDTH_SWEEP[5], HEIGHT_SWEEP[0], LEVEL_COUNTS[2]]


def auto_cases():
    return [c for c in ALL_CASES if c.expect == NO_PLAN] + AUTO_PLAN_CASES


# ---- frames --------------------------------------------------------------------------------------
def block_frame(rng, W, H):
    """Random 0 / 255 blocks of random sizes 1 .. 5 px: both vertical formulas at their extremes."""
    out = np.empty((H, W), np.uint8)
    y = 0
    while y < H:
        bh = int(rng.integers(1, 6))
        x = 0
        while x < W:
            bw = int(rng.integers(1, 6))
            out[y:y + bh, x:x + bw] = 255 * int(rng.integers(0, 2))
            x += bw
        y += bh
    return out


@lru_cache(maxsize=None)
def _frames(W, H, B, seed):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, size=(B, H, W), dtype=np.uint8)
    if B > 1:
        f[1] = block_frame(rng, W, H)
    f.setflags(write=False)
    return f


def frames(case, B, seed=20):
    """(B, H, W) uint8, read-only and shared: frame 0 uniform random bytes, frame 1 the 0 / 255
    blocks, the rest random bytes."""
    return _frames(case.W, case.H, B, seed)


# ---- the oracle's pyramid, computed once per (case, frame content) --------------------------------
_ref_cache = {}


def oracle_levels(case, img):
    """The oracle's padded levels of one frame (ComputePyramid: resize + copyMakeBorder)."""
    key = (case.nf, case.sf, case.nl, img.shape, img.tobytes())
    if key not in _ref_cache:
        ora = Oracle(case.nf, case.sf, case.nl, 1, 20)
        ora.extract(img)
        lv = [ora.level_image(l) for l in range(case.nl)]
        for a in lv:
            a.setflags(write=False)
        _ref_cache[key] = lv
    return _ref_cache[key]


def level_sizes(case):
    """[(w, h)] per level, read from the oracle's pyramid."""
    return [(a.shape[1] - 32, a.shape[0] - 32) for a in oracle_levels(case, frames(case, 2)[0])]


# ---- coverage predicates ---------------------------------------------------------------------------
def tail_columns(dw):
    """Columns of VResizeLinear's scalar tail at level width dw (the host's xs_resize walk)."""
    xs = 0
    while xs <= dw - 16:
        xs += 16
    while xs < dw - 4:
        xs += 4
    return dw - xs


def mirror_rows(h):
    """Rows of a level of height h that carry (a top mirror store, a bottom one, both)."""
    top = {dy for dy in range(h) if 1 <= dy <= 16}
    bot = {dy for dy in range(h) if h - 17 <= dy <= h - 2}
    return top, bot, top & bot


def load_classes(ptr, stride, fpitch, W, H, B):
    """What load_unit16 sees for a batch at device address ptr: the align class (16, 4 or 1) and
    the set of (need, sh + need > 16) over every 16-byte unit that takes the funnel-shift path."""
    al = ptr | stride | fpitch
    align = 16 if al % 16 == 0 else 4 if al % 4 == 0 else 1
    seen = set()
    for b in range(B):
        for r in range(H):
            for u in range((W + 15) // 16):
                nvalid = W - 16 * u
                if nvalid >= 16 and align == 16:
                    continue
                p = ptr + b * fpitch + r * stride + 16 * u
                sh, need = p % 16, min(nvalid, 16)
                seen.add((need, sh + need > 16))
    return align, seen


def embed(case, B, offset, extra, seed=31):
    """The case's frames inside a larger host buffer of random bytes: rows at stride W + extra,
    the first at byte `offset`; returns (buffer, stride).  A byte read past a row's end, or before
    its start, is then a random one and changes the result."""
    f = frames(case, B)
    stride = case.W + extra
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, size=offset + B * case.H * stride + 64, dtype=np.uint8)
    view = buf[offset:offset + B * case.H * stride].reshape(B, case.H, stride)
    view[:, :, :case.W] = f
    return buf, stride
