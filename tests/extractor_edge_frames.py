"""TEST INFRASTRUCTURE: constructed extractor frames whose octave-0 result is known by construction.

The frames of synth_stream / synth_special carry noise on every pixel, which removes exactly the
inputs on which several branches of k_fast, k_rerun, k_select and k_orient_desc decide (DESIGN.md
§5.3).  The builders here put those inputs on a noise-free background:

  threshold_table   strength exactly at fastTh, one above it, the `<= 3` re-run rule at 3 and at 4,
                    dark marks (ORBextractor.cc:609-614); `saturated` for the largest strength byte
  nms_pairs         equal and unequal adjacent marks swept over every column / row, so that every
                    cell boundary (and any tile or wave boundary of the kernel) falls inside a pair
  orientation_ties  IC_Angle's moments zero, on an axis and on a diagonal (fastAtan2's ties)
  blur_ties         7x7 blur sums that are exact halves with an even integer part, in the SSE2
                    columns (half to even) and in the scalar tail columns (half up)
  mass_ties         more equal-strength corners than every quota, so that both retainBest passes cut
                    inside one tie class

All frames are 323 x 243: 323 mod 4 = 3 leaves three scalar-tail blur columns, and the detection
width 291 is more than one 256-column k_fast tile.  A single pixel of contrast c on a flat background
is a FAST corner at threshold t iff |c| > t, with response |c| - 1 (test_oracle_kat.py
test_fast_cell_semantics); FAST runs per cell image, so a neighbour in the next cell scores 0 in NMS.
By-construction expectations are about octave 0 only.

Two restatements serve the guards of tests/test_extractor_edge_frames_oracle.py: the cell grid of
ORBextractor.cc:527-544 (`cell_grid`) and computeOrbDescriptor on a given blurred plane
(`descriptors_level0`, ORBextractor.cc:155-194).
"""
from __future__ import annotations

import pathlib
import re
from dataclasses import dataclass, field

import numpy as np

F32 = np.float32
W, H = 323, 243
BG = 100
EDGE = 16
SCALE, NLEVELS = 1.2, 4
TAPS = np.array([18, 34, 49, 55, 49, 34, 18], np.int64)
K_FAST_TILE = 256  # detection columns per k_fast tile at level 0 (FT_TW_MAX, csrc/orb_extract.h)


@dataclass
class EdgeFrame:
    name: str
    img: np.ndarray
    nf: int
    th: int = 20
    # marks: (x, y) -> label, for the failure messages and the class checks
    labels: dict = field(default_factory=dict)
    # octave-0 keypoints known by construction: {(x, y): response}, or None (parity only)
    expected: dict | None = None

    def describe(self, x, y) -> str:
        """Label of the mark at or next to (x, y) (level-0 coordinates)."""
        x, y = int(round(float(x))), int(round(float(y)))
        for dy in (0, -1, 1):
            for dx in (0, -1, 1):
                if (x + dx, y + dy) in self.labels:
                    return self.labels[(x + dx, y + dy)]
        return "no mark"


# ---- ORBextractor's constructor and cell grid, restated --------------------------------------
def features_per_level(nf, scale=SCALE, nlevels=NLEVELS):
    """mnFeaturesPerLevel (ORBextractor.cc:474-487): float arithmetic, cvRound per level."""
    factor = F32(1.0 / float(F32(scale)))
    n = F32(nf) * (F32(1) - factor) / (F32(1) - F32(float(factor) ** nlevels))
    out = []
    for _ in range(nlevels - 1):
        out.append(int(np.rint(n)))
        n = F32(n * factor)
    out.append(max(nf - sum(out), 0))
    return out


@dataclass
class CellGrid:
    cols: int
    rows: int
    cellW: int
    cellH: int
    w: int
    h: int
    per_cell: int  # nfeaturesCell

    def cell_of(self, x, y):
        """(row, col) of the cell whose FAST detects pixel (x, y), None outside [16, w-16) x [16, h-16)."""
        if not (EDGE <= x < self.w - EDGE and EDGE <= y < self.h - EDGE):
            return None
        return (min((y - EDGE) // self.cellH, self.rows - 1), min((x - EDGE) // self.cellW, self.cols - 1))

    def x_bounds(self):
        """First column of every cell but the first."""
        return [EDGE + j * self.cellW for j in range(1, self.cols)]

    def y_bounds(self):
        return [EDGE + i * self.cellH for i in range(1, self.rows)]


def cell_grid(nf, w=W, h=H, level_w=None, level_h=None):
    """Level-0 grid (ORBextractor.cc:527-544): levelCols = int(sqrt(float(nDesired) / (5 * ratio))),
    levelRows = int(ratio * levelCols) in float32, cell size = ceil(span / count); the last row and
    column take what is left."""
    n0 = features_per_level(nf)[0]
    ratio = F32(w) / F32(h)
    cols = int(np.sqrt(F32(n0) / (F32(5) * ratio), dtype=F32))
    rows = int(ratio * F32(cols))
    lw, lh = (level_w or w) - 2 * EDGE, (level_h or h) - 2 * EDGE
    cw, ch = int(np.ceil(F32(lw) / F32(cols))), int(np.ceil(F32(lh) / F32(rows)))
    assert (cols - 1) * cw < lw and (rows - 1) * ch < lh  # no cell starts past the border here
    return CellGrid(cols, rows, cw, ch, w, h, int(np.ceil(F32(n0) / F32(rows * cols))))


def _flat(v=BG):
    return np.full((H, W), v, np.uint8)


def _far_enough(pts, d=8):
    p = np.array(sorted(pts))
    for i in range(len(p)):
        c = np.abs(p[i + 1:] - p[i]).max(axis=1)
        if len(c) and c.min() < d:
            return False
    return True


# ---- frame 1: threshold and re-run table ------------------------------------------------------
CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
          (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]  # FAST's 16 pixels


@dataclass(frozen=True)
class Arc:
    """A mark whose strength is decided by the arc test, not by the compass pre-test: centre
    BG + s + 4, the eight circle pixels 8 .. 15 at BG + 4 and the other eight at BG.  Every 9-arc
    holds a pixel that is exactly s below the centre, and circle points 0 and 4 are s + 4 below it:
    the largest t at which the mark is a corner is s - 1, its response there s - 1.  The pixels at
    BG + 4 are below every threshold."""
    s: int


def strength(m):
    """The largest threshold a mark is a corner at, plus one (a single pixel: its contrast)."""
    return m.s if isinstance(m, Arc) else abs(m)


def table_cases(th):
    """The marks of the five cells, relative to fastTh = th: single pixels by their contrast, and arc
    marks whose strength sits exactly at th, or at the re-run's 7."""
    return [
        [th + 10, th + 20, th + 30, th + 40, th, th + 1, 8, Arc(th)],   # 5 over th: no re-run
        [th + 10, th + 20, th + 30, 8, 9, 7, th, Arc(7)],               # 3 over: FAST(7) re-run
        [th + 10, th + 20, th + 30, th + 1, 8, 7],                      # 4 over: no re-run
        [th, th - 1, 8, 7, 6, Arc(th)],                                 # 0 over: re-run
        [-(th + 10), -(th + 20), -(th + 30), -8, -7, th + 1],           # dark marks, 4 over
    ]


def cell_rule(marks, th):
    """What the reference keeps of one cell's marks: FAST(th), and FAST(7) instead when that left
    <= 3 (ORBextractor.cc:609-614)."""
    over = [m for m in marks if strength(m) > th]
    return over if len(over) > 3 else [m for m in marks if strength(m) > 7]


def threshold_table(th=20, nf=500):
    """One cell per case, twice: case k in cell (k, k % 4) and in cell (k, (k + 2) % 4), so that both
    k_fast tiles hold cases.  Marks sit on a 4 x 2 lattice of 16 x 16 steps inside the cell, at least
    8 px from its border."""
    g = cell_grid(nf)
    assert (g.cols, g.rows, g.cellW, g.cellH) == (4, 5, 73, 43)
    img = _flat()
    f = EdgeFrame(f"threshold_table(th={th})", img, nf, th, expected={})
    for k, marks in enumerate(table_cases(th)):
        assert len(marks) <= min(8, g.per_cell)
        for col in (k % 4, (k + 2) % 4):
            x0, y0 = EDGE + col * g.cellW + 10, EDGE + k * g.cellH + 10
            kept = cell_rule(marks, th)
            for m, c in enumerate(marks):
                x, y = x0 + 16 * (m % 4), y0 + 16 * (m // 4)
                assert g.cell_of(x - 8, y - 8) == g.cell_of(x + 8, y + 8) == (k, col)
                if isinstance(c, Arc):
                    img[y, x] = BG + c.s + 4
                    for dx, dy in CIRCLE[8:]:
                        img[y + dy, x + dx] = BG + 4
                    f.labels[(x, y)] = f"case {k} cell ({k},{col}) arc mark of strength {c.s}"
                else:
                    img[y, x] = BG + c
                    f.labels[(x, y)] = f"case {k} cell ({k},{col}) contrast {c}"
                if c in kept:
                    f.expected[(x, y)] = strength(c) - 1
    assert _far_enough(f.labels)
    return f


def saturated(nf=500):
    """Left half 0 with marks of 255, right half 255 with marks of 0: response 254, the largest
    strength byte; every third mark has contrast 254.  Marks on a 30 x 22 lattice, at most six per
    cell (under the cell quota), at least 8 px from the step between the halves."""
    g = cell_grid(nf)
    img = np.zeros((H, W), np.uint8)
    half = 161
    img[:, half:] = 255
    f = EdgeFrame("saturated", img, nf, 20, expected={})
    n = 0
    for y in range(20, H - EDGE, 22):
        for x in range(20, W - EDGE, 30):
            if abs(x - half) < 9 or abs(x - (half - 1)) < 9:
                continue
            dark = x >= half
            c = 254 if n % 3 == 2 else 255
            img[y, x] = (255 - c) if dark else c
            f.labels[(x, y)] = f"{'dark' if dark else 'bright'} mark contrast {c}"
            f.expected[(x, y)] = c - 1
            n += 1
    per = {}
    for p in f.labels:
        per[g.cell_of(*p)] = per.get(g.cell_of(*p), 0) + 1
    assert None not in per and max(per.values()) <= g.per_cell and len(f.labels) <= features_per_level(nf)[0]
    assert 254 in f.expected.values() and 253 in f.expected.values()
    return f


# ---- frame 2: NMS pair sweep ------------------------------------------------------------------
PAIR_SECOND = {"h": [(1, 0)], "v": [(0, 1)], "d": [(1, 1), (-1, 1)]}


def nms_pairs(kind, nf=2000):
    """Adjacent marks (200, 200): kind 'h' pairs (x, y), (x+1, y) in rows 9 px apart, 11 px apart in
    the row, row r shifted by r % 11, so that every column 16 .. 305 is the left pixel of a pair;
    'v' the same transposed over every row 16 .. 225; 'd' diagonal and anti-diagonal pairs
    alternating (a sweep over the columns).  Every fourth pair is unequal (200, 201), the stronger
    pixel first or second in turn.
    By construction: a pair survives whole iff its pixels lie in different cells; otherwise an equal
    pair is suppressed whole and of an unequal pair only the stronger pixel survives."""
    g = cell_grid(nf)
    assert (g.cols, g.rows, g.cellW, g.cellH) == (9, 11, 33, 20)
    img = _flat()
    f = EdgeFrame(f"nms_pairs({kind})", img, nf, 20, expected={})
    long_n, short_n = (W, H) if kind != "v" else (H, W)
    first_seen, n, straddling = set(), 0, 0
    for r, s in enumerate(range(19, short_n - EDGE - 2, 9)):         # position across the sweep
        for t in range(EDGE - 11 + r % 11, long_n - EDGE, 11):       # position along the sweep
            p1 = (t, s) if kind != "v" else (s, t)
            dx, dy = PAIR_SECOND[kind][n % len(PAIR_SECOND[kind])]
            if dx < 0:
                p1 = (p1[0] + 1, p1[1])
            p2 = (p1[0] + dx, p1[1] + dy)
            c1, c2 = g.cell_of(*p1), g.cell_of(*p2)
            if c1 is None or c2 is None:
                continue
            unequal = n % 4 == 3
            v1, v2 = (200, 200) if not unequal else ((201, 200) if n % 8 == 3 else (200, 201))
            n += 1
            img[p1[1], p1[0]], img[p2[1], p2[0]] = v1, v2
            straddle = c1 != c2
            straddling += straddle
            what = f"{kind} pair {'straddling cells ' + str(c1) + '/' + str(c2) if straddle else 'inside cell ' + str(c1)}"
            f.labels[p1] = f"{what}, values {v1},{v2}, first pixel"
            f.labels[p2] = f"{what}, values {v1},{v2}, second pixel"
            first_seen.add(min(p1[0], p2[0]) if kind != "v" else p1[1])
            if straddle:
                f.expected[p1], f.expected[p2] = v1 - BG - 1, v2 - BG - 1
            elif v1 > v2:
                f.expected[p1] = v1 - BG - 1
            elif v2 > v1:
                f.expected[p2] = v2 - BG - 1
    lo, hi = EDGE, long_n - EDGE - 2
    assert first_seen >= set(range(lo, hi + 1)), sorted(set(range(lo, hi + 1)) - first_seen)
    # every cell boundary along the sweep is straddled, and no cell holds more survivors than its quota
    assert straddling >= (g.cols - 1 if kind != "v" else g.rows - 1)
    per = {}
    for p in f.expected:
        per[g.cell_of(*p)] = per.get(g.cell_of(*p), 0) + 1
    assert max(per.values()) <= g.per_cell
    f.straddling = straddling
    return f


# ---- frame 3: orientation ties ----------------------------------------------------------------
ORIENT_KINDS = [  # (helper offset or None, class of (m10, m01), nominal angle)
    (None, "m10=m01=0", 0.0),
    ((6, 0), "m01=0,m10>0", 0.0),
    ((-6, 0), "m01=0,m10<0", 180.0),
    ((0, 6), "m10=0,m01>0", 90.0),
    ((0, -6), "m10=0,m01<0", 270.0),
    ((6, 6), "|m10|=|m01|", 45.0),
    ((-6, 6), "|m10|=|m01|", 135.0),
    ((-6, -6), "|m10|=|m01|", 225.0),
    ((6, -6), "|m10|=|m01|", 315.0),
]


def moment_class(m10, m01):
    if m10 == 0 and m01 == 0:
        return "m10=m01=0"
    if m01 == 0:
        return "m01=0,m10>0" if m10 > 0 else "m01=0,m10<0"
    if m10 == 0:
        return "m10=0,m01>0" if m01 > 0 else "m10=0,m01<0"
    return "|m10|=|m01|" if abs(m10) == abs(m01) else "general"


def orientation_ties(nf=2000):
    """Isolated bright pixels (200) on a 40 x 40 lattice (8 x 6 = 48 marks, 40 px from every other
    mark: the 31-px patch of a mark holds nothing but its own helper), each alone or with one helper
    pixel of contrast 4 (below every threshold) at the offset of ORIENT_KINDS, the kinds dealt round
    robin down the columns: five marks of each kind at least, and the last column, which lies in
    k_fast's second tile, holds six kinds."""
    img = _flat()
    f = EdgeFrame("orientation_ties", img, nf, 20, expected={})
    f.kinds = {}
    n = 0
    for x in range(20, W - EDGE, 40):
        for y in range(20, H - EDGE, 40):
            off, cls, ang = ORIENT_KINDS[n % len(ORIENT_KINDS)]
            n += 1
            img[y, x] = 200
            if off is not None:
                img[y + off[1], x + off[0]] = BG + 4
            f.labels[(x, y)] = f"mark with helper at {off}: {cls}, nominal angle {ang}"
            f.kinds[(x, y)] = (off, cls, ang)
            f.expected[(x, y)] = 99
    assert n == 48 and max(x for x, _ in f.labels) >= EDGE + K_FAST_TILE
    for (x, y), (off, _, _) in f.kinds.items():  # nothing but the helper within the patch
        patch = img[y - 15:y + 16, x - 15:x + 16].astype(int) - BG
        assert np.count_nonzero(patch) == (1 if off is None else 2)
    return f


def umax_table():
    """ORBextractor's umax (ORBextractor.cc:493-510): the half widths of the circular patch's rows."""
    hp = 15
    vmax, vmin = int(np.floor(hp * np.sqrt(F32(2)) / 2 + 1)), int(np.ceil(hp * np.sqrt(F32(2)) / 2))
    u = [0] * (hp + 1)
    for v in range(vmax + 1):
        u[v] = int(np.rint(np.sqrt(float(hp * hp - v * v))))
    v0 = 0
    for v in range(hp, vmin - 1, -1):
        while u[v0] == u[v0 + 1]:
            v0 += 1
        u[v] = v0
        v0 += 1
    return u


def ic_moments(padded, x, y, umax):
    """IC_Angle's exact integer moments (m10, m01) at level pixel (x, y) of a padded level image."""
    m10 = m01 = 0
    for v in range(-15, 16):
        d = umax[abs(v)]
        row = padded[EDGE + y + v, EDGE + x - d:EDGE + x + d + 1].astype(np.int64)
        m10 += int((np.arange(-d, d + 1) * row).sum())
        m01 += v * int(row.sum())
    return m10, m01


# ---- frame 4: blur ties -------------------------------------------------------------------------
BLUR_D = [1, 0, 0, 2, 0, 0, 0]
BLUR_SEAM = 308  # from this column on the background's phase is 5, not 2


def blur_ties(nf=2000):
    """Every background row equal, 128 - d[(x + 2) % 7]: with taps 18 34 49 55 49 34 18 (sum 257) the
    columns x % 7 == 1 have row sum 257 * 128 - 18 * 1 - 55 * 2 = 32768, so T = 257 * 32768: an exact
    half with the even integer part 128 (half to even: 128, half up: 129).  That phase puts no tie
    into the tail columns (320 .. 322 are 5, 6, 0 mod 7), so the columns from 308 on use
    128 - d[(x + 5) % 7]: 317 is 127 and 320 is 126, the reflected border (323 -> 321) reads 128, and
    column 320 is a tie in every row.  Marks: single pixels 0 and
    255 in turn on a 13 x 17 lattice for x < 290, and at x = 302 + k % 5 every 9 rows marks with a
    helper of value 104 at (-6, -6) (upper half) or (-6, +6) (lower half), whose rotated patterns
    reach the scalar-tail columns 320 .. 322."""
    img = np.empty((H, W), np.uint8)
    img[:] = np.array([128 - BLUR_D[(x + (2 if x < BLUR_SEAM else 5)) % 7] for x in range(W)], np.uint8)[None, :]
    f = EdgeFrame("blur_ties", img, nf, 20)
    n = 0
    for y in range(20, H - EDGE - 3, 17):
        for x in range(20, 290, 13):
            img[y, x] = 0 if n % 2 == 0 else 255
            f.labels[(x, y)] = f"main-field mark {int(img[y, x])}"
            n += 1
    ys = list(range(24, H - EDGE - 8, 9))
    for k, y in enumerate(ys):
        x = 302 + k % 5
        img[y, x] = 0 if k % 2 == 0 else 255
        sy = -6 if k < len(ys) // 2 else 6
        img[y + sy, x - 6] = 104
        f.labels[(x, y)] = f"right-edge mark {int(img[y, x])} with helper at (-6,{sy})"
        f.labels[(x - 6, y + sy)] = f"helper of the right-edge mark at ({x},{y})"
    return f


def blur_sums(padded):
    """T = sum_ij k_i k_j P of every ROI pixel of a padded level image (int64, h x w)."""
    P = padded.astype(np.int64)
    h, w = P.shape[0] - 2 * EDGE, P.shape[1] - 2 * EDGE
    R = sum(TAPS[i] * P[:, EDGE - 3 + i:EDGE - 3 + i + w] for i in range(7))
    return sum(TAPS[j] * R[EDGE - 3 + j:EDGE - 3 + j + h, :] for j in range(7))


def blur_plane(T, tail_rule="up", simd_rule="even"):
    """GaussianBlur's column pass on the sums T: the SSE2 columns x < 4 * (w // 4) round T / 65536 half
    to even, the scalar tail columns half up; `tail_rule` / `simd_rule` swap a rule."""
    q, r = T >> 16, T & 0xFFFF
    up = (T + 32768) >> 16
    even = q + ((r > 32768) | ((r == 32768) & (q % 2 == 1)))
    xs = (T.shape[1] // 4) * 4
    out = np.empty_like(T)
    out[:, :xs] = (even if simd_rule == "even" else up)[:, :xs]
    out[:, xs:] = (up if tail_rule == "up" else even)[:, xs:]
    return np.minimum(out, 255).astype(np.uint8)


def discriminating_ties(T):
    """Pixels on which the two rounding rules differ: T mod 65536 = 32768 with an even integer part
    (below 255).  Returns (count in the SSE2 columns, count in the tail columns, mask)."""
    m = ((T & 0xFFFF) == 32768) & ((T >> 16) % 2 == 0) & ((T >> 16) < 255)
    xs = (T.shape[1] // 4) * 4
    return int(m[:, :xs].sum()), int(m[:, xs:].sum()), m


# ---- frame 5: mass ties ---------------------------------------------------------------------------
def mass_ties(nf=300):
    """Identical marks (180) at x % 8 == 4, y % 8 == 4: 36 x 26 = 936 corners in the detection area,
    all with response 79, against nDesired[0] = 97: every cell's retainBest and the level's cut
    inside one tie class, so the survivors are libstdc++'s nth_element permutation."""
    img = _flat()
    img[4::8, 4::8] = 180
    f = EdgeFrame("mass_ties", img, nf, 20)
    g = cell_grid(nf)
    assert (g.cols, g.rows) == (3, 3)
    for y in range(4, H, 8):
        for x in range(4, W, 8):
            if g.cell_of(x, y) is not None:
                f.labels[(x, y)] = f"lattice mark in cell {g.cell_of(x, y)}"
    assert len(f.labels) == 936 and features_per_level(nf)[0] == 97
    return f


# ---- computeOrbDescriptor on a given plane (ORBextractor.cc:155-194) -----------------------------
def pattern31():
    text = (pathlib.Path(__file__).resolve().parent.parent / "orbslam_jpminipc_amd" / "csrc" / "pattern31.inc").read_text()
    body = text[text.index("{") + 1: text.index("};")]
    return np.array([int(v) for v in re.findall(r"-?\d+", body)], np.int64).reshape(512, 2)


def _fma32(p, c, t):
    """float32 fma(p, c, t) for integer p and float32 c, t, exactly: the sum is formed in extended
    precision, where it is exact for these magnitudes, and rounded once."""
    LD = np.longdouble
    return (p.astype(LD) * c.astype(LD) + t.astype(LD)).astype(F32)


def descriptors_level0(plane, padded, xy, a, b, pattern):
    """Descriptors of level-0 keypoints `xy` (n x 2, integers) sampled on `plane` (h x w, the blurred
    level) inside the ROI and on the raw padded level outside it.  a, b: cos and sin of the angle
    (float32, n).  Sample positions are cvRound(px*b + py*a) down and cvRound(px*a - py*b) across, the
    products contracted as g++ -O3 contracts them: fma(px, b, py*a) and fma(px, a, -(py*b))."""
    h, w = plane.shape
    px, py = pattern[None, :, 0], pattern[None, :, 1]
    a, b = np.asarray(a, F32)[:, None], np.asarray(b, F32)[:, None]
    pya, pyb = py.astype(F32) * a, py.astype(F32) * b
    dy = np.rint(_fma32(px, b, pya)).astype(np.int64)
    dx = np.rint(_fma32(px, a, -pyb)).astype(np.int64)
    X, Y = np.asarray(xy)[:, 0:1] + dx, np.asarray(xy)[:, 1:2] + dy
    inside = (X >= 0) & (X < w) & (Y >= 0) & (Y < h)
    v = np.where(inside, plane[np.clip(Y, 0, h - 1), np.clip(X, 0, w - 1)], padded[Y + EDGE, X + EDGE]).astype(np.int64)
    bits = (v[:, 0::2] < v[:, 1::2]).astype(np.uint8)  # n x 256
    return np.packbits(bits, axis=1, bitorder="little"), X, Y


ALL_BUILDERS = {
    "threshold_table_20": lambda: threshold_table(20),
    "threshold_table_12": lambda: threshold_table(12),
    "threshold_table_7": lambda: threshold_table(7),
    "saturated": saturated,
    "nms_pairs_h": lambda: nms_pairs("h"),
    "nms_pairs_v": lambda: nms_pairs("v"),
    "nms_pairs_d": lambda: nms_pairs("d"),
    "orientation_ties": orientation_ties,
    "blur_ties": blur_ties,
    "mass_ties": mass_ties,
}
_cache = {}


def frame(name) -> EdgeFrame:
    """The named frame, built once and shared (read only)."""
    if name not in _cache:
        f = ALL_BUILDERS[name]()
        f.img.setflags(write=False)
        _cache[name] = f
    return _cache[name]
