"""TEST INFRASTRUCTURE: SearchForInitialization's window, grid and rotation gates at their exact
thresholds (k_match_init, csrc/orb_sfi.hip; Frame.cc:200-277, ORBmatcher.cc:598-713, 1748-1789).

The companion of gate_tables.py for the one matcher it leaves out.  A table is one
SearchForInitialization call (one rectangle, one window, checkOri on or off); a row is one F1
query with its vbPrevMatched entry and the F2 candidates it needs, and states the vnMatches12
entry the reference line dictates.  Every builder evaluates the gated quantity in numpy float32
as the reference line is written and asserts the intended relation, so a row that misses its
target fails the builder, not the product.

Rows are isolated in descriptor space: a row's candidates lie 0 .. 34 bits from its query, every
other descriptor of the call (other rows, fillers) at least FOREIGN_MIN = 60 bits from it
(asserted by `build`): beyond TH_LOW, and no ratio test of a row changes when such a keypoint
falls into its window (34 < 0.9 * 60).  A row's outcome therefore cannot depend on its
neighbours, whatever their windows cover.

Two rectangles: RECT_A = (64, 576, 64, 448), mfGridElementWidthInv = HeightInv = 0.125 exactly,
cells of 8 px, minX != 0; RECT_B = (-37, 683, -29, 511), the kind ComputeImageBounds returns for
a distorted camera (64 / 720 and 48 / 540 are no floats).  In RECT_B the builder's float32
evaluation alone decides on which side of a gate a row lies; the side names say what it found.

Gates (`Row.inp["key"]` = (gate, side, direction)):
  box            |x2 - qx| against r (Frame.cc:255), closed: a lone candidate at r exactly is kept,
                 the adjacent float outside is not; window 100, 40 and 0
  box second     the same candidate as the SECOND best, 11 bits away against a best of 10: kept, it
                 fails the ratio test (10 < 0.9 * 11 is false); one float outside, the query matches
  posingrid      Frame::PosInGrid's round (Frame.cc:269-273): cell coordinate -0.5 -> -1 and
                 63.5 / 47.5 -> 64 / 48 leave the grid, the adjacent floats stay in cells 0 and
                 63 / 47.  Interior half cells (k + 0.5) are parity only: a keypoint the box admits
                 lies in a cell of the window's range whichever way k + 0.5 rounds (the range ends
                 are floor / ceil of the box edges), so for finite inputs the interior rounding
                 shows in the traversal order alone, which decides nothing between a query's
                 candidates of different distances
  cells          the cell range (Frame.cc:205-223): the only candidate in the window's first /
                 last grid column / row, windows clamped at column 0 / 63 and row 0 / 47, windows
                 left / right / above / below the grid, the whole grid (window 10000), one cell
                 (window 0 on a cell centre), and windows with empty grid columns on either side
                 (window 8; k_match_init's column table then has runs of equal entries)
  level          an octave-1 F2 keypoint on the query is no candidate, an octave-1 F1 keypoint no
                 query (negative octaves: DESIGN.md, known limits)
  steal          a keypoint held at distance d is dead for a later query at the same d
  nonfinite      NaN / +-inf / +-1e12 in vbPrevMatched and NaN / +-inf F2 keypoints: no candidate,
                 never matched (the x86 conversion, DESIGN.md FP policy); candidates wait where a
                 NaN -> 0 or saturating conversion would look
  rescan         box and cells rows whose query has eleven in-window candidates, the eight nearest
                 each held by an earlier query at distance 0, so the truncated top-8 has no live
                 entry and k_match_init's exact rescan decides
  rotbin         rot = 15, 45 .. 345 and the adjacent floats, -0.0f, a1 < a2 by a denormal, -15
                 (ORBmatcher.cc:664-675)
  maxima         ComputeThreeMaxima at equality (max2 / max3 = 0.1f * max1 is kept in float), one
                 short of it, four equal bins, equal second and third, a bin that reaches the top
                 three only through robbed queries' entries
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from orbslam_jpminipc_amd import KEYPOINT_DTYPE

from adversarial_scenes import at_distance, hamming_matrix
from gate_tables import F32, INF, NAN, Row, down, side_of, up
from test_matcher_oracle import c_round, cvt_x86, rot_bin, three_maxima

RECT_A = (64, 576, 64, 448)
RECT_B = (-37, 683, -29, 511)
RECTS = {"A": RECT_A, "B": RECT_B}
QDIST = 10            # a row's gate candidate
FOREIGN_MIN = 60      # every descriptor outside a row's group
FAR = F32(-1e6)       # vbPrevMatched of a filler query: no window reaches the grid from there
FILL_COLS = (40.0, 44.4)  # F2 fillers live in grid columns 40 .. 44
DIRS = ("+x", "-x", "+y", "-y")


class Geom:
    """The grid arithmetic of one rectangle, in float32 as Frame.cc writes it."""

    def __init__(self, bounds):
        self.bounds = tuple(bounds)
        self.mn = (bounds[0], bounds[2])
        self.n = (64, 48)
        self.inv = (F32(64) / F32(bounds[1] - bounds[0]), F32(48) / F32(bounds[3] - bounds[2]))

    def cellf(self, v, ax):
        with np.errstate(all="ignore"):
            return F32(F32(F32(v) - F32(self.mn[ax])) * self.inv[ax])

    def pos(self, v, ax):
        """PosInGrid's coordinate: (int) round((kp - min) * inv)."""
        return cvt_x86(c_round(self.cellf(v, ax)))

    def in_grid(self, x, y):
        return 0 <= self.pos(x, 0) < 64 and 0 <= self.pos(y, 1) < 48

    def edge(self, q, r, ax, sign):
        """(q - min -/+ r) * inv, the value GetFeaturesInArea floors / ceils."""
        with np.errstate(all="ignore"):
            d = F32(F32(q) - F32(self.mn[ax]))
            return F32((F32(d - F32(r)) if sign < 0 else F32(d + F32(r))) * self.inv[ax])

    def raw_range(self, q, r, ax):
        with np.errstate(all="ignore"):
            return cvt_x86(np.floor(self.edge(q, r, ax, -1))), cvt_x86(np.ceil(self.edge(q, r, ax, +1)))

    def cells(self, q, r, ax):
        """(min cell, max cell) after the clamps, or None where GetFeaturesInArea returns early."""
        lo, hi = self.raw_range(q, r, ax)
        lo = max(0, lo)
        if lo >= self.n[ax]:
            return None
        hi = min(self.n[ax] - 1, hi)
        return None if hi < 0 else (lo, hi)

    def coord(self, c, ax):
        """A coordinate near cell coordinate c (callers check what they need of it)."""
        return F32(self.mn[ax] + np.float64(c) / np.float64(self.inv[ax]))

    def candidate(self, qx, qy, x, y, r):
        """GetFeaturesInArea(qx, qy, r) returns an octave-0 keypoint at (x, y)."""
        cx, cy = self.cells(qx, r, 0), self.cells(qy, r, 1)
        if cx is None or cy is None:
            return False
        px, py = self.pos(x, 0), self.pos(y, 1)
        with np.errstate(all="ignore"):
            box = not (abs(F32(F32(x) - F32(qx))) > F32(r) or abs(F32(F32(y) - F32(qy))) > F32(r))
        return bool(cx[0] <= px <= cx[1] and cy[0] <= py <= cy[1] and box)


@dataclass
class Q:
    """One F1 keypoint.  cands: (x, y, dist, octave, angle) F2 keypoints whose descriptors lie `dist`
    bits from this query's.  near: (query, candidate, dist): this query's descriptor lies `dist`
    bits from that candidate's instead of being random (a holder or a robber).  accepts: the
    (query, candidate) it accepts at its turn; robbed: a later query takes that candidate."""
    row: Row
    prev: tuple
    octave: int = 0
    angle: float = 0.0
    cands: list = field(default_factory=list)
    near: tuple = None
    accepts: tuple = None
    robbed: bool = False
    group: int = -1


class SfiTable:
    def __init__(self, name, rect, window, ori=False):
        self.name, self.rect, self.bounds, self.window, self.ori = name, rect, RECTS[rect], int(window), bool(ori)
        self.G = Geom(self.bounds)
        self.q = []
        self.sparse = []  # (row, axis-0 cell range) whose neighbouring grid columns must stay empty
        self.rescans = []  # indices of the queries the exact rescan must decide
        self.maxima = None  # the ComputeThreeMaxima claim of an orientation table: (counts by bin, kept bins)

    def __repr__(self):
        return f"{self.name}/{self.rect}/w{self.window}"

    @property
    def rows(self):
        return [e.row for e in self.q]

    def add(self, gate, side, dirn, prev, cands=(), accept=None, **kw):
        """A query at `prev` with candidates; accept: index into `cands` of the dictated match."""
        i = len(self.q)
        row = Row(f"{self.name}/{self.rect}/w{self.window} {gate} {dirn}", side, None,
                  dict(key=(gate, side, dirn), table=self.name))
        e = Q(row, (F32(prev[0]), F32(prev[1])), cands=[self._cand(*c) for c in cands],
              accepts=None if accept is None else (i, accept), group=i, **kw)
        self.q.append(e)
        return i

    @staticmethod
    def _cand(x, y, dist=QDIST, octave=0, angle=0.0):
        return (F32(x), F32(y), int(dist), int(octave), F32(angle))

    def add_near(self, gate, side, dirn, of, dist, robs=False, angle=0.0, accept=True):
        """A query whose descriptor lies `dist` bits from candidate `of` = (query, candidate), with its
        vbPrevMatched on that candidate: it accepts it (and robs the earlier holder when robs), or,
        accept False, is dictated to find it taken."""
        qi, ci = of
        c = self.q[qi].cands[ci]
        i = self.add(gate, side, dirn, (c[0], c[1]), angle=angle)
        e = self.q[i]
        e.near, e.accepts, e.group = (qi, ci, dist), ((qi, ci) if accept else None), self.q[qi].group
        if robs:
            assert self.q[qi].accepts == (qi, ci) and dist < c[2]
            self.q[qi].robbed = True
        return i

    # ---- expectation ---------------------------------------------------------------------------
    def expectation(self):
        """Per query the (query, candidate) of its final match or None, by the reference's rules
        applied to what each row states: accepted unless robbed, then the orientation filter."""
        keep = None
        if self.ori:
            hist = [[] for _ in range(30)]
            for i, e in enumerate(self.q):
                if e.accepts is not None:  # robbed entries stay in rotHist (ORBmatcher.cc:664-676)
                    c = self.q[e.accepts[0]].cands[e.accepts[1]]
                    hist[rot_bin(e.angle, c[4])].append(i)
            keep = three_maxima(hist)
            self.hist = [len(h) for h in hist]
            self.keep = tuple(keep)
            self.bin_of = {i: b for b, h in enumerate(hist) for i in h}
        out = []
        for i, e in enumerate(self.q):
            ok = e.accepts is not None and not e.robbed and (keep is None or self.bin_of[i] in keep)
            out.append(e.accepts if ok else None)
        return out

    # ---- arrays ----------------------------------------------------------------------------------
    def build(self, lead1=0, lead2=0, seed=1):
        """Arrays of the call: `lead1` filler queries in front of F1 (octave 0, vbPrevMatched far
        outside), `lead2` filler keypoints in front of F2 (octave 0, in grid columns 40 .. 44).
        Returns dict(k1, d1, prev, k2, d2, m12, n, lead1, lead2)."""
        for s in range(seed, seed + 50):
            b = self._build(lead1, lead2, s)
            if b is not None:
                return b
        raise AssertionError(f"{self}: no seed isolates the rows")

    def _build(self, lead1, lead2, seed):
        rng = np.random.default_rng([seed, lead1, lead2])
        nq = len(self.q)
        qd = rng.integers(0, 256, (lead1 + nq, 32), dtype=np.uint8)
        off, cd, owner = {}, [], []
        for i, e in enumerate(self.q):
            if e.near is None:
                for ci, c in enumerate(e.cands):
                    off[i, ci] = len(cd)
                    cd.append(at_distance(rng, qd[lead1 + i], c[2]))
                    owner.append(e.group)
        for i, e in enumerate(self.q):
            if e.near is not None:
                assert not e.cands
                qd[lead1 + i] = at_distance(rng, cd[off[e.near[0], e.near[1]]], e.near[2])
        nc = len(cd)
        fd = rng.integers(0, 256, (lead2, 32), dtype=np.uint8)
        d2 = np.vstack([fd, np.array(cd, np.uint8).reshape(nc, 32)])
        D = hamming_matrix(qd, d2)
        grp = np.concatenate([np.full(lead1, -2), [e.group for e in self.q]])
        own = np.concatenate([np.full(lead2, -3), owner])
        D[grp[:, None] == own[None, :]] = 255
        if D.size and D.min() < FOREIGN_MIN:
            return None
        k1 = np.zeros(lead1 + nq, KEYPOINT_DTYPE)
        k1["x"][:lead1] = k1["y"][:lead1] = FAR
        k1["x"][lead1:] = [e.prev[0] for e in self.q]
        k1["y"][lead1:] = [e.prev[1] for e in self.q]
        k1["octave"][lead1:] = [e.octave for e in self.q]
        k1["angle"][lead1:] = [e.angle for e in self.q]
        k2 = np.zeros(lead2 + nc, KEYPOINT_DTYPE)
        k2["x"][:lead2], k2["y"][:lead2] = self.filler_xy(lead2)
        flat = [c for e in self.q if e.near is None for c in e.cands]
        for name, col in (("x", 0), ("y", 1), ("octave", 3), ("angle", 4)):
            k2[name][lead2:] = [c[col] for c in flat]
        for k in (k1, k2):
            k["size"], k["response"], k["class_id"] = 31, 50, -1
        prev = np.ascontiguousarray(np.stack([k1["x"], k1["y"]], 1).astype(np.float32))
        exp = self.expectation()
        m12 = np.full(lead1 + nq, -1, np.int32)
        for i, a in enumerate(exp):
            self.q[i].row.expect = -1 if a is None else off[a]
            if a is not None:
                m12[lead1 + i] = lead2 + off[a]
        return dict(k1=k1, d1=qd, prev=prev, k2=k2, d2=d2, m12=m12, n=int((m12 >= 0).sum()), lead1=lead1, lead2=lead2,
                    off=off)

    def filler_xy(self, n):
        """Filler i's position does not depend on n: columns 40 .. 44, every grid row."""
        i = np.arange(n)
        cx = FILL_COLS[0] + (i % 23) * ((FILL_COLS[1] - FILL_COLS[0]) / 22.0)
        cy = 0.2 + ((i // 23) % 47) + 0.6 * ((i // (23 * 47)) % 2)
        x = np.array([self.G.coord(c, 0) for c in cx], F32)
        y = np.array([self.G.coord(c, 1) for c in cy], F32)
        assert all(40 <= self.G.pos(a, 0) <= 44 for a in x) and all(0 <= self.G.pos(a, 1) < 48 for a in y)
        return x, y


# ---- searches over a fine lattice ---------------------------------------------------------------
def scan(start, stop, step, pred):
    n = int(abs((stop - start) / step)) + 1
    for k in range(n):
        v = F32(start + k * step * (1 if stop >= start else -1))
        if pred(v):
            return v
    raise AssertionError(("no value", start, stop))


def grid_edge(G: Geom, ax, upper):
    """(outside float, inside float), adjacent, around PosInGrid's first / last cell boundary."""
    want_out = G.n[ax] if upper else -1
    v = G.coord(G.n[ax] - 0.5 if upper else -0.5, ax)
    for _ in range(64):  # walk to the boundary float by float
        p = G.pos(v, ax)
        outside = p >= G.n[ax] if upper else p < 0
        nxt = (down(v) if outside else up(v)) if upper else (up(v) if outside else down(v))
        if outside and not (G.pos(nxt, ax) >= G.n[ax] if upper else G.pos(nxt, ax) < 0):
            assert G.pos(v, ax) == want_out and G.pos(nxt, ax) == (G.n[ax] - 1 if upper else 0)
            return v, nxt
        v = nxt
    raise AssertionError("no grid edge")


def spot(k):
    """Spot k of a 32 px lattice (15 x 11) inside both rectangles' interiors."""
    assert 0 <= k < 165
    return F32(96.0 + 32.0 * (k % 15)), F32(96.0 + 32.0 * (k // 15))


def along(dirn, q, d):
    """The point at signed offset d from q along the row's direction."""
    ax, sg = (0 if dirn[1] == "x" else 1), (1 if dirn[0] == "+" else -1)
    p = [F32(q[0]), F32(q[1])]
    p[ax] = F32(p[ax] + sg * F32(d))
    return tuple(p)


def step_out(dirn, p, k):
    """p moved k floats away from the query along the direction (k < 0: towards it)."""
    ax, sg = (0 if dirn[1] == "x" else 1), (1 if dirn[0] == "+" else -1)
    p = list(p)
    p[ax] = up(p[ax], abs(k)) if sg * k > 0 else down(p[ax], abs(k)) if k else p[ax]
    return tuple(p)


# ---- the rescan dressing ---------------------------------------------------------------------------
def add_rescan(T: SfiTable, gate, side, dirn, q, gate_cand, inside):
    """The row's query preceded by eight holders: its eight nearest candidates (1 .. 8 bits) are
    each taken at distance 0 before its turn, the gate candidate (20 bits) is its ninth, two more
    (26 and 34 bits) follow.  Dictated: the gate candidate when the reference admits it (20 < 0.9
    * 26), else the tenth (26 < 0.9 * 34)."""
    offs = [(3, 2), (-4, 3), (5, -3), (-2, -5), (6, 4), (-6, -2), (2, 6), (-3, -6)]
    cands = [(F32(q[0] + a), F32(q[1] + b), d + 1) for d, (a, b) in enumerate(offs)]
    cands += [(gate_cand[0], gate_cand[1], 20), (F32(q[0] + 1), F32(q[1] - 2), 26), (F32(q[0] - 1), F32(q[1] + 1), 34)]
    for c in cands[:8] + cands[9:]:
        assert T.G.candidate(q[0], q[1], c[0], c[1], T.window), (T, gate, c)
    assert T.G.candidate(q[0], q[1], gate_cand[0], gate_cand[1], T.window) == inside, (T, gate, side, dirn)
    # the holders come first in F1; each is tied to the row's candidate h once the row exists
    base = len(T.q)
    r = base + 8
    for h in range(8):
        T.add("rescan holder", "in", dirn, (cands[h][0], cands[h][1]))
    i = T.add("rescan " + gate, side, dirn, q, cands, accept=8 if inside else 9)
    assert i == r
    for h in range(8):
        e = T.q[base + h]
        e.near, e.accepts, e.group = (r, h, 0), (r, h), r
    T.rescans.append(r)
    return i


# ---- tables ------------------------------------------------------------------------------------------
def box_table(rect, window):
    """|d| against r = window in each direction: lone candidate, and as the second best."""
    T = SfiTable("box", rect, window)
    r = F32(window)
    k = 0
    if window == 0:
        q = spot(40)
        T.add("box", "on", "0", q, [(q[0], q[1])], accept=0)
        for dirn in DIRS:
            k += 1
            q = spot(40 + k)
            c = step_out(dirn, q, 1)
            assert T.G.in_grid(*c) and not T.G.candidate(*q, *c, 0)
            T.add("box", "above", dirn, q, [c])
        # one cell: a query on a cell centre whose floor and ceil agree
        for n in range(18, 40):
            q = (T.G.coord(n, 0), T.G.coord(n + 1, 1))
            if T.G.raw_range(q[0], 0, 0) == (n, n) and T.G.raw_range(q[1], 0, 1) == (n + 1, n + 1):
                T.add("cells one cell", "on", "0", q, [q], accept=0)
                break
        else:  # (RECT_A always has it; in RECT_B no cell centre need be a float)
            assert rect != "A"
        return T
    for variant in ("box", "box second"):
        for dirn in DIRS:
            for side, kf in (("below", -1), ("on", 0), ("above", 1)):
                # a spot whose edge candidate stays inside the rectangle
                q = (F32(320.0 + 8 * (k % 5)), F32(256.0 + 8 * (k // 5)))
                k += 1
                c = step_out(dirn, along(dirn, q, r), kf)
                ax = 0 if dirn[1] == "x" else 1
                with np.errstate(all="ignore"):
                    d = abs(F32(c[ax] - q[ax]))
                # (the candidate's coordinate is the adjacent float; |d| itself is a float subtraction)
                assert side_of(c[ax], along(dirn, q, r)[ax]) == ("on" if kf == 0 else "above" if kf * (1 if dirn[0] == "+" else -1) > 0 else "below")
                assert (d < r, d == r, d > r) == (side == "below", side == "on", side == "above"), (rect, window, dirn, side, d)
                # the cell range holds the candidate on all three sides: the box test alone decides
                cx, cy = T.G.cells(q[0], r, 0), T.G.cells(q[1], r, 1)
                assert cx[0] <= T.G.pos(c[0], 0) <= cx[1] and cy[0] <= T.G.pos(c[1], 1) <= cy[1]
                inside = side != "above"
                assert T.G.candidate(*q, *c, r) == inside
                if variant == "box":
                    T.add("box", side, dirn, q, [c], accept=0 if inside else None)
                else:
                    T.add("box second", side, dirn, q, [(q[0], q[1], QDIST), (c[0], c[1], QDIST + 1)],
                          accept=None if inside else 0)
                    assert not F32(QDIST) < F32(F32(QDIST + 1) * F32(0.9))
    if window == 100:  # the exact rescan decides the same gate
        for dirn in DIRS:
            for side, kf in (("below", -1), ("on", 0), ("above", 1)):
                q = (F32(300.0 + 8 * (k % 5)), F32(240.0 + 8 * (k // 5)))
                k += 1
                c = step_out(dirn, along(dirn, q, r), kf)
                add_rescan(T, "box", side, dirn, q, c, side != "above")
    return T


def window_table(rect):
    """Window 40: PosInGrid's edges, the cell range, levels, non-finite inputs."""
    T = SfiTable("window", rect, 40)
    G, r = T.G, F32(40)
    # -- PosInGrid: the grid's first and last boundary on each axis
    for ax, name in ((0, "x"), (1, "y")):
        for upper in (False, True):
            out, inn = grid_edge(G, ax, upper)
            half = F32(G.n[ax] - 0.5 if upper else -0.5)
            other = spot(52 + 2 * ax + upper)[1 - ax]
            for v, is_in in ((out, False), (inn, True)):
                cf = G.cellf(v, ax)
                side = "on" if cf == half else "below" if cf < half else "above"
                p = (v, other) if ax == 0 else (other, v)
                q = list(p)
                q[ax] = F32(q[ax] + (-3 if upper else 3))  # the window holds the position, the box too
                assert (G.candidate(*q, *p, r)) == is_in and G.in_grid(*p) == is_in
                with np.errstate(all="ignore"):
                    assert not abs(F32(p[ax] - q[ax])) > r
                T.add("posingrid " + ("last + 0.5" if upper else "-0.5"), side, ("+" if upper else "-") + name, q, [p],
                      accept=0 if is_in else None)
                T.q[-1].row.inp["in"] = is_in
    # interior half cells (parity only, see the module docstring)
    for j, kc in enumerate((16, 17, 30)):
        for ax, name in ((0, "x"), (1, "y")):
            v = G.coord(kc + 0.5, ax)
            other = spot(60 + j)[1 - ax]
            p = (v, other) if ax == 0 else (other, v)
            assert G.candidate(p[0] + 2, p[1] + 2, *p, r)
            T.add("posingrid interior half cell", "on", "+" + name, (p[0] + 2, p[1] + 2), [p], accept=0)
    # -- the cell range: the candidate in the window's first / last column or row
    k = 0
    for ax, name in ((0, "x"), (1, "y")):
        for last in (False, True):
            for rescan in (False, True):
                found = None
                for t in range(200):
                    qa = F32(G.coord(14 + k, ax) + 0.5 * t)
                    rng_ = G.cells(qa, r, ax)
                    want = rng_[1] if last else rng_[0]
                    start = F32(qa + r) if last else F32(qa - r)
                    for u in range(64):
                        c = F32(start - 0.25 * u) if last else F32(start + 0.25 * u)
                        with np.errstate(all="ignore"):
                            if G.pos(c, ax) == want and not abs(F32(c - qa)) > r:
                                found = (qa, c, want)
                                break
                        if G.pos(c, ax) != want and u > 40:
                            break
                    if found:
                        break
                assert found, (rect, name, last)
                qa, c, want = found
                other = F32(G.coord(10 + 3 * k, 1 - ax))
                k += 1
                q = (qa, other) if ax == 0 else (other, qa)
                p = (c, other) if ax == 0 else (other, c)
                assert G.candidate(*q, *p, r) and G.pos(c, ax) == want
                dirn = ("+" if last else "-") + name
                gate = "cells " + ("last" if last else "first") + (" column" if ax == 0 else " row")
                if rescan:
                    add_rescan(T, gate, "in", dirn, q, p, True)
                else:
                    T.add(gate, "in", dirn, q, [p], accept=0)
    # clamped at column 0 / 63 and row 0 / 47, the candidate in the clamped cell
    for ax, name in ((0, "x"), (1, "y")):
        for upper in (False, True):
            last = G.n[ax] - 1
            qa = G.coord(last - 0.75 if upper else 0.75, ax)
            raw = G.raw_range(qa, r, ax)
            assert raw[1] > last if upper else raw[0] < 0
            c = scan(qa, qa + (30 if upper else -30), 0.25, lambda v: G.pos(v, ax) == (last if upper else 0))
            other = spot(70 + 2 * ax + upper)[1 - ax]
            q = (qa, other) if ax == 0 else (other, qa)
            p = (c, other) if ax == 0 else (other, c)
            assert G.candidate(*q, *p, r)
            T.add("cells clamped", "in", ("+" if upper else "-") + name, q, [p], accept=0)
    # windows entirely outside the grid: a keypoint waits in the nearest cell
    for ax, name in ((0, "x"), (1, "y")):
        for upper in (False, True):
            last = G.n[ax] - 1
            if upper:
                qa = scan(G.coord(last + 1, ax) + r, G.coord(last + 1, ax) + r + 40, 0.5, lambda v: G.raw_range(v, r, ax)[0] > last)
            else:
                qa = scan(G.coord(0, ax) - r, G.coord(0, ax) - r - 40, 0.5, lambda v: G.raw_range(v, r, ax)[1] < 0)
            assert G.cells(qa, r, ax) is None
            c = grid_edge(G, ax, upper)[1]
            other = spot(75 + 2 * ax + upper)[1 - ax]
            q = (qa, other) if ax == 0 else (other, qa)
            p = (c, other) if ax == 0 else (other, c)
            assert G.in_grid(*p) and not G.candidate(*q, *p, r)
            T.add("cells outside the grid", "out", ("+" if upper else "-") + name, q, [p])
    # -- levels
    q = spot(90)
    T.add("level F2 octave 1", "out", "0", q, [(q[0], q[1], QDIST, 1)])
    q = spot(91)
    T.add("level F1 octave 1", "out", "0", q, [(q[0], q[1], QDIST, 0)], octave=1)
    q = spot(92)  # (the octave-1 keypoint is nearer: it is skipped, not compared)
    T.add("level F2 octave 1 beside octave 0", "in", "0", q, [(q[0], q[1], 5, 1), (q[0] + 1, q[1], QDIST, 0)], accept=1)
    q = spot(94)  # an octave-1 query is skipped even where an octave-1 keypoint waits (level1 > 0)
    T.add("level F1 octave 1 on an octave-1 keypoint", "out", "0", q, [(q[0], q[1], QDIST, 1)], octave=1)
    # a keypoint held at distance 10 is dead for a later query at the same distance
    # (`vMatchedDistance[i2] <= dist`, ORBmatcher.cc:640): the holder keeps it
    q = spot(93)
    i = T.add("steal at equal distance: holder", "in", "0", q, [(q[0], q[1], QDIST)], accept=0)
    T.add_near("steal at equal distance", "on", "0", (i, 0), QDIST, accept=False)
    # -- non-finite vbPrevMatched: candidates wait in column 0 / row 0 / cell (0, 0) (NaN -> 0) and in
    # the last column / row (a saturated conversion), the finite coordinate inside the box
    x0, y0 = grid_edge(G, 0, False)[1], grid_edge(G, 1, False)[1]
    x9, y9 = grid_edge(G, 0, True)[1], grid_edge(G, 1, True)[1]
    fin = spot(100)
    for side, bad in (("nan", NAN), ("inf", INF), ("inf", -INF), ("1e12", F32(1e12)), ("1e12", F32(-1e12))):
        neg = not bad > 0  # NaN and the negative values look at cell 0
        ex, ey = (x0, y0) if neg else (x9, y9)
        T.add("nonfinite prev x", side, "-x" if neg else "+x", (bad, fin[1]), [(ex, fin[1])])
        T.add("nonfinite prev y", side, "-y" if neg else "+y", (fin[0], bad), [(fin[0], ey)])
        T.add("nonfinite prev x and y", side, "-x" if neg else "+x", (bad, bad), [(ex, ey)])
    for e in T.q:
        if e.row.inp["key"][0].startswith("nonfinite prev"):
            assert G.in_grid(*e.cands[0][:2]) and not G.candidate(*e.prev, *e.cands[0][:2], r)
    # -- non-finite F2 keypoints beside a finite one in cell (0, 0): the finite one is matched
    qc = (F32(x0 + 2), F32(y0 + 2))
    assert G.pos(qc[0], 0) == 0 and G.pos(qc[1], 1) == 0 and G.cells(qc[0], r, 0)[0] == 0
    for side, bx, by in (("nan", NAN, qc[1]), ("nan", qc[0], NAN), ("nan", NAN, NAN), ("inf", INF, qc[1]),
                         ("inf", -INF, qc[1]), ("inf", qc[0], INF), ("inf", qc[0], -INF), ("inf", -INF, -INF)):
        T.add("nonfinite F2 keypoint", side, "-x", qc, [(bx, by, QDIST), (qc[0], qc[1], 20)], accept=1)
    return T


def sparse_table(rect):
    """Window 8: two clusters of first / last column rows with empty grid columns around them."""
    T = SfiTable("sparse", rect, 8)
    G, r = T.G, F32(8)
    for c0 in (10, 24):
        for j in range(4):
            for last in (False, True):
                qx = None
                for t in range(60):
                    qa = F32(G.coord(c0, 0) + 0.25 * t)
                    cr = G.cells(qa, r, 0)
                    want = cr[1] if last else cr[0]
                    start = F32(qa + r) if last else F32(qa - r)
                    for u in range(40):
                        c = F32(start - 0.25 * u) if last else F32(start + 0.25 * u)
                        with np.errstate(all="ignore"):
                            if G.pos(c, 0) == want and not abs(F32(c - qa)) > r:
                                qx = (qa, c, cr)
                                break
                    if qx:
                        break
                assert qx
                qa, c, cr = qx
                y = G.coord(5 + 9 * j + 3 * last, 1)
                assert G.candidate(qa, y, c, y, r)
                i = T.add("cells sparse " + ("last" if last else "first") + " column", "in", "+x" if last else "-x", (qa, y),
                          [(c, y)], accept=0)
                T.sparse.append((i, cr))
    return T


def whole_table(rect):
    """Window 10000: every cell is in range and every keypoint in the box."""
    T = SfiTable("whole", rect, 10000)
    G = T.G
    x0, y0 = grid_edge(G, 0, False)[1], grid_edge(G, 1, False)[1]
    x9, y9 = grid_edge(G, 0, True)[1], grid_edge(G, 1, True)[1]
    for j, p in enumerate(((x0, y0), (x9, y9), (x0, y9), (x9, y0), spot(80))):
        q = spot(3 + j)
        assert G.cells(q[0], 10000, 0) == (0, 63) and G.cells(q[1], 10000, 1) == (0, 47) and G.candidate(*q, *p, 10000)
        T.add("cells whole grid", "in", "0", q, [p], accept=0)
    return T


# ---- rotation tables -----------------------------------------------------------------------------
def _ori_table(name, rect, pops):
    """pops: (gate, side, dirn, a1, a2) lone-candidate rows; returns the table."""
    T = SfiTable(name, rect, 40, ori=True)
    for j, (gate, side, dirn, a1, a2) in enumerate(pops):
        q = spot(j)
        T.add(gate, side, dirn, q, [(q[0], q[1], QDIST, 0, a2)], accept=0, angle=F32(a1))
    return T


def _anchors(bins, n=5):
    return [("anchor", "in", str(b), F32(30 * b), F32(0)) for b in bins for _ in range(n)]


def rotbin_tables():
    """One table per boundary rot = 15 + 30 k: bins k, k + 15 and k + 20 hold five anchors each
    and are kept; the boundary rows are kept exactly when they fall into bin k (bin k + 1 holds
    boundary rows only, at most four, and comes fourth)."""
    out = []
    third = F32(F32(1.0) / F32(30))
    assert F32(F32(15) * third) == F32(0.5)  # the one boundary that lands on .5 exactly
    for k in range(12):
        b = F32(15 + 30 * k)
        rows = []
        vals = [("below", down(b)), ("on", b), ("above", up(b))]
        # the last float of bin k, where the product at `below` already rounds past k + 0.5
        v = down(b)
        for _ in range(8):
            if rot_bin(v, F32(0)) == k:
                break
            v = down(v)
        assert rot_bin(v, F32(0)) == k and rot_bin(up(v), F32(0)) == k + 1
        if v != down(b):
            vals.append(("last of bin", v))
        for side, a1 in vals:
            rows.append(("rotbin", side, str(int(b)), a1, F32(0)))
        T = _ori_table(f"rotbin{int(b)}", "AB"[k % 2], _anchors((k, (k + 15) % 30, (k + 20) % 30)) + rows)
        T.expectation()
        assert set(T.keep) == {k, (k + 15) % 30, (k + 20) % 30} and T.hist[k + 1] <= 4
        assert rot_bin(b, F32(0)) == k + 1 and rot_bin(up(b), F32(0)) == k + 1
        out.append(T)
    # rot = -0.0f stays in bin 0 (`rot < 0` is false); alone in bin 12 it would be dropped
    T = _ori_table("rotbin-0", "A", _anchors((0, 20, 25)) + [("rotbin", "on", "-0", F32(-0.0), F32(0.0))])
    assert np.signbit(F32(F32(-0.0) - F32(0.0))) and rot_bin(F32(-0.0), F32(0.0)) == 0
    T.expectation()
    assert 0 in T.keep and 12 not in T.keep
    out.append(T)
    # a1 < a2 by a denormal: rot + 360 = 360 -> bin 12; rot = -15 -> 345 -> 11.5.. -> bin 12
    den = F32(1e-40)
    T = _ori_table("rotbin360", "B", _anchors((12, 20, 25)) + [("rotbin", "denormal", "360", F32(0), den),
                                                               ("rotbin", "on", "-15", F32(0), F32(15))])
    assert F32(F32(0) - den) < 0 and F32(F32(F32(0) - den) + F32(360)) == 360 and rot_bin(F32(0), den) == 12
    assert rot_bin(F32(0), F32(15)) == 12
    T.expectation()
    assert 12 in T.keep and 0 not in T.keep and 11 not in T.keep
    out.append(T)
    return out


def maxima_tables():
    """ComputeThreeMaxima's float comparisons `max2 < 0.1f * (float) max1`, `max3 < ...` at equality
    and one short of it, and its tie order."""
    out = []

    def table(name, counts, keep, rect="A"):
        pops = [("maxima", name, str(b), F32(30 * b), F32(0)) for b, n in counts for _ in range(n)]
        T = _ori_table("maxima " + name, rect, pops)
        T.expectation()
        assert [T.hist[b] for b, _ in counts] == [n for _, n in counts] and sum(T.hist) == sum(n for _, n in counts)
        assert sorted(x for x in T.keep if x >= 0) == sorted(keep), (name, T.keep, keep)
        T.maxima = (dict(counts), tuple(sorted(keep)))
        out.append(T)

    for m in (10, 20, 30):
        s = m // 10
        assert F32(0.1) * F32(m) == F32(s) and np.float64(F32(0.1)) * m > s  # kept in float, dropped in double
        table(f"max2 at equality ({m}, {s})", [(7, m), (19, s)], [7, 19], "AB"[s % 2])
        table(f"max3 at equality ({m}, {s + 2}, {s})", [(22, s), (4, m), (13, s + 2)], [4, 13, 22], "AB"[s % 2])
        if s > 1:  # one entry fewer: dropped
            table(f"max2 one short ({m}, {s - 1})", [(7, m), (19, s - 1)], [7])
            table(f"max3 one short ({m}, {s + 2}, {s - 1})", [(22, s - 1), (4, m), (13, s + 2)], [4, 13])
        else:  # (10, 0) is an empty bin: one entry more in max1 instead
            table("max2 one short (11, 1)", [(7, 11), (19, 1)], [7])
            table("max3 one short (11, 3, 1)", [(22, 1), (4, 11), (13, 3)], [4, 13])
    # four bins of equal count in non-monotone positions: the three lowest-numbered stay
    table("four equal bins", [(17, 4), (3, 4), (25, 4), (9, 4)], [3, 9, 17], "B")
    # equal second and third, a fourth below them
    table("equal second and third", [(20, 3), (5, 6), (2, 3), (28, 2)], [2, 5, 20])
    # equal first and second, the third tied with a fourth: the lower bin stays
    table("tie for third", [(11, 5), (6, 5), (27, 2), (14, 2)], [6, 11, 14], "B")
    # bin 9 reaches the top three (4 entries against bin 16's 3) only through three queries that were
    # accepted and later robbed: their entries stay in rotHist (ORBmatcher.cc:664-676)
    T = SfiTable("maxima robbed", "A", 40, ori=True)
    k = 0

    def lone(b, gate="maxima"):
        nonlocal k
        q = spot(k)
        k += 1
        return T.add(gate, "robbed", str(b), q, [(q[0], q[1], QDIST, 0, F32(0))], accept=0, angle=F32(30 * b))

    victims = [lone(9) for _ in range(3)]
    lone(9)
    for _ in range(3):
        lone(16)
    for _ in range(3):
        lone(21)
    for _ in range(2):
        lone(2)
    for v in victims:  # the robbers come later, 5 bits from the victims' candidates, and vote for bin 2
        T.add_near("maxima robber", "robbed", "2", (v, 0), 5, robs=True, angle=F32(60))
    T.expectation()
    assert (T.hist[9], T.hist[16], T.hist[21], T.hist[2]) == (4, 3, 3, 5) and sorted(T.keep) == [2, 9, 16]
    live9 = [i for i, e in enumerate(T.q) if T.bin_of.get(i) == 9 and not e.robbed]
    assert len(live9) == 1  # without the robbed entries bin 9 would hold 1 and lose to bins 16 and 21
    T.maxima = ({9: 4, 16: 3, 21: 3, 2: 5}, (2, 9, 16))
    out.append(T)
    return out


@functools.lru_cache(maxsize=None)
def all_tables():
    """Every table: (rect, window) of the geometric gates with checkOri off, then the orientation tables."""
    T = []
    for rect in ("A", "B"):
        T += [box_table(rect, 100), box_table(rect, 40), box_table(rect, 0), window_table(rect), sparse_table(rect),
              whole_table(rect)]
    T += rotbin_tables() + maxima_tables()
    for t in T:
        b = t.build(0, MAX_LEAD2)
        # sparse rows: three empty grid columns on either side of the window, fillers included
        cols = {t.G.pos(x, 0) for x, y in zip(b["k2"]["x"], b["k2"]["y"]) if t.G.in_grid(x, y)}
        for i, (lo, hi) in t.sparse:
            assert not cols & (set(range(lo - 3, lo)) | set(range(hi + 1, hi + 4))), (t, i)
        t.build()
    return tuple(T)


MAX_LEAD2 = 1100  # the most F2 fillers any test adds (the large-capacity body)
