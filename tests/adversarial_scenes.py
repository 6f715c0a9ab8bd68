"""TEST INFRASTRUCTURE: deterministic matcher scenes whose result is known by construction.

The seeded random scenes of tests/scenes.py leave three things to chance that the parallel
resolvers (k_resolve_fix, k_resolve, k_match_init, k_bow_pairs) depend on; the builders here
pin them:

* chain scenes: query q's decision depends on what query q-1 accepted, for every q, so the
  sequential result is reached only by carrying state through the whole chain
  (`chain_scene`, kinds A and B below);
* ratio tables: pairs that sit exactly on, just below and just above every acceptance rule's
  float comparison and integer cut (`ratio_table`);
* node sweeps: vocabulary nodes of every size at which k_bow_pairs switches path
  (`node_sweep`), with a plain Python loop over a node as the expectation (`bow_loop`).

Chain kinds (targets T are a random walk, T[q] = T[q-1] with STEP distinct bits flipped, the
bits of consecutive steps disjoint; T[-1] is a start descriptor that no target carries):
  A  "own 20 / prev 22": Q[q] = T[q-1] with the first 22 bits of step q flipped.  Alone, q is
     rejected by every ratio test (20 is not below nnratio * 22 for nnratio <= 0.9); once q-1
     holds T[q-1] the second best is >= 55 away and q accepts T[q].  Remove the head and
     nothing matches.
  B  "prev 10 / own 30": Q[q] = T[q-1] with the first 10 bits of step q flipped.  Alone, q
     takes T[q-1]; in sequence q takes T[q].  Remove query k and every later query takes its
     predecessor's target: the mapping shifts by one from k on.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from orbslam_jpminipc_amd import KEYPOINT_DTYPE
from orbslam_jpminipc_amd.views import FeatureVector, MapPointSet, View

import scenes as S
from test_matcher_oracle import rot_bin, three_maxima

F32 = np.float32
INT_MAX = 2**31 - 1
W, H = S.W, S.H
# far: every off-chain distance is at least this (asserted).  A: beyond TH_LOW, and 20 < 0.6 * 55.
# B: a link's third candidate only has to lose to its own target (30 <= 0.9 * 45 for the ratio rules).
KIND = {"A": dict(step=42, near=22, prev=22, own=20, far=55), "B": dict(step=40, near=10, prev=10, own=30, far=45)}


# ---- descriptors at exact distances ----------------------------------------------------------
def flip_bits(d, bits):
    """Copy of descriptor `d` (32 bytes) with the listed bit positions (0..255) flipped."""
    d = np.array(d, np.uint8).reshape(32).copy()
    for b in np.asarray(bits, np.int64).reshape(-1):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def at_distance(rng, d, k):
    """A descriptor at Hamming distance exactly `k` from `d`."""
    return flip_bits(d, rng.choice(256, int(k), replace=False))


def _pack(bits):
    return np.packbits(np.asarray(bits, np.uint8), axis=-1, bitorder="little")


def hamming_matrix(A, B):
    """All pairwise Hamming distances of two descriptor arrays, (len(A), len(B)) int32."""
    a = np.unpackbits(np.asarray(A, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    b = np.unpackbits(np.asarray(B, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    return np.rint(a @ (1 - b).T + (1 - a) @ b.T).astype(np.int32)


def chain_descriptors(rng, n, kind):
    """(Q, T) of an n-link chain.  Step q flips STEP random bits of one half of the descriptor
    (even q the low 128 bits, odd q the high ones: consecutive steps are disjoint), so
    d(Q[q], T[q-1]) = prev, d(Q[q], T[q]) = own, d(Q[q], T[q+1]) = own + STEP and
    d(Q[q], T[q-2]) = prev + STEP exactly; every other distance is asserted >= KIND[kind]["far"]."""
    p = KIND[kind]
    order = np.argsort(rng.random((n, 128)), axis=1)[:, : p["step"]] + 128 * (np.arange(n)[:, None] & 1)
    step = np.zeros((n, 256), bool)
    near = np.zeros((n, 256), bool)
    np.put_along_axis(step, order, True, 1)
    np.put_along_axis(near, order[:, : p["near"]], True, 1)
    start = rng.integers(0, 2, 256).astype(bool)
    tb = np.logical_xor.accumulate(np.vstack([start[None], step]), axis=0)  # tb[q + 1] = T[q]
    Q, T = _pack(tb[:-1] ^ near), _pack(tb[1:])
    D = hamming_matrix(Q, T)
    i = np.arange(n)
    assert (D[i, i] == p["own"]).all() and (D[i[1:], i[:-1]] == p["prev"]).all()
    D[i, i] = D[i[1:], i[:-1]] = 255
    assert D.min() >= p["far"], D.min()
    return Q, T


# ---- keypoints -------------------------------------------------------------------------------
def kps_at(x, y, octave=0, angle=0.0):
    x = np.asarray(x, np.float32).reshape(-1)
    k = np.zeros(len(x), KEYPOINT_DTYPE)
    k["x"], k["y"] = x, np.asarray(y, np.float32).reshape(-1)
    k["octave"] = octave
    k["angle"] = angle
    k["size"] = 31 * S.SF[k["octave"]]
    k["response"] = 50
    k["class_id"] = -1
    return k


def target_view(kps, desc):
    """A Frame / KeyFrame at the world origin looking down +z (identity pose)."""
    return View(kps, desc, (0, W, 0, H), S.NLEVELS, 1.2, S.CALIB, np.eye(3), np.zeros(3))


GRID_STEP, GRID_COLS, GRID_X0, GRID_Y0 = 10.0, 60, 25.0, 25.0
SHORT_WINDOW = 12  # box half-width: a query sees its two chain targets and at most 4 neighbours
LONG_WINDOW = 100


def serpentine(n):
    """Target t on a 10 px grid walked row by row, alternate rows reversed (consecutive targets
    are grid neighbours); query q halfway between T[q-1] and T[q] (q = 0: half a step before
    T[0])."""
    t = np.arange(n)
    r, c = t // GRID_COLS, t % GRID_COLS
    c = np.where(r & 1, GRID_COLS - 1 - c, c)
    tx, ty = GRID_X0 + GRID_STEP * c, GRID_Y0 + GRID_STEP * r
    assert tx.max() < W - 20 and ty.max() < H - 20
    px, py = np.concatenate([[tx[0] - GRID_STEP], tx[:-1]]), np.concatenate([[ty[0]], ty[:-1]])
    return (tx + px) / 2, (ty + py) / 2, tx, ty


def packed(n):
    """All targets on a 1 px grid inside one window, every query at its centre: each candidate
    list is the whole chain (truncated by the GPU's top-k lists: the exact rescans decide)."""
    assert n <= 200
    t = np.arange(n)
    tx, ty = 300.0 + (t % 20), 200.0 + (t // 20)
    return np.full(n, 310.0), np.full(n, 205.0), tx, ty


def box_counts(qx, qy, tx, ty, r):
    """Targets inside each query's search box (|dx| <= r and |dy| <= r), plain numpy."""
    return ((np.abs(tx[None] - qx[:, None]) <= r) & (np.abs(ty[None] - qy[:, None]) <= r)).sum(1)


ORI_PATTERN = np.array([1, 1, 1, 1, 2, 2, 2, 3, 3, 4])  # rotation bin of chain link q, by q % 10


@dataclass
class Chain:
    kind: str
    n: int
    lead: int
    broken: int | None
    window: int
    Q: View  # query frame: `lead` unusable fillers, then the chain's queries
    T: View  # target frame (identity pose)
    usable: np.ndarray  # per query row
    taken0: np.ndarray  # per target: taken before the call
    by_target: np.ndarray  # expected out[target] = query row or -1, orientation check off
    by_target_ori: np.ndarray  # the same with the orientation check on

    @property
    def count(self):
        return int((self.by_target >= 0).sum())

    @property
    def count_ori(self):
        return int((self.by_target_ori >= 0).sum())

    def by_query(self, ori=False):
        """Expected match12[query row] = target or -1."""
        bt = self.by_target_ori if ori else self.by_target
        out = np.full(self.Q.n, -1, np.int32)
        t = np.flatnonzero(bt >= 0)
        out[bt[t]] = t
        return out


def rot_filter(pairs_q_angle, pairs_t_angle):
    """keep[i] for accepted pairs i: the pair's rotation bin is one of ComputeThreeMaxima's."""
    bins = np.array([rot_bin(a, b) for a, b in zip(pairs_q_angle, pairs_t_angle)], np.int64)
    hist = [[] for _ in range(30)]
    for i, b in enumerate(bins):
        hist[b].append(i)
    keep = three_maxima(hist)
    return np.isin(bins, [k for k in keep if k >= 0])


def chain_scene(rng, n, kind, layout="short", lead=0, broken=None, take_first=False, disabled_octave=None):
    """An n-link chain of `kind` as a query frame and a target frame, all octave 0.

    layout "short": serpentine grid, SHORT_WINDOW sees the chain neighbours and at most 8
    targets (asserted); "long": everything in one LONG_WINDOW (n <= 200).
    lead: unusable filler queries before the chain (the chain starts at every alignment of the
    speculation groups).  broken = k: chain query k unusable.  take_first: T[0] taken before the
    call (kind A, ratio matchers with TH_LOW: query 0 has nothing left, query 1 finds T[0] taken
    as if query 0 had matched, so exactly the links 1 .. n-1 match).
    disabled_octave: octave given to the unusable queries (SearchForInitialization has no usable
    flag: it skips octave > 0).
    Query angles put link q's pair into rotation bin ORI_PATTERN[q % 10] (40/30/20/10 % of the
    pairs in bins 1..4): ComputeThreeMaxima keeps bins 1, 2, 3 and the orientation check drops
    the 10 % in bin 4.
    """
    Qd, Td = chain_descriptors(rng, n, kind)
    qx, qy, tx, ty = serpentine(n) if layout == "short" else packed(n)
    window = SHORT_WINDOW if layout == "short" else LONG_WINDOW
    cnt = box_counts(qx, qy, tx, ty, window)
    i = np.arange(n)
    inside = (np.abs(tx - qx) <= window) & (np.abs(ty - qy) <= window)
    inside[1:] &= (np.abs(tx[:-1] - qx[1:]) <= window) & (np.abs(ty[:-1] - qy[1:]) <= window)
    assert inside.all(), "a query does not see its chain targets"
    if layout == "short":
        assert cnt.max() <= 8 and cnt.min() >= 1, (cnt.min(), cnt.max())
    else:
        assert (cnt == n).all()
    usable = np.ones(lead + n, np.uint8)
    usable[:lead] = 0
    if broken is not None:
        usable[lead + broken] = 0
    qang = np.concatenate([np.zeros(lead), 30.0 * ORI_PATTERN[i % 10] + 5.0]).astype(np.float32)
    qk = kps_at(np.concatenate([np.full(lead, qx[0]), qx]), np.concatenate([np.full(lead, qy[0]), qy]), 0, qang)
    if disabled_octave is not None:
        qk["octave"][usable == 0] = disabled_octave
        qk["size"] = 31 * S.SF[qk["octave"]]
    Qdesc = np.vstack([S.descriptors(rng, lead), Qd]) if lead else Qd
    taken0 = np.zeros(n, np.uint8)
    by_t = np.full(n, -1, np.int32)
    k = n if broken is None else broken
    by_t[:k] = lead + i[:k]
    if kind == "B" and broken is not None:
        by_t[k : n - 1] = lead + i[k + 1 :]
    if take_first:
        assert kind == "A" and broken is None and layout == "short"  # (query 0 must see nothing but T[0])
        taken0[0] = 1
        by_t[0] = -1
    by_o = by_t.copy()
    acc = np.flatnonzero(by_t >= 0)
    keep = rot_filter(qang[by_t[acc]], np.zeros(len(acc), np.float32))
    by_o[acc[~keep]] = -1
    return Chain(kind, n, lead, broken, window, View(qk, Qdesc, (0, W, 0, H)), target_view(kps_at(tx, ty), Td), usable,
                 taken0, by_t, by_o)


def map_points_at(V: View, kps, desc, depth=5.0, kind="reloc"):
    """MapPoints that view V (identity pose) sees at the pixels of `kps`, with descriptors `desc`.
    Relocalisation predicts level 0 (dist / dmin <= 1); the Sim3 projections and Fuse need
    dmin <= dist <= dmax, so they predict level 1 and search 1.2 * th."""
    P = S.backproject(V, kps["x"], kps["y"], np.full(len(kps), depth))
    PO = P.astype(np.float64) - V.Ow.astype(np.float64)
    dist = np.linalg.norm(PO, axis=1)
    dmin = dist * (1.05 if kind == "reloc" else 0.9)
    return MapPointSet(P, (PO / dist[:, None]).astype(np.float32), dmin.astype(np.float32), (dist * 3).astype(np.float32),
                       desc)


def chain_map_points(C: Chain, kind="reloc"):
    """MapPoints seen at the query keypoints' pixels from the target frame."""
    return map_points_at(C.T, C.Q.kps, C.Q.desc, kind=kind)


def chain_bow(C: Chain, node=5, duplicate=False):
    """The chain as one vocabulary node of a KeyFrame (queries) and a Frame / KeyFrame (targets).
    duplicate: the query vector lists feature 0 a second time under a node the target vector
    lacks (the host entry points then take the generic resolver, the result is unchanged)."""
    d1 = {node: list(range(C.Q.n))}
    d2 = {node: list(range(C.T.n))}
    if duplicate:
        d1[node + 1000] = [0]
    return FeatureVector.from_dict(d1), FeatureVector.from_dict(d2)


# ---- acceptance rules in float32, as the reference evaluates them -----------------------------
def _f(d):
    return F32(2147483648.0) if d >= INT_MAX else F32(d)


def rule(name, nnratio, orbdist=100):
    """accept(d1, d2) of matcher `name` for best / second-best distances (d2 = INT_MAX: none;
    levels equal), evaluated in float32 exactly as written in the reference."""
    r = F32(nnratio)
    return {
        "bow_kf_f": lambda a, b: a <= 50 and _f(a) < r * _f(b),
        "bow_kf_kf": lambda a, b: a < 50 and _f(a) < r * _f(b),
        "sfi": lambda a, b: a <= 50 and _f(a) < _f(b) * r,
        "window": lambda a, b: a <= 100 and _f(a) <= _f(b) * r,
        "f2f": lambda a, b: a <= 100 and _f(a) <= _f(b) * r,
        "local": lambda a, b: a <= 100 and not (b < INT_MAX and _f(a) > r * _f(b)),
        "motion": lambda a, b: a <= 100,
        "reloc": lambda a, b: a <= orbdist,
        "sim3": lambda a, b: a <= 50,
        "fuse": lambda a, b: a <= 50,
        "triang": lambda a, b: a <= 50,
        "sim3_pair": lambda a, b: a <= 100,
    }[name]


# ---- ratio / threshold tables ----------------------------------------------------------------
@dataclass
class Table:
    rows: list  # (d1, d2 or None)
    Q: View
    T: View
    best: np.ndarray  # target index of each row's best candidate
    fvq: FeatureVector
    fvt: FeatureVector
    window: int = 4

    def expect(self, name, nnratio, orbdist=100):
        """(count, out-by-target, out-by-query) under matcher `name`'s rule."""
        acc = np.array([rule(name, nnratio, orbdist)(d1, INT_MAX if d2 is None else d2) for d1, d2 in self.rows])
        by_t = np.full(self.T.n, -1, np.int32)
        by_q = np.full(self.Q.n, -1, np.int32)
        q = np.flatnonzero(acc)
        by_t[self.best[q]] = q
        by_q[q] = self.best[q]
        return int(acc.sum()), by_t, by_q

    def exact_ties(self, nnratio):
        return sum(1 for d1, d2 in self.rows if d2 is not None and F32(d1) == F32(nnratio) * F32(d2))


TABLE_SINGLES = (49, 50, 51, 99, 100, 101, 63, 64, 65)  # TH_LOW, TH_HIGH, ORBdist = 64, each +-1


def ratio_rows(nnratio):
    rows = []
    for d2 in range(2, 84):
        x = nnratio * d2
        for d1 in sorted({int(np.floor(x)) - 1, int(np.floor(x)), int(np.ceil(x))}):
            if 0 <= d1 <= d2:
                rows.append((d1, d2))
    return rows


def ratio_table(rng, nnratio, singles=True, pairs=True):
    """One isolated query per row: two candidates at exact distances (d1, d2) from it (d1 the
    best; in every other row the second best comes first in index order) or, for the
    single-candidate rows, one at d1.  Row i sits alone at its own spot of a 30 px lattice
    (windows of 4 px) and in its own vocabulary node."""
    rows = (ratio_rows(nnratio) if pairs else []) + ([(d, None) for d in TABLE_SINGLES] if singles else [])
    assert len(rows) <= 21 * 15
    qd = S.descriptors(rng, len(rows))
    td, tx, ty, best, n1, n2 = [], [], [], [], {}, {}
    i = np.arange(len(rows))
    sx, sy = 20.0 + 30.0 * (i % 21), 20.0 + 30.0 * (i // 21)
    for r, (d1, d2) in enumerate(rows):
        first = len(td)
        a = at_distance(rng, qd[r], d1)
        if d2 is None:
            td += [a]
        else:
            b = at_distance(rng, qd[r], d2)
            td += [b, a] if r & 1 else [a, b]
        # (d1 == d2: the first in index order is the best; both share a grid cell, so every scan agrees)
        best.append(first + (1 if d2 is not None and d1 != d2 and r & 1 else 0))
        for j in range(first, len(td)):
            tx.append(sx[r] + (1.0 if j == best[-1] else -1.0))
            ty.append(sy[r] + (0.0 if j == best[-1] else 1.0))
        n1[10 * r + 3] = [r]
        n2[10 * r + 3] = list(range(first, len(td)))
    td = np.array(td, np.uint8)
    D = hamming_matrix(qd, td)
    for r, (d1, d2) in enumerate(rows):
        assert D[r, best[r]] == d1 and (d2 is None or D[r, n2[10 * r + 3]].max() == d2)
    return Table(rows, View(kps_at(sx, sy), qd, (0, W, 0, H)), target_view(kps_at(tx, ty), td), np.array(best),
                 FeatureVector.from_dict(n1), FeatureVector.from_dict(n2))


# ---- SearchByBoW as a plain loop over the nodes ------------------------------------------------
def bow_loop(kf_kf, nnratio, Q, uq, fvq, T, ut, fvt, stats=None):
    """SearchByBoW without the orientation check, node by node: (count, by-target, by-query).
    stats (dict node -> set): which of the three dependency outcomes each acceptance produced
    for the node's next three usable queries ("best", "second", "neither" of them lost)."""
    acc = rule("bow_kf_kf" if kf_kf else "bow_kf_f", nnratio)
    taken = np.zeros(T.n, bool)
    by_t, by_q = np.full(T.n, -1, np.int32), np.full(Q.n, -1, np.int32)
    tn = {int(x): k for k, x in enumerate(fvt.nodes)}

    def best2(D, q, cand, free):
        d = np.where(free, D[q], 1 << 20)
        j1 = int(np.argmin(d))  # first minimum in candidate order
        if d[j1] >= 1 << 20:
            return -1, -1, INT_MAX, INT_MAX
        d1 = int(d[j1])
        d[j1] = 1 << 20
        j2 = int(np.argmin(d))
        return j1, (j2 if d[j2] < 1 << 20 else -1), d1, (int(d[j2]) if d[j2] < 1 << 20 else INT_MAX)

    for a, node in enumerate(fvq.nodes):
        b = tn.get(int(node))
        if b is None:
            continue
        qs = fvq.features[fvq.offsets[a] : fvq.offsets[a + 1]]
        cand = fvt.features[fvt.offsets[b] : fvt.offsets[b + 1]]
        if len(cand) == 0:
            continue
        D = hamming_matrix(Q.desc[qs], T.desc[cand])
        ok = np.ones(len(cand), bool) if (ut is None or not kf_kf) else ut[cand].astype(bool)
        live = [i for i, q in enumerate(qs) if uq is None or uq[q]]
        for pos, i in enumerate(live):
            free = ok & ~taken[cand]
            j1, _, d1, d2 = best2(D, i, cand, free)
            if j1 < 0 or not acc(d1, d2):
                continue
            if stats is not None:
                for i2 in live[pos + 1 : pos + 4]:
                    k1, k2, _, _ = best2(D, i2, cand, free)
                    stats.setdefault(int(node), set()).add("best" if k1 == j1 else "second" if k2 == j1 else "neither")
            taken[cand[j1]] = True
            by_t[cand[j1]], by_q[qs[i]] = qs[i], cand[j1]
    n = int((by_t >= 0).sum())
    return (n, by_t, by_q)


@dataclass
class Sweep:
    Q: View
    T: View
    fvq: FeatureVector
    fvt: FeatureVector
    uq: np.ndarray
    ut: np.ndarray
    shapes: dict  # node id -> (nc, nq)
    tie_nodes: list


def node_sweep(rng, sizes_c, sizes_q, tie_every=7):
    """One frame pair with a node for every (nc, nq) of sizes_c x sizes_q.

    A node's candidates are a kind-A-like walk C[0..nc) (42-bit steps, consecutive ones
    disjoint); its i-th query aims at c = i % nc and is, by i % 4:
      0  C[c] + 3 bits: accepts C[c] whenever it is free;
      1  22 from C[c-1], 20 from C[c]: accepts C[c] only once C[c-1] is gone (chain A link);
      2  10 from C[c-1], 32 from C[c]: takes C[c-1] if free, else maybe C[c] (chain B link);
      3  C[c-1] + 5 bits: competes with the two before it for C[c-1].
    so acceptances take later queries' best, their second, or neither (bow_loop's stats).  In
    every `tie_every`-th node the last candidate repeats the one before it (equal distances: the
    first in candidate order is the best).  Every third query overall is unusable, as is every
    fifth target.  Feature indices are scattered over both frames, ascending within a node."""
    shapes = [(c, q) for c in sizes_c for q in sizes_q]
    NQ, NC = sum(q for _, q in shapes), sum(c for c, _ in shapes)
    pq, pc = rng.permutation(NQ), rng.permutation(NC)
    qd, td = np.zeros((NQ, 32), np.uint8), np.zeros((NC, 32), np.uint8)
    d1, d2, info, ties = {}, {}, {}, []
    oq = oc = 0
    for k, (nc, nq) in enumerate(shapes):
        node = 100 + 7 * k
        Qc, Cc = chain_descriptors(rng, nc, "A")  # Cc[c]; Qc[c] = 22 from C[c-1], 20 from C[c]
        if k % tie_every == tie_every - 1 and nc >= 2:
            Cc[nc - 1] = Cc[nc - 2]
            ties.append(node)
        iq, ic = np.sort(pq[oq : oq + nq]), np.sort(pc[oc : oc + nc])
        oq, oc = oq + nq, oc + nc
        for i in range(nq):
            c = i % nc
            m = i % 4  # (c = 0 has no predecessor: its queries aim at C[0] alone)
            if m == 0:
                q = at_distance(rng, Cc[c], 3)
            elif m == 1:
                q = Qc[c]
            elif m == 2 and c > 0:
                diff = np.flatnonzero(np.unpackbits(Cc[c - 1] ^ Cc[c], bitorder="little"))
                q = flip_bits(Cc[c - 1], diff[:10])
            elif m == 2:
                q = at_distance(rng, Cc[c], 32)
            else:
                q = at_distance(rng, Cc[c - 1] if c > 0 else Cc[c], 5)
            qd[iq[i]] = q
        td[ic] = Cc
        d1[node], d2[node] = iq.tolist(), ic.tolist()
        info[node] = (nc, nq)
    uq = (np.arange(NQ) % 3 != 2).astype(np.uint8)
    ut = (np.arange(NC) % 5 != 4).astype(np.uint8)
    ang_q = (30.0 * ORI_PATTERN[np.arange(NQ) % 10] + 5.0).astype(np.float32)
    Q = View(kps_at(rng.uniform(20, W - 20, NQ), rng.uniform(20, H - 20, NQ), 0, ang_q), qd, (0, W, 0, H))
    T = target_view(kps_at(rng.uniform(20, W - 20, NC), rng.uniform(20, H - 20, NC)), td)
    return Sweep(Q, T, FeatureVector.from_dict(d1), FeatureVector.from_dict(d2), uq, ut, info, ties)


def apply_rot_filter(by_key, q_of, t_of, Q, T):
    """Drop from an expected result (index array, -1 = none) the pairs outside the three
    rotation maxima.  q_of / t_of map (position, value) of an accepted entry to its query /
    target row."""
    out = by_key.copy()
    pos = np.flatnonzero(by_key >= 0)
    if len(pos) == 0:
        return 0, out
    qa = Q.kps["angle"][[q_of(p, by_key[p]) for p in pos]]
    ta = T.kps["angle"][[t_of(p, by_key[p]) for p in pos]]
    keep = rot_filter(qa, ta)
    out[pos[~keep]] = -1
    return int(keep.sum()), out


# ---- large frames, vectorised ----------------------------------------------------------------
def big_bow_pair(rng, n1, n2, per_node=10):
    """Two frames of n1 / n2 features over ~n1 / per_node shared nodes, built without a Python
    loop over features.  Frame 1's descriptors are node-wise pool entries with ~15 bits
    flipped (near-duplicates inside a node: second-best candidates that matter); frame 2's
    features are copies of random frame-1 features with ~5 more bits flipped, nine in ten in
    their source's node (true counterparts, several queries per target and the reverse)."""
    nn = max(n1 // per_node, 1)
    ids = np.sort(rng.choice(10**6, nn, replace=False)).astype(np.uint32)
    pool = S.descriptors(rng, 4 * nn)

    def frame(a, desc):
        n = len(a)
        k = kps_at(rng.uniform(20, W - 20, n), rng.uniform(20, H - 20, n), 0, rng.choice([0.0, 35.0, 65.0], n))
        order = np.argsort(a, kind="stable")
        cnt = np.bincount(a, minlength=nn)
        has = cnt > 0
        off = np.concatenate([[0], np.cumsum(cnt[has])])
        return target_view(k, desc), FeatureVector(ids[has], off, order)

    a1 = rng.integers(0, nn, n1)
    d1 = pool[4 * a1 + rng.integers(0, 4, n1)] ^ _pack(rng.random((n1, 256)) < 0.06)
    src = rng.integers(0, n1, n2)
    a2 = np.where(rng.random(n2) < 0.9, a1[src], rng.integers(0, nn, n2))
    d2 = d1[src] ^ _pack(rng.random((n2, 256)) < 0.02)
    V1, fv1 = frame(a1, d1)
    V2, fv2 = frame(a2, d2)
    return V1, fv1, V2, fv2


# ---- one call surface for the GPU matcher and the oracle ---------------------------------------
GRID_MODES = ("window", "local", "f2f", "motion", "reloc", "sim3")
ORI_MODES = ("window", "motion", "reloc")  # grid matchers with a rotation histogram


def table_chain(Tb: Table) -> Chain:
    """A ratio table in the shape run_grid takes (every query usable, nothing taken)."""
    none = np.full(Tb.T.n, -1, np.int32)
    return Chain("table", Tb.Q.n, 0, None, Tb.window, Tb.Q, Tb.T, np.ones(Tb.Q.n, np.uint8), np.zeros(Tb.T.n, np.uint8),
                 none, none)


def run_grid(m, mode, C: Chain, taken=None, orbdist=100):
    """Matcher `m` (orbslam_jpminipc_amd.ORBmatcher or oracle_lib.OracleMatcher) in `mode` over
    chain scene C with the search box of C.window.  Returns (count, out-by-target)."""
    Q, T, u, w = C.Q, C.T, C.usable, C.window
    if mode == "window":
        return m.WindowSearch(Q, u, T, w)
    if mode == "local":  # r = 2.5 * th at view_cos 1 and level 0
        return m.SearchByProjection_Local(T, taken, u, Q.kps["x"], Q.kps["y"], np.zeros(Q.n, np.int32),
                                          np.ones(Q.n, np.float32), Q.desc, w / 2.5)
    if mode == "f2f":
        return m.SearchByProjection_F2F(Q, chain_map_points(C), u, T, taken, w)
    if mode == "motion":
        return m.SearchByProjection_Motion(T, taken, Q, chain_map_points(C), u, float(w))
    if mode == "reloc":
        return m.SearchByProjection_Reloc(T, taken, Q, chain_map_points(C), u, float(w), orbdist)
    if mode == "sim3":  # predicted level 1: radius 1.2 * th
        return m.SearchByProjection_Sim3(T, taken, chain_map_points(C, kind="sim3"), u, int(w / 1.2))
    raise ValueError(mode)


F12_ROWS = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32)  # epipolar line of (x1, y1): y2 = y1


def run_table_by_query(m, name, Tb: Table):
    """Fuse / SearchForTriangulation / SearchBySim3 over a ratio table (all report by query; the
    first two cut the best distance at TH_LOW, the third at TH_HIGH in both directions).  The
    table's best candidates lie on their query's image row, the second ones one pixel off it:
    inside 3.84 sigma^2 as well, but later in the triangulation walk.  SearchBySim3 runs with the
    identity similarity between two keyframes at the origin: query i finds its best candidate
    and that candidate finds query i (the only keypoint of the query frame in its reach)."""
    if name == "sim3_pair":
        K1 = target_view(Tb.Q.kps, Tb.Q.desc)
        eye, zero = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
        return m.SearchBySim3(K1, map_points_at(K1, K1.kps, K1.desc, kind="sim3"), None, Tb.T,
                              map_points_at(Tb.T, Tb.T.kps, Tb.T.desc, kind="sim3"), None, eye, zero, eye, zero,
                              Tb.window / 1.2)
    if name == "fuse":  # predicted level 1: radius 1.2 * th, levels 0 .. 1
        return m.Fuse(Tb.T, chain_map_points(table_chain(Tb), kind="sim3"), None, Tb.window / 1.2)
    h1, h2 = np.zeros(Tb.Q.n, np.uint8), np.zeros(Tb.T.n, np.uint8)
    return m.SearchForTriangulation(Tb.Q, h1, Tb.fvq, Tb.T, h2, Tb.fvt, F12_ROWS)


def triangulation_scene(rng, n, lead=0, broken=None):
    """A kind-B chain for SearchForTriangulation: one node, every keypoint on the image row
    y = 240.  With F12 = [0 0 0; 0 0 -1; 0 1 0] (a translation along x between two cameras with
    equal fy, up to scale) the epipolar line of (x1, y1) is y2 = y1 and the squared distance of
    a candidate to it is (y2 - y1)^2 = 0, so every link passes CheckDistEpipolarLine exactly.
    The walk takes the first unmatched candidate within 2 * bestDist: T[q-1] (10) alone, T[q]
    (30) once T[q-1] is matched.  Returns (V1, has_mp1, fv1, V2, fv2, F12, expected match12,
    expected match12 under the orientation check)."""
    Qd, Td = chain_descriptors(rng, n, "B")
    i = np.arange(n)
    qang = np.concatenate([np.zeros(lead), 30.0 * ORI_PATTERN[i % 10] + 5.0]).astype(np.float32)
    V1 = View(kps_at(np.concatenate([np.full(lead, 40.0), 50.0 + 2.5 * i]), np.full(lead + n, 240.0), 0, qang),
              np.vstack([S.descriptors(rng, lead), Qd]) if lead else Qd, (0, W, 0, H))
    V2 = target_view(kps_at(52.0 + 2.5 * i, np.full(n, 240.0)), Td)
    h1 = np.zeros(lead + n, np.uint8)
    h1[:lead] = 1
    exp = np.full(lead + n, -1, np.int32)
    exp[lead:] = i
    if broken is not None:
        h1[lead + broken] = 1
        exp[lead + broken] = -1
        exp[lead + broken + 1 :] = i[broken:-1]
    n_o, exp_o = apply_rot_filter(exp, lambda p, v: p, lambda p, v: v, V1, V2)
    F12 = F12_ROWS
    return (V1, h1, FeatureVector.from_dict({5: list(range(lead + n))}), V2, FeatureVector.from_dict({5: list(range(n))}),
            F12, exp, exp_o)
