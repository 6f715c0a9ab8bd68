"""Tables and frames for the local-map tests: a seeded generator of consistent maps (kf_mp and pt_obs
agree), and the hand-made cases that random maps miss.  Every scene is (Tables, [frames]) or Tables."""
from __future__ import annotations

import numpy as np

from local_map_model import Tables


def consistent(kf_mp, n_pt, kf_bad=None, pt_bad=None, kf_cov=None) -> Tables:
    """Tables whose observations are exactly what kf_mp says: point p is observed by every keyframe
    that holds it."""
    n_kf = len(kf_mp)
    obs = [set() for _ in range(n_pt)]
    for k, row in enumerate(kf_mp):
        for p in row:
            if p >= 0:
                obs[p].add(k)
    return Tables(kf_bad if kf_bad is not None else [0] * n_kf, kf_mp, kf_cov if kf_cov is not None else [[]] * n_kf,
                  pt_bad if pt_bad is not None else [0] * n_pt, [sorted(s) for s in obs])


def random_map(seed, n_kf, n_pt, row_len, p_null=0.3, p_kf_bad=0.1, p_pt_bad=0.1, window=None) -> Tables:
    """Keyframe k holds row_len keypoints; a keypoint holds no point with p_null, else one of a window
    of points around k's share of the map (neighbouring keyframes overlap, far ones do not).  Covisibility
    rows: 0 .. 10 random keyframes, then -1, then anything (what follows the first -1 is not read)."""
    rng = np.random.default_rng(seed)
    window = window if window is not None else max(4, min(n_pt, 3 * row_len))
    kf_mp = []
    for k in range(n_kf):
        c = int(k * n_pt / max(n_kf, 1))
        pts = (c + rng.permutation(window)[:row_len]) % max(n_pt, 1) if n_pt else np.zeros(0, int)
        row = [int(p) if rng.random() >= p_null else -1 for p in pts]
        row += [-1] * (row_len - len(row))
        kf_mp.append(row)
    cov = []
    for k in range(n_kf):
        m = int(rng.integers(0, 11))
        row = [int(v) for v in rng.integers(0, n_kf, m)]
        if m < 10:
            row = row + [-1] + [int(v) for v in rng.integers(0, n_kf, 9 - m)]
        cov.append(row)
    return consistent(kf_mp, n_pt, (rng.random(n_kf) < p_kf_bad).astype(int), (rng.random(n_pt) < p_pt_bad).astype(int),
                      cov)


def random_frame(seed, T: Tables, n, around=None, p_null=0.3):
    """A frame of n slots whose points come from keyframe `around` and its index neighbours."""
    rng = np.random.default_rng(seed)
    if T.n_kf == 0 or T.n_pt == 0:
        return [-1] * n
    k = int(rng.integers(0, T.n_kf)) if around is None else around
    pool = [p for d in range(-2, 3) for p in T.kf_mp[(k + d) % T.n_kf] if p >= 0]
    if not pool:
        return [-1] * n
    return [int(pool[int(rng.integers(0, len(pool)))]) if rng.random() >= p_null else -1 for _ in range(n)]


def voted_chain(n_voted, n_kf=200, bad_voted=()):
    """Keyframes 0 .. n_voted - 1 get one vote each (point k is seen by keyframe k alone); every voted
    keyframe's first covisible is an unvoted keyframe of its own, so that each visit can append one."""
    kf_mp = [[k] if k < n_voted else [] for k in range(n_kf)]
    cov = [[(n_voted + k) % n_kf, 0] if k < n_voted else [] for k in range(n_kf)]
    kf_bad = [1 if k in bad_voted else 0 for k in range(n_kf)]
    T = consistent(kf_mp, n_voted, kf_bad=kf_bad, kf_cov=cov)
    return T, list(range(n_voted))


def packed_counter_extremes():
    """65536 keyframes; 65534 gets 8192 votes, 65535 gets 8191 and 65533 one: both halves of the last
    packed counter at their largest counts, next to a counter holding 1 in its high half."""
    n_kf, n = 65536, 8192
    kf_mp = [[] for _ in range(n_kf)]
    kf_mp[65534] = list(range(n))
    kf_mp[65535] = list(range(n - 1))
    kf_mp[65533] = [0]
    return consistent(kf_mp, n), list(range(n))


def shared_rows(n_rows, row_len, n_pt, seed=5):
    """n_rows keyframes of row_len keypoints drawn from only n_pt points (heavy sharing), all voted by a
    frame that holds one point of each."""
    rng = np.random.default_rng(seed)
    kf_mp = [[int(p) for p in rng.integers(0, n_pt, row_len)] for _ in range(n_rows)]
    T = consistent(kf_mp, n_pt, pt_bad=(rng.random(n_pt) < 0.05).astype(int))
    frame = [next((p for p in row if not T.pt_bad[p]), -1) for row in kf_mp]
    return T, frame


def last_is_first():
    """Point 7 occurs only as the last keypoint of the last local keyframe."""
    kf_mp = [[0, 1, 2], [2, 1, 0, 3], [3, 0, -1, 7]]
    return consistent(kf_mp, 8), [0, 3]


def neighbour_rows():
    """Voted keyframes 0 .. 4 whose covisibility rows are: empty; all bad; all already in the list; bad,
    present, then eligible; eligible only after a -1 (not read)."""
    n_kf = 12
    kf_mp = [[k] for k in range(5)] + [[] for _ in range(7)]
    cov = [[], [8, 9], [0, 1, 3], [8, 2, 10, 11], [-1, 11]] + [[] for _ in range(7)]
    kf_bad = [0] * n_kf
    kf_bad[8] = kf_bad[9] = 1
    return consistent(kf_mp, 5, kf_bad=kf_bad, kf_cov=cov), [0, 1, 2, 3, 4]


def connections_scene():
    """Keyframe 0 shares 14, 15 and 16 points with keyframes 1, 2, 3, 16 with keyframe 4 (equal weights),
    20 with the bad keyframe 5; keyframe 6 shares 3 with 7 and 3 with 8 (the fallback's tie); keyframe 9
    holds only bad and NULL points (the empty counter)."""
    n_kf = 10
    kf_mp = [[] for _ in range(n_kf)]
    nxt = [0]

    def share(a, b, n):
        for _ in range(n):
            kf_mp[a].append(nxt[0]), kf_mp[b].append(nxt[0])
            nxt[0] += 1

    share(0, 1, 14), share(0, 2, 15), share(0, 3, 16), share(0, 4, 16), share(0, 5, 20)
    share(6, 7, 3), share(6, 8, 3)
    bad_pt = nxt[0]
    share(9, 1, 1)
    kf_mp[9].append(-1)
    kf_bad = [0] * n_kf
    kf_bad[5] = 1
    pt_bad = [0] * nxt[0]
    pt_bad[bad_pt] = 1
    return consistent(kf_mp, nxt[0], kf_bad=kf_bad, pt_bad=pt_bad)
