"""Tracking::UpdateReference with the "already matched" pass of SearchReferencePointsInFrustum, and
KeyFrame::UpdateConnections, restated in plain Python over the flat tables of DESIGN.md §23.

The reference's std::map<KeyFrame*, ...> is a dict iterated in sorted key order, its vectors are lists,
and the loops are written as the reference writes them (Tracking.cc:718-734, 778-801, 804-879;
KeyFrame.cc:332-411), so that the yardstick can be read against the source line by line.  Nothing here
knows how the device computes."""
from __future__ import annotations

import numpy as np


class Tables:
    """The map as the calls take it.  kf_mp: one list of point indices (-1: NULL) per keyframe; kf_cov:
    one list of up to 10 keyframe indices per keyframe (GetBestCovisibilityKeyFrames(10));
    pt_obs: one ascending list of keyframe indices per point (the keys of mObservations)."""

    def __init__(self, kf_bad, kf_mp, kf_cov, pt_bad, pt_obs):
        self.kf_bad = [int(b) for b in kf_bad]
        self.kf_mp = [[int(p) for p in row] for row in kf_mp]
        self.kf_cov = [[int(k) for k in row] for row in kf_cov]
        self.pt_bad = [int(b) for b in pt_bad]
        self.pt_obs = [[int(k) for k in row] for row in pt_obs]
        assert len(self.kf_bad) == len(self.kf_mp) == len(self.kf_cov)
        assert len(self.pt_bad) == len(self.pt_obs)

    @property
    def n_kf(self):
        return len(self.kf_bad)

    @property
    def n_pt(self):
        return len(self.pt_bad)

    def arrays(self):
        """The flat arrays of orb_local_map_tables_t."""
        kf_mp_off = np.zeros(self.n_kf + 1, np.int32)
        kf_mp_off[1:] = np.cumsum([len(r) for r in self.kf_mp])
        pt_obs_off = np.zeros(self.n_pt + 1, np.int32)
        pt_obs_off[1:] = np.cumsum([len(r) for r in self.pt_obs])
        cov = np.full((self.n_kf, 10), -1, np.int32)
        for k, row in enumerate(self.kf_cov):
            cov[k, :len(row)] = row
        flat = lambda rows: np.array([v for r in rows for v in r], np.int32)  # noqa: E731
        return dict(kf_bad=np.array(self.kf_bad, np.uint8), kf_mp_off=kf_mp_off, kf_mp=flat(self.kf_mp), kf_cov=cov,
                    pt_bad=np.array(self.pt_bad, np.uint8), pt_obs_off=pt_obs_off, pt_obs_kf=flat(self.pt_obs))


def cov_row(T: Tables, k: int):
    """GetBestCovisibilityKeyFrames(10) of keyframe k: the row up to its first -1."""
    row = []
    for c in T.kf_cov[k][:10]:
        if c == -1:
            break
        row.append(c)
    return row


def local_map_reference(T: Tables, f_mp):
    """One frame.  Returns a dict: f_mp_out, local_kf, local_pt, local_pt_seen, kf_votes (n_kf), n_voted,
    n_local_kf, ref_kf, ref_votes, n_local_pt, n_cleared."""
    frame = [int(p) for p in f_mp]  # mCurrentFrame.mvpMapPoints
    n_cleared = 0

    # UpdateReferenceKeyFrames, lines 807-824
    keyframeCounter = {}
    for i in range(len(frame)):
        if frame[i] != -1:
            pMP = frame[i]
            if not T.pt_bad[pMP]:
                observations = T.pt_obs[pMP]
                for kf in observations:
                    keyframeCounter[kf] = keyframeCounter.get(kf, 0) + 1
            else:
                frame[i] = -1
                n_cleared += 1

    # lines 826-848
    vmax = 0
    pKFmax = -1
    local_kf = []  # mvpLocalKeyFrames, reserve(3 * size): no reallocation below
    track_ref_kf = set()  # mnTrackReferenceForFrame == mCurrentFrame.mnId
    for pKF in sorted(keyframeCounter):
        if T.kf_bad[pKF]:
            continue
        if keyframeCounter[pKF] > vmax:
            vmax = keyframeCounter[pKF]
            pKFmax = pKF
        local_kf.append(pKF)
        track_ref_kf.add(pKF)
    n_voted = len(local_kf)

    # lines 852-876: itEndKF is taken once, before the loop, and stays valid because of the reserve
    itKF, itEndKF = 0, len(local_kf)
    while itKF != itEndKF:
        if len(local_kf) > 80:
            break
        pKF = local_kf[itKF]
        for pNeighKF in cov_row(T, pKF):
            if not T.kf_bad[pNeighKF]:
                if pNeighKF not in track_ref_kf:
                    local_kf.append(pNeighKF)
                    track_ref_kf.add(pNeighKF)
                    break
        itKF += 1

    # UpdateReferencePoints, lines 780-800
    local_pt = []
    track_ref_pt = set()
    for pKF in local_kf:
        for pMP in T.kf_mp[pKF]:
            if pMP == -1:
                continue
            if pMP in track_ref_pt:
                continue
            if not T.pt_bad[pMP]:
                local_pt.append(pMP)
                track_ref_pt.add(pMP)

    # SearchReferencePointsInFrustum, lines 718-734: after the clearing above no frame point is bad, so
    # every point the frame still holds gets mnLastFrameSeen = mnId; line 744 then skips those
    last_frame_seen = set()
    for i in range(len(frame)):
        pMP = frame[i]
        if pMP != -1:
            if T.pt_bad[pMP]:
                frame[i] = -1
            else:
                last_frame_seen.add(pMP)
    seen = [1 if pMP in last_frame_seen else 0 for pMP in local_pt]

    votes = [keyframeCounter.get(k, 0) for k in range(T.n_kf)]
    return dict(f_mp_out=frame, local_kf=local_kf, local_pt=local_pt, local_pt_seen=seen, kf_votes=votes,
                n_voted=n_voted, n_local_kf=len(local_kf), ref_kf=pKFmax, ref_votes=vmax, n_local_pt=len(local_pt),
                n_cleared=n_cleared)


def update_connections(T: Tables, k: int):
    """KeyFrame::UpdateConnections of keyframe k.  Returns a dict: conn_kf, conn_w, ord_kf, ord_w,
    unchanged."""
    # lines 334-363
    KFcounter = {}
    for pMP in T.kf_mp[k]:
        if pMP == -1:
            continue
        if T.pt_bad[pMP]:
            continue
        for kf in T.pt_obs[pMP]:
            if kf == k:
                continue
            KFcounter[kf] = KFcounter.get(kf, 0) + 1

    if not KFcounter:  # line 365
        return dict(conn_kf=[], conn_w=[], ord_kf=[], ord_w=[], unchanged=1)

    # lines 370-394
    nmax = 0
    pKFmax = -1
    th = 15
    vPairs = []
    for kf in sorted(KFcounter):
        if KFcounter[kf] > nmax:
            nmax = KFcounter[kf]
            pKFmax = kf
        if KFcounter[kf] >= th:
            vPairs.append((KFcounter[kf], kf))
    if not vPairs:
        vPairs.append((nmax, pKFmax))

    # lines 396-403: sort of pair<int, KeyFrame*> (weight, then pointer), then push_front
    vPairs.sort()
    lKFs, lWs = [], []
    for w, kf in vPairs:
        lKFs.insert(0, kf)
        lWs.insert(0, w)

    conn = sorted(KFcounter)
    return dict(conn_kf=conn, conn_w=[KFcounter[c] for c in conn], ord_kf=lKFs, ord_w=lWs, unchanged=0)
