"""The local map of a tracked frame and a keyframe's covisibility over the C ABI
(csrc/orb_localmapref.hip): Tracking::UpdateReference with the "already matched" pass of
SearchReferencePointsInFrustum, and KeyFrame::UpdateConnections, as counting over flat tables.  The map
and its mutation stay with the caller: results are indices, weights and flags.

std::map<KeyFrame*, ...>'s pointer order is ascending keyframe index here, so the caller's numbering
decides ties for the reference keyframe, who is inside the limit of 80, and the order of the local
points (which the projection matcher's greedy pass consumes)."""
from __future__ import annotations

import ctypes

import numpy as np

from ._native import ORB_ERANGE, ORB_OK, OrbError, check, hip_lib, ptr

MAX_KF = 65536
MAX_ROW = 8192
MAX_SCRATCH_BYTES = 256 << 20

INFO_DTYPE = np.dtype([(n, "<i4") for n in ("status", "n_voted", "n_local_kf", "ref_kf", "ref_votes", "n_local_pt",
                                            "n_cleared")])
CONN_INFO_DTYPE = np.dtype([(n, "<i4") for n in ("status", "n_conn", "n_ord", "unchanged")])
assert INFO_DTYPE.itemsize == 28 and CONN_INFO_DTYPE.itemsize == 16


def _a256(x: int) -> int:
    return (x + 255) & ~255


def frame_scratch_bytes(n_kf: int, n_pt: int, votes: bool = False) -> int:
    """What one frame of reference() counts against the scratch cap (csrc/orb_localmapref.hip,
    launch_local_map): the marks, three keyframe-sized lists (four with the vote table), the record and
    one 256-byte unit for the table status.  A cap below it is refused with -95."""
    return _a256(4 * n_pt) + (4 if votes else 3) * _a256(4 * n_kf) + _a256(28) + 256


def keyframe_scratch_bytes(n_kf: int) -> int:
    """The same for one keyframe of update_connections(): the sort keys, a power of two >= n_kf."""
    p = 1
    while p < n_kf:
        p <<= 1
    return _a256(4 * p) + 256


class _Tables(ctypes.Structure):
    """orb_local_map_tables_t"""

    _fields_ = [(n, ctypes.c_void_p) for n in ("kf_bad", "kf_mp_off", "kf_mp", "kf_cov", "pt_bad", "pt_obs_off",
                                                "pt_obs_kf")] + \
               [(n, ctypes.c_int32) for n in ("n_kf", "n_pt", "n_kf_mp", "n_obs")]


class MapTables:
    """The map as flat tables, on the host (numpy) or on a device (torch tensors, for the batch forms).

    kf_bad (n_kf,) u8; kf_mp_off (n_kf + 1,) / kf_mp int32: GetMapPointMatches() per keypoint, a point
    index or -1; kf_cov (n_kf, 10) int32: GetBestCovisibilityKeyFrames(10) in its order, the first -1
    ends a row; pt_bad (n_pt,) u8; pt_obs_off (n_pt + 1,) / pt_obs_kf int32: the keys of mObservations,
    each row strictly ascending.  The arrays are used as they are: the content is checked on the device."""

    NAMES = ("kf_bad", "kf_mp_off", "kf_mp", "kf_cov", "pt_bad", "pt_obs_off", "pt_obs_kf")

    def __init__(self, kf_bad, kf_mp_off, kf_mp, kf_cov, pt_bad, pt_obs_off, pt_obs_kf):
        given = dict(zip(self.NAMES, (kf_bad, kf_mp_off, kf_mp, kf_cov, pt_bad, pt_obs_off, pt_obs_kf)))
        self.on_device = not isinstance(kf_mp_off, np.ndarray) and hasattr(kf_mp_off, "data_ptr")
        self.a = {}
        for name, v in given.items():
            dt = np.uint8 if name.endswith("_bad") else np.int32
            if self.on_device:
                import torch

                want = torch.uint8 if dt is np.uint8 else torch.int32
                if v.dtype != want or not v.is_contiguous():
                    raise ValueError(f"{name} must be a contiguous {want} tensor")
                self.a[name] = v
            else:
                self.a[name] = np.ascontiguousarray(v, dt)
        self.n_kf = int(self.a["kf_bad"].shape[0])
        self.n_pt = int(self.a["pt_bad"].shape[0])
        if self.a["kf_mp_off"].shape[0] != self.n_kf + 1 or self.a["pt_obs_off"].shape[0] != self.n_pt + 1:
            raise ValueError("offset tables hold one entry per row and one more")
        if int(np.prod(tuple(self.a["kf_cov"].shape))) != self.n_kf * 10:
            raise ValueError("kf_cov holds 10 entries per keyframe")
        self.c = _Tables()
        for name in self.NAMES:
            setattr(self.c, name, ptr(self.a[name]).value)
        self.c.n_kf, self.c.n_pt = self.n_kf, self.n_pt
        self.c.n_kf_mp = int(np.prod(tuple(self.a["kf_mp"].shape)))
        self.c.n_obs = int(np.prod(tuple(self.a["pt_obs_kf"].shape)))

    def ref(self):
        return ctypes.byref(self.c)

    def to(self, device) -> "MapTables":
        """The same tables as tensors on `device`."""
        import torch

        return MapTables(*[torch.as_tensor(self.a[n]).to(device).contiguous() for n in self.NAMES])


def _ref(tables):
    return ctypes.cast(tables.ref(), ctypes.c_void_p)


class LocalMap:
    """The counting of Tracking::UpdateReference and KeyFrame::UpdateConnections on device `device`."""

    def __init__(self, device: int = 0):
        self._lib = hip_lib()
        self.device = int(device)

    def reference(self, tables: MapTables, f_mp, cap_kf=None, cap_pt=None, votes: bool = False, out=None) -> dict:
        """orb_local_map_reference for one frame: f_mp (n,) = mCurrentFrame.mvpMapPoints as point indices
        or -1.  Returns f_mp_out, local_kf, local_pt, local_pt_seen (trimmed to their counts), kf_votes
        (votes=True) and the record's fields.  cap_kf / cap_pt default to what always fits (n_kf, n_pt).
        A capacity too small raises OrbError(-34) whose `info` holds the counts needed.  out: a dict of
        preallocated arrays (f_mp_out, local_kf, local_pt, local_pt_seen) to write into."""
        mp = np.ascontiguousarray(np.asarray(f_mp, np.int32).reshape(-1))
        n = len(mp)
        cap_kf = tables.n_kf if cap_kf is None else int(cap_kf)
        cap_pt = tables.n_pt if cap_pt is None else int(cap_pt)
        o = dict(out or {})
        o.setdefault("f_mp_out", np.full(max(n, 1), -1, np.int32))
        o.setdefault("local_kf", np.full(max(cap_kf, 1), -1, np.int32))
        o.setdefault("local_pt", np.full(max(cap_pt, 1), -1, np.int32))
        o.setdefault("local_pt_seen", np.zeros(max(cap_pt, 1), np.uint8))
        kv = np.zeros(max(tables.n_kf, 1), np.int32) if votes else None
        info = np.zeros(1, INFO_DTYPE)
        r = self._lib.orb_local_map_reference(_ref(tables), n, ptr(mp), cap_kf, cap_pt, ptr(o["f_mp_out"]),
                                              ptr(o["local_kf"]), ptr(o["local_pt"]), ptr(o["local_pt_seen"]),
                                              ptr(kv), ptr(info), self.device)
        rec = {k: int(info[0][k]) for k in INFO_DTYPE.names}
        if r != ORB_OK:
            try:
                check(r)
            except OrbError as e:
                e.info = rec
                raise
        nk, npt = rec["n_local_kf"], rec["n_local_pt"]
        res = dict(f_mp_out=o["f_mp_out"][:n], local_kf=o["local_kf"][:nk], local_pt=o["local_pt"][:npt],
                   local_pt_seen=o["local_pt_seen"][:npt], **rec)
        if votes:
            res["kf_votes"] = kv[:tables.n_kf]
        return res

    def reference_batch_device(self, tables: MapTables, d_f_mp, d_counts, cap_kf: int, cap_pt: int, votes: bool = False,
                               out=None, stream=None) -> dict:
        """orb_local_map_reference_batch_device: d_f_mp (B, cap) int32 with d_counts[b] entries used, the
        tables on the same device.  Returns device tensors f_mp_out (B, cap), local_kf (B, cap_kf),
        local_pt (B, cap_pt), local_pt_seen (B, cap_pt), info (B, 7) int32 (INFO_DTYPE's fields) and
        kf_votes (B, n_kf) when asked for; a frame's status is in its record.  out: preallocated tensors
        by those names.  Asynchronous on `stream`."""
        import torch

        if not tables.on_device:
            raise ValueError("the batch form takes device-resident tables (MapTables.to)")
        B, cap = int(d_f_mp.shape[0]), int(d_f_mp.shape[1])
        dev = d_f_mp.device
        o = dict(out or {})
        shapes = dict(f_mp_out=((B, cap), torch.int32), local_kf=((B, cap_kf), torch.int32),
                      local_pt=((B, cap_pt), torch.int32), local_pt_seen=((B, cap_pt), torch.uint8),
                      info=((B, 7), torch.int32))
        if votes:
            shapes["kf_votes"] = ((B, tables.n_kf), torch.int32)
        for k, (shape, dt) in shapes.items():
            if k not in o:
                o[k] = torch.zeros(shape, dtype=dt, device=dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        check(self._lib.orb_local_map_reference_batch_device(
            _ref(tables), B, cap, ptr(d_f_mp), ptr(d_counts), int(cap_kf), int(cap_pt), ptr(o["f_mp_out"]),
            ptr(o["local_kf"]), ptr(o["local_pt"]), ptr(o["local_pt_seen"]), ptr(o.get("kf_votes")), ptr(o["info"]),
            ctypes.c_void_p(st.cuda_stream)))
        return o

    def update_connections(self, tables: MapTables, kf_idx, cap_conn=None, cap_ord=None) -> list:
        """orb_keyframe_update_connections for the keyframes kf_idx: a list of dicts conn_kf, conn_w
        (mConnectedKeyFrameWeights, ascending index), ord_kf, ord_w (mvpOrderedConnectedKeyFrames /
        mvOrderedWeights), unchanged, n_conn, n_ord, status.  A keyframe whose capacity is too small
        raises OrbError(-34) with `info` = the list of records."""
        idx = np.ascontiguousarray(np.asarray(kf_idx, np.int32).reshape(-1))
        K = len(idx)
        cap_conn = tables.n_kf if cap_conn is None else int(cap_conn)
        cap_ord = tables.n_kf if cap_ord is None else int(cap_ord)
        ck, cw = (np.full((max(K, 1), max(cap_conn, 1)), -1, np.int32) for _ in range(2))
        ok, ow = (np.full((max(K, 1), max(cap_ord, 1)), -1, np.int32) for _ in range(2))
        info = np.zeros(max(K, 1), CONN_INFO_DTYPE)
        r = self._lib.orb_keyframe_update_connections(_ref(tables), K, ptr(idx), cap_conn, cap_ord, ptr(ck), ptr(cw),
                                                      ptr(ok), ptr(ow), ptr(info), self.device)
        recs = [{k: int(info[q][k]) for k in CONN_INFO_DTYPE.names} for q in range(K)]
        if r != ORB_OK:
            try:
                check(r)
            except OrbError as e:
                e.info = recs
                raise
        res = []
        for q, rec in enumerate(recs):
            nc, no = rec["n_conn"], rec["n_ord"]
            res.append(dict(conn_kf=ck[q, :nc].copy(), conn_w=cw[q, :nc].copy(), ord_kf=ok[q, :no].copy(),
                            ord_w=ow[q, :no].copy(), **rec))
        return res

    def update_connections_batch_device(self, tables: MapTables, d_kf_idx, cap_conn: int, cap_ord: int, out=None,
                                        stream=None) -> dict:
        """orb_keyframe_update_connections_batch_device: device tensors conn_kf, conn_w (K, cap_conn),
        ord_kf, ord_w (K, cap_ord), info (K, 4) int32 (CONN_INFO_DTYPE's fields).  Asynchronous on `stream`."""
        import torch

        if not tables.on_device:
            raise ValueError("the batch form takes device-resident tables (MapTables.to)")
        K = int(d_kf_idx.shape[0])
        dev = d_kf_idx.device
        o = dict(out or {})
        shapes = dict(conn_kf=(K, cap_conn), conn_w=(K, cap_conn), ord_kf=(K, cap_ord), ord_w=(K, cap_ord), info=(K, 4))
        for k, shape in shapes.items():
            if k not in o:
                o[k] = torch.zeros(shape, dtype=torch.int32, device=dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        check(self._lib.orb_keyframe_update_connections_batch_device(
            _ref(tables), K, ptr(d_kf_idx), int(cap_conn), int(cap_ord), ptr(o["conn_kf"]), ptr(o["conn_w"]),
            ptr(o["ord_kf"]), ptr(o["ord_w"]), ptr(o["info"]), ctypes.c_void_p(st.cuda_stream)))
        return o

    def set_scratch_cap(self, nbytes: int = 0) -> None:
        """Test hook (orb_debug_set_local_map_scratch_cap): the byte cap of the per-chunk scratch; 0 restores
        MAX_SCRATCH_BYTES."""
        check(self._lib.orb_debug_set_local_map_scratch_cap(int(nbytes)))


__all__ = ["LocalMap", "MapTables", "INFO_DTYPE", "CONN_INFO_DTYPE", "MAX_KF", "MAX_ROW", "MAX_SCRATCH_BYTES", "ORB_ERANGE"]
