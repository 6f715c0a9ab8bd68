"""gpu::LocalMap of include/orb_slam_gpu.hpp (tests/native/local_map_facade.cpp, built by
__graft_entry__.build()) on the GPU: UpdateReference and UpdateConnections over POD tables give what the
model gives (tests/local_map_model.py)."""
import pathlib
import subprocess

import numpy as np
import pytest

import local_map_model as lm
import local_map_scenes as sc

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _fnv(h, data: bytes):
    for b in data:
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h


def _h(values, dtype):
    return f"{_fnv(2166136261, np.asarray(values, dtype).tobytes()):08x}"


def test_cpp_facade(tmp_path):
    T = sc.random_map(4, 65, 300, 20)
    frame = sc.random_frame(5, T, 50)
    kfs = [0, 7, 64, 33]
    a = T.arrays()
    path = tmp_path / "map.bin"
    with open(path, "wb") as f:
        f.write(np.int32([T.n_kf, T.n_pt, len(a["kf_mp"]), len(a["pt_obs_kf"]), len(frame), len(kfs)]).tobytes())
        for k in ("kf_bad", "kf_mp_off", "kf_mp", "kf_cov", "pt_bad", "pt_obs_off", "pt_obs_kf"):
            f.write(a[k].tobytes())
        f.write(np.int32(frame).tobytes())
        f.write(np.int32(kfs).tobytes())
    r = subprocess.run([str(ROOT / "build" / "local_map_facade"), str(path)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "local map facade OK" in r.stdout, r.stdout
    w = lm.local_map_reference(T, frame)
    assert w["n_local_kf"] > 5 and w["n_local_pt"] > 50
    lines = r.stdout.splitlines()
    assert lines[0] == (f"REF ref={w['ref_kf']} votes={w['ref_votes']} voted={w['n_voted']} kfs={w['n_local_kf']} "
                        f"pts={w['n_local_pt']} cleared={w['n_cleared']}"), r.stdout
    assert lines[1] == (f"LISTS {_h(w['f_mp_out'], np.int32)} {_h(w['local_kf'], np.int32)} {_h(w['local_pt'], np.int32)} "
                        f"{_h(w['local_pt_seen'], np.uint8)}"), r.stdout
    for q, k in enumerate(kfs):
        c = lm.update_connections(T, k)
        h = 2166136261
        for name in ("conn_kf", "conn_w", "ord_kf", "ord_w"):
            h = _fnv(h, np.asarray(c[name], np.int32).tobytes())
        assert lines[2 + q] == (f"CONN {k} conn={len(c['conn_kf'])} ord={len(c['ord_kf'])} unchanged={c['unchanged']} "
                                f"{h:08x}"), r.stdout
