"""TEST INFRASTRUCTURE: build a pyramid on a poisoned workspace and read it back.

The pyramid workspace of a handle is allocated once per geometry and never cleared, so a builder
that misses a store leaves whatever the previous build (or the previous owner of the memory)
wrote, which in a test that runs two builders on the same frames is the right answer.  Every
pyramid comparison therefore goes through poisoned_build(): the whole workspace is set to a poison
byte (orb_debug_fill_pyramid) between the last build and the one under test, and a byte the
builder did not write still holds the poison when the levels are read.
"""
import ctypes

import numpy as np

import orbslam_jpminipc_amd as orb

POISON = 0xA5       # a correctly written 0xA5 cannot be told from an unwritten byte,
POISON_ALT = 0x5A   # so one case per builder runs with the complement as well

STREAM, PER_LEVEL, AUTO = 2, 1, 0  # orb_debug_set_pyramid_path modes


def level(ext, b, l):
    """Padded level l of frame b, (h + 32, w + 32), and the (h + 32, pitch - w - 32) row slack."""
    lib = orb.hip_lib()
    w, h = ctypes.c_int(), ctypes.c_int()
    assert lib.orb_debug_level_image(ext._h, b, l, None, ctypes.byref(w), ctypes.byref(h)) == 0
    g = np.empty((h.value + 32, w.value + 32), np.uint8)
    assert lib.orb_debug_level_image(ext._h, b, l, g.ctypes.data_as(ctypes.c_void_p), None, None) == 0
    n = lib.orb_debug_level_row_slack(ext._h, b, l, None)
    assert 0 <= n < 16
    s = np.empty((h.value + 32, n), np.uint8)
    if n:
        assert lib.orb_debug_level_row_slack(ext._h, b, l, s.ctypes.data_as(ctypes.c_void_p)) == n
    return g, s


def levels(ext, b):
    return [level(ext, b, l) for l in range(ext.nlevels)]


def fill(ext, value=POISON):
    assert orb.hip_lib().orb_debug_fill_pyramid(ext._h, value) == 0


def _geometry_is(ext, W, H):
    w, h = ctypes.c_int(), ctypes.c_int()
    if orb.hip_lib().orb_debug_level_image(ext._h, 0, 0, None, ctypes.byref(w), ctypes.byref(h)) != 0:
        return False  # no workspace yet
    return (w.value, h.value) == (W, H)


def poisoned_build(ext, d, mode, phases=1, frames=None, value=POISON):
    """Poison the workspace, run one builder (orb_debug_set_pyramid_path mode) on the device
    batch d with the given phase mask, and return (kps, desc, counts, {frame: levels()}).  The
    workspace exists only after the first extraction at a frame size: that one is run first
    (pyramid only), and poisoned over like any other."""
    import torch

    lib = orb.hip_lib()
    B, H, W = d.shape
    assert lib.orb_debug_set_pyramid_path(ext._h, mode) == 0
    if not _geometry_is(ext, W, H):
        ext.set_phases(1)
        ext.extract_batch_device(d)
    fill(ext, value)
    ext.set_phases(phases)
    try:
        kps, desc, counts = ext.extract_batch_device(d)
        torch.cuda.synchronize()
    finally:
        ext.set_phases(3)
        lib.orb_debug_set_pyramid_path(ext._h, AUTO)
    lv = {b: levels(ext, b) for b in (range(B) if frames is None else frames)}
    if phases & 2:
        return kps.cpu().numpy(), desc.cpu().numpy(), counts.cpu().numpy(), lv
    return None, None, None, lv


def plan(ext):
    """(has a stream plan, level-0 rows per round K0, rounds, LDS bytes) of the current geometry."""
    k0, nr, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    ok = orb.hip_lib().orb_debug_pyramid_plan(ext._h, ctypes.byref(k0), ctypes.byref(nr), ctypes.byref(lds))
    assert ok in (0, 1)
    return ok, k0.value, nr.value, lds.value


def plan_levels(ext):
    """[(nq, nWaves, ring rows)] per level of the stream plan, [] without one."""
    nq, nw, ring = (np.zeros(16, np.int32) for _ in range(3))
    p = [a.ctypes.data_as(ctypes.c_void_p) for a in (nq, nw, ring)]
    n = orb.hip_lib().orb_debug_pyramid_plan_levels(ext._h, *p, 16)
    assert 0 <= n <= 16
    return [(int(nq[l]), int(nw[l]), int(ring[l])) for l in range(n)]


def diff_message(got, ref, what, value=POISON):
    """None when the device level `got` = (image, slack) equals the reference image `ref` and its
    slack is zero; else `what` with the first differing (row, column), both values and whether the
    device byte is the poison."""
    g, s = got
    if g.shape != ref.shape:
        return f"{what}: device level is {g.shape[1] - 32}x{g.shape[0] - 32}, reference {ref.shape[1] - 32}x{ref.shape[0] - 32}"
    bad = np.argwhere(g != ref)
    if len(bad):
        r, c = (int(v) for v in bad[0])
        dev = int(g[r, c])
        return (f"{what}: {len(bad)} bytes differ, first at padded (row {r}, column {c}): device {dev:#04x}"
                f"{' (the poison byte: not written)' if dev == value else ''}, reference {int(ref[r, c]):#04x}")
    bad = np.argwhere(s != 0)
    if len(bad):
        r, c = (int(v) for v in bad[0])
        dev = int(s[r, c])
        return (f"{what}: {len(bad)} bytes of the row slack are not zero, first at padded (row {r}, column "
                f"{g.shape[1] + c}): device {dev:#04x}{' (the poison byte: not written)' if dev == value else ''}")
    return None


def assert_levels(lv, refs, what, value=POISON):
    """lv: {frame: levels()}, refs: {frame: [reference padded level images]}."""
    for b, per_level in lv.items():
        assert len(per_level) == len(refs[b]), f"{what} frame {b}: {len(per_level)} levels, reference {len(refs[b])}"
        for l, got in enumerate(per_level):
            msg = diff_message(got, refs[b][l], f"{what} frame {b} level {l}", value)
            assert msg is None, msg
