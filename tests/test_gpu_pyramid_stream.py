"""k_pyr_stream (the whole pyramid of a frame in one streaming pass) vs the per-level launches
(k_pyr0 + k_pyr_resize + k_pyr_resize_tail) and vs the oracle's ComputePyramid
(ORBextractor.cc:781-822): every padded level of every frame byte-identical, and identical
keypoints / descriptors, at the BASELINE sizes, odd sizes and unaligned input rows.  Every build
runs on a workspace poisoned just before it (tests/pyramid_build.py): the two paths share the
handle's pyramid buffer, and a store that one of them missed would otherwise still hold the
other's, correct, byte."""
import numpy as np
import pytest

import orbslam_jpminipc_amd as orb
import pyramid_build as pb
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu


def _run(ext, d, mode, frames=None):
    """A whole extraction on mode's pyramid path, the workspace poisoned first:
    (keypoints, descriptors, counts, {frame: [(padded level, row slack)]})."""
    return pb.poisoned_build(ext, d, mode, phases=3, frames=frames)


def _same(got, ref):
    """Image and row slack of a level equal in both runs, and the slack zero."""
    return np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and not got[1].any()


_plan = pb.plan


@pytest.mark.parametrize("W,H,nf,nl", [(640, 480, 1000, 8), (1241, 376, 2000, 8), (1280, 720, 2500, 8),
                                       (641, 479, 1000, 8), (320, 240, 1000, 8), (161, 121, 300, 4),
                                       (752, 480, 1000, 8)])
def test_stream_pyramid_equals_per_level(W, H, nf, nl):
    import torch

    B = 3
    frames = orb.synth_stream(W, H, stream=7, first=0, count=B)
    ext = orb.ORBextractor(nf, 1.2, nl, orb.FAST_SCORE, 20, device=0, max_batch=B)
    d = torch.from_numpy(frames).cuda()
    ref = _run(ext, d, 1)
    ok, k0, nr, lds = _plan(ext)
    assert ok == 1, "every BASELINE-like size has a stream plan"
    assert 1 <= k0 <= 32 and nr >= (H + k0 - 1) // k0 and 0 < lds <= 76 * 1024
    got = _run(ext, d, 2)
    for b in range(B):
        for l in range(nl):
            assert _same(got[3][b][l], ref[3][b][l]), \
                f"frame {b} level {l} differs at {np.argwhere(got[3][b][l][0] != ref[3][b][l][0])[:5]}"
    assert np.array_equal(got[2], ref[2])
    for b in range(B):
        n = ref[2][b]
        assert got[0][b, :n].tobytes() == ref[0][b, :n].tobytes()
        assert got[1][b, :n].tobytes() == ref[1][b, :n].tobytes()
    # and the oracle's pyramid (frame 0)
    ora = Oracle(nf, 1.2, nl, 1, 20)
    ko, do = ora.extract(frames[0])
    for l in range(nl):
        for name, run in (("stream", got), ("per-level", ref)):
            msg = pb.diff_message(run[3][0][l], ora.level_image(l), f"{name} path, frame 0 level {l} vs the oracle")
            assert msg is None, msg
    assert got[0][0, :len(ko)].tobytes() == ko.tobytes() and got[2][0] == len(ko)


@pytest.mark.parametrize("offset,extra", [(1, 3), (4, 12), (16, 16)])
def test_stream_pyramid_unaligned_rows(offset, extra):
    """Input rows at byte / dword / 16-byte alignment (k_pyr_stream's three load widths)."""
    import torch

    B, W, H = 2, 640, 480
    frames = orb.synth_stream(W, H, stream=9, first=0, count=B)
    stride = W + extra
    buf = torch.zeros(offset + B * H * stride + 64, dtype=torch.uint8)
    view = buf[offset:offset + B * H * stride].view(B, H, stride)
    view[:, :, :W] = torch.from_numpy(frames)
    d_buf = buf.cuda()
    d = d_buf[offset:offset + B * H * stride].view(B, H, stride)[:, :, :W]
    ext = orb.ORBextractor(1000, 1.2, 8, orb.FAST_SCORE, 20, device=0, max_batch=B)
    ref = _run(ext, d, 1)
    got = _run(ext, d, 2)
    for b in range(B):
        for l in range(8):
            assert _same(got[3][b][l], ref[3][b][l]), f"frame {b} level {l}"
        n = ref[2][b]
        assert got[2][b] == n and got[0][b, :n].tobytes() == ref[0][b, :n].tobytes()


def test_stream_pyramid_default_large_batch_sampled():
    """The automatic path at B = 256 (k_pyr_stream) against the per-level path on the same
    batch: all 256 frames' keypoints and descriptors, and the pyramid of a few frames."""
    import torch

    B, W, H = 256, 640, 480
    frames = orb.synth_stream(W, H, stream=4, first=100, count=B)
    ext = orb.ORBextractor(1000, 1.2, 8, orb.FAST_SCORE, 20, device=0, max_batch=B)
    d = torch.from_numpy(frames).cuda()
    k1, d1, c1, lv1 = _run(ext, d, pb.PER_LEVEL, frames=(0, 77, 255))
    assert _plan(ext)[0] == 1
    k0, d0, c0, lv0 = _run(ext, d, pb.AUTO, frames=(0, 77, 255))
    assert np.array_equal(c0, c1)
    for b in range(B):
        n = c1[b]
        assert k0[b, :n].tobytes() == k1[b, :n].tobytes(), f"frame {b}"
        assert d0[b, :n].tobytes() == d1[b, :n].tobytes(), f"frame {b}"
    for b, ref in lv1.items():
        for l in range(8):
            assert _same(lv0[b][l], ref[l]), f"frame {b} level {l}"


# whether the geometry has a stream plan, as orb_debug_pyramid_plan answered on an MI355X: a geometry
# that loses its plan fails here instead of skipping
OTHER_GEOMETRIES_PLAN = {(1920, 1080): True, (1024, 768): True, (800, 600): True}


@pytest.mark.parametrize("W,H,nf,sf,nl", [(1920, 1080, 3000, 1.2, 8), (1024, 768, 1500, 1.5, 5),
                                          (800, 600, 1200, 1.25, 7)])
def test_stream_pyramid_other_geometries(W, H, nf, sf, nl):
    """Wider frames (smaller rounds) and other scale factors (other tap tables): the stream
    plan, where the geometry has one, gives the per-level pyramid byte for byte; where it has
    none, the automatic path does.  Either way both equal the oracle's pyramid."""
    import torch

    B = 2
    frames = orb.synth_stream(W, H, stream=5, first=0, count=B)
    ext = orb.ORBextractor(nf, sf, nl, orb.FAST_SCORE, 20, device=0, max_batch=B)
    d = torch.from_numpy(frames).cuda()
    ref = _run(ext, d, pb.PER_LEVEL)
    ok, k0, nr, lds = _plan(ext)
    assert bool(ok) == OTHER_GEOMETRIES_PLAN[(W, H)], f"stream plan {ok} for {W}x{H} scale {sf} levels {nl}"
    got = _run(ext, d, pb.STREAM if ok else pb.AUTO)
    ora = Oracle(nf, sf, nl, 1, 20)
    for b in range(B):
        for l in range(nl):
            assert _same(got[3][b][l], ref[3][b][l]), f"frame {b} level {l}"
        n = ref[2][b]
        assert got[2][b] == n and got[0][b, :n].tobytes() == ref[0][b, :n].tobytes()
        assert got[1][b, :n].tobytes() == ref[1][b, :n].tobytes()
        ora.extract(frames[b])
        for l in range(nl):
            msg = pb.diff_message(got[3][b][l], ora.level_image(l), f"frame {b} level {l} vs the oracle")
            assert msg is None, msg
