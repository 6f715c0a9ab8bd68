"""The extraction kernels on the constructed frames of tests/extractor_edge_frames.py, bit for bit
against the oracle: 28-byte keypoint records and descriptors, no tolerance anywhere.

tests/test_extractor_edge_frames_oracle.py pins the oracle on these frames to what is known by
construction (threshold and re-run table, NMS pairs inside and across cells, IC_Angle's zero and
equal moments, blur sums that are exact halves, one tie class larger than every quota); here the
product is pinned to the oracle through the host call (both score types), the device batches at the
sizes where the launch plan changes, k_fast's plane-scan fallback and the blur image.  A failure
names the frame, the first differing keypoint and the mark it belongs to.
"""
import ctypes

import numpy as np
import pytest

import extractor_edge_frames as E
import orbslam_jpminipc_amd as orb
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

NAMES = list(E.ALL_BUILDERS)
# the extractor settings under which the device batches run, each with the frames built for it first
GROUPS = [(2000, 20), (500, 20), (500, 12), (500, 7), (300, 20)]
_oracle_cache = {}


def _oracle(name, nf, th, score):
    """The oracle's (keypoints, descriptors) of a frame under the given settings, computed once."""
    key = (name, nf, th, score)
    if key not in _oracle_cache:
        ora = Oracle(nf, E.SCALE, E.NLEVELS, 1 if score == orb.FAST_SCORE else 0, th)
        _oracle_cache[key] = ora.extract(E.frame(name).img)
    return _oracle_cache[key]


def _kp_text(f, kp):
    s = float(E.SCALE) ** int(kp["octave"])
    return f"{kp} [{f.describe(kp['x'] / s, kp['y'] / s)}]"


def _compare(f, what, kg, dg, ko, do):
    """Fail with the frame, the first differing keypoint and its mark's class."""
    head = f"{f.name} ({what})"
    m = min(len(kg), len(ko))
    raw = [np.ascontiguousarray(k[:m]).view(np.uint8).reshape(m, 28) for k in (kg, ko)]
    rec = (raw[0] != raw[1]).any(axis=1)
    if rec.any():
        i = int(np.nonzero(rec)[0][0])
        pytest.fail(f"{head}: keypoint {i} of {len(kg)} (oracle {len(ko)}) differs\n  gpu    {_kp_text(f, kg[i])}\n"
                    f"  oracle {_kp_text(f, ko[i])}")
    if len(kg) != len(ko):
        longer, who = (kg, "gpu") if len(kg) > len(ko) else (ko, "oracle")
        pytest.fail(f"{head}: gpu {len(kg)} keypoints, oracle {len(ko)}; first extra one ({who}) {_kp_text(f, longer[m])}")
    if m == 0:
        assert dg is None or len(dg) == 0
        return
    rows = np.nonzero((np.asarray(dg) != do).any(axis=1))[0]
    if len(rows):
        i = int(rows[0])
        bits = np.nonzero(np.unpackbits(dg[i] ^ do[i], bitorder="little"))[0]
        pytest.fail(f"{head}: descriptors differ in {len(rows)} rows, first row {i} bits {bits[:8].tolist()}: "
                    f"{_kp_text(f, ko[i])}{_tie_hits(f, ko[i], bits)}")


def _tie_hits(f, kp, bits):
    """For a level-0 keypoint of the blur-tie frame: which samples of the differing bits lie on a
    blur sum that the two rounding rules round differently, and in which kind of column."""
    if f.name != "blur_ties" or kp["octave"] != 0:
        return ""
    from oracle_lib import lib

    ora = Oracle(f.nf, E.SCALE, E.NLEVELS, 1, f.th)
    ora.extract(f.img)
    padded = ora.level_image(0)
    T = E.blur_sums(padded)
    _, _, ties = E.discriminating_ties(T)
    rad = float(np.float32(kp["angle"]) * np.float32(np.pi / float(np.float32(180.0))))
    a, b = lib().oracle_cosf(rad), lib().oracle_sinf(rad)
    _, X, Y = E.descriptors_level0(E.blur_plane(T), padded, [[int(kp["x"]), int(kp["y"])]], [a], [b], E.pattern31())
    out = []
    for bit in bits[:8]:
        for s in (2 * bit, 2 * bit + 1):
            x, y = int(X[0, s]), int(Y[0, s])
            if 0 <= x < E.W and 0 <= y < E.H and ties[y, x]:
                kind = "a scalar-tail" if x >= (E.W // 4) * 4 else "an SSE2"
                out.append(f"bit {bit} samples the tie at ({x}, {y}), {kind} column")
    return "; " + ("; ".join(out) if out else "no differing bit samples a tie")


@pytest.mark.parametrize("score", [orb.FAST_SCORE, orb.HARRIS_SCORE], ids=["fast", "harris"])
@pytest.mark.parametrize("name", NAMES)
def test_host_call_parity(name, score):
    f = E.frame(name)
    ext = orb.ORBextractor(f.nf, E.SCALE, E.NLEVELS, score, f.th, device=0)
    kg, dg = ext(f.img)
    ko, do = _oracle(name, f.nf, f.th, score)
    _compare(f, f"host call, {'FAST_SCORE' if score == orb.FAST_SCORE else 'HARRIS_SCORE'}", kg, dg, ko, do)
    if score == orb.FAST_SCORE and f.expected is not None:  # the guard of the oracle test, on the product
        k0 = kg[kg["octave"] == 0]
        assert {(int(x), int(y)) for x, y in zip(k0["x"], k0["y"])} == set(f.expected)


@pytest.mark.parametrize("B", [8, 64, 256])
@pytest.mark.parametrize("nf,th", GROUPS)
def test_device_batch_parity(nf, th, B):
    """All frames in one device batch, repeated to fill it.  8, 64 and 256 frames: at and above
    KR_SHORT_BATCH, below and above k_rerun's workgroup-count switch, and KR_STREAM_BATCH, where k_pyr_stream builds the pyramid."""
    import torch

    own = [n for n in NAMES if (E.frame(n).nf, E.frame(n).th) == (nf, th)]
    order = own + [n for n in NAMES if n not in own]
    names = [order[i % len(order)] for i in range(B)]
    imgs = np.stack([E.frame(n).img for n in names])
    ext = orb.ORBextractor(nf, E.SCALE, E.NLEVELS, orb.FAST_SCORE, th, device=0, max_batch=B)
    kps, desc, counts = ext.extract_batch_device(torch.from_numpy(imgs).cuda())
    torch.cuda.synchronize()
    kps, desc, counts = kps.cpu().numpy(), desc.cpu().numpy(), counts.cpu().numpy()
    if B >= 256:
        assert orb.hip_lib().orb_debug_pyramid_plan(ext._h, None, None, None) == 1, "no k_pyr_stream plan"
    for b, n in enumerate(names):
        ko, do = _oracle(n, nf, th, orb.FAST_SCORE)
        c = int(counts[b])
        assert 0 <= c <= ext.max_keypoints
        _compare(E.frame(n), f"frame {b} of a device batch of {B}, nf {nf} th {th}",
                 orb.keypoints_from_bytes(kps[b], c), desc[b, :c], ko, do)


@pytest.mark.parametrize("name", ["nms_pairs_h", "nms_pairs_v", "nms_pairs_d", "mass_ties"])
def test_corner_list_fallback_parity(name):
    """k_fast's plane-scan fallback has an NMS of its own: a corner list of 8 entries sends the pair
    sweeps and the lattice through it."""
    f = E.frame(name)
    ext = orb.ORBextractor(f.nf, E.SCALE, E.NLEVELS, orb.FAST_SCORE, f.th, device=0)
    assert orb.hip_lib().orb_debug_set_fast_corner_list(ext._h, 8) == 0
    kg, dg = ext(f.img)
    ko, do = _oracle(name, f.nf, f.th, orb.FAST_SCORE)
    _compare(f, "host call, corner list of 8", kg, dg, ko, do)


def test_blur_image_ties():
    """Level 0's descriptor image of the blur-tie frame equals the oracle's blurred level, the three
    scalar-tail columns included, and holds the ties: 128 in the SSE2 columns, 129 in the tail."""
    f = E.frame("blur_ties")
    ext = orb.ORBextractor(f.nf, E.SCALE, E.NLEVELS, orb.FAST_SCORE, f.th, device=0)
    ora = Oracle(f.nf, E.SCALE, E.NLEVELS, 1, f.th)
    ext(f.img)
    ora.extract(f.img)
    bl = np.empty((E.H + 32, E.W + 32), np.uint8)
    assert orb.hip_lib().orb_debug_blur_image(ext._h, 0, 0, bl.ctypes.data_as(ctypes.c_void_p)) == 0
    ob = np.empty((E.H, E.W), np.uint8)
    assert ora.L.oracle_level_blurred(ora.h, 0, ob.ctypes.data_as(ctypes.c_void_p)) == 0
    got = bl[16:16 + E.H, 16:16 + E.W]
    T = E.blur_sums(ora.level_image(0))
    _, _, ties = E.discriminating_ties(T)
    xs = (E.W // 4) * 4
    if not np.array_equal(got, ob):
        y, x = np.argwhere(got != ob)[0]
        pytest.fail(f"blur_ties: blur image differs at {len(np.argwhere(got != ob))} pixels, first (x {x}, y {y}) in a "
                    f"{'scalar-tail' if x >= xs else 'SSE2'} column: gpu {got[y, x]} oracle {ob[y, x]}, T = {T[y, x]} "
                    f"({'a tie' if ties[y, x] else 'no tie'})")
    half = (T >> 16).astype(np.uint8)
    assert (got[:, :xs][ties[:, :xs]] == half[:, :xs][ties[:, :xs]]).all()          # half to even
    assert (got[:, xs:][ties[:, xs:]] == half[:, xs:][ties[:, xs:]] + 1).all()      # half up
    assert (half[:, xs:][ties[:, xs:]] == 128).all() and ties[:, xs:].sum() >= 100
