"""The four pyramid builders (k_pyr_stream; k_pyr0 + k_pyr_resize<4>; k_pyr0 + k_pyr_resize<32>;
k_pyr_resize_tail) and k_pyr0_color against the oracle's ComputePyramid at the small geometries
of tests/pyramid_cases.py, which reach every geometry-dependent branch (tests/test_pyramid_cases.py
proves that on the CPU).  Every build runs on a poisoned workspace (tests/pyramid_build.py), only
the pyramid phase is run, and every padded level of the checked frames must equal the oracle's
byte for byte, with zeros in the row slack."""
import ctypes
import pathlib

import numpy as np
import pytest

import orbslam_jpminipc_amd as orb
import pyramid_build as pb
import pyramid_cases as pc
import test_extract_plan_host as plan_host
from oracle_lib import Oracle
from orbslam_jpminipc_amd import _native

pytestmark = pytest.mark.gpu

# builder: (orb_debug_set_pyramid_path mode, batch size, frames checked)
BUILDERS = {
    "stream": (pb.STREAM, 2, (0, 1)),                  # k_pyr_stream
    "short": (pb.PER_LEVEL, 2, (0, 1)),                # k_pyr0 + k_pyr_resize<4> (B < 8)
    "rows32": (pb.PER_LEVEL, 8, tuple(range(8))),      # k_pyr0 + k_pyr_resize<32> (8 <= B < 256)
    "tail": (pb.PER_LEVEL, 256, (0, 1, 127, 255)),     # ... + k_pyr_resize_tail (B >= 256)
    "auto": (pb.AUTO, 256, (0, 1, 127, 255)),          # k_pyr_stream with a plan, else as "tail"
}


def _extractor(case, B):
    return orb.ORBextractor(case.nf, case.sf, case.nl, orb.FAST_SCORE, 20, device=0, max_batch=B)


def _refs(case, f, checked):
    return {b: pc.oracle_levels(case, f[b]) for b in checked}


def _refused(case, ext, d):
    """A REFUSED case: the geometry is built by the first extraction, which must fail with
    ORB_ENOTSUP and the recorded reason."""
    ext.set_phases(1)
    with pytest.raises(orb.OrbError) as e:
        ext.extract_batch_device(d)
    assert e.value.code == _native.ORB_ENOTSUP and case.why in str(e.value), f"{case.name}: {e.value}"


def _check(case, builder, value=pb.POISON, phases=1):
    """One case through one builder; returns what poisoned_build() returned, and the extractor."""
    import torch

    mode, B, checked = BUILDERS[builder]
    f = pc.frames(case, B)
    d = torch.from_numpy(f.copy()).cuda()  # (the shared frames are read-only)
    ext = _extractor(case, B)
    if case.expect == pc.REFUSED:
        _refused(case, ext, d)
        return None, ext
    out = pb.poisoned_build(ext, d, mode, phases=phases, frames=checked, value=value)
    ok, k0, nr, lds = pb.plan(ext)
    assert ok == (case.expect == pc.PLAN), f"{case.name}: stream plan {ok}, expected '{case.expect}' ({case.why})"
    pb.assert_levels(out[3], _refs(case, f, checked), f"{case.name} builder {builder}", value)
    return out, ext


@pytest.mark.parametrize("builder", ["stream", "short", "rows32"])
@pytest.mark.parametrize("group", list(pc.GROUPS))
def test_small_batch_builders(group, builder):
    for case in pc.GROUPS[group]:
        _check(case, builder)


@pytest.mark.parametrize("part", ["width", "height", "levels"])
def test_fused_tail(part):
    """k_pyr_resize_tail (B = 256, per-level path): its rowsPerPass walk and LDS ping-pong over
    other level sizes than 640 x 480's, and nlevels == 2, where there is no tail to launch."""
    for case in pc.TAIL_CASES:
        if case in pc.GROUPS[part]:
            _check(case, "tail")


def test_automatic_path():
    """Mode 0 at B = 256: k_pyr_stream where the geometry has a plan, the per-level launches with
    the fused tail where it has none; exact either way."""
    cases = pc.auto_cases()
    assert {c.expect for c in cases} == {pc.PLAN, pc.NO_PLAN}
    for case in cases:
        _check(case, "auto")


def test_plans_match_the_table():
    """Which cases have a stream plan, with which K0, and which of their levels decode their
    columns once (hoisted) or per round: as recorded in the table, and covering the K0 ladder."""
    import torch

    k0s, hoisted, per_round = set(), [], []
    for case in pc.ALL_CASES:
        if case.expect == pc.REFUSED:
            continue
        ext = _extractor(case, 1)
        ext.set_phases(1)
        ext.extract_batch_device(torch.from_numpy(pc.frames(case, 1).copy()).cuda())
        ok, k0, nr, lds = pb.plan(ext)
        lv = pb.plan_levels(ext)
        assert ok == (case.expect == pc.PLAN), f"{case.name}: stream plan {ok}, expected '{case.expect}' ({case.why})"
        if not ok:
            assert lv == []
            continue
        assert k0 == case.k0, f"{case.name}: K0 {k0}, recorded {case.k0}"
        assert nr >= (case.H + k0 - 1) // k0 and 0 < lds <= 76 * 1024
        assert len(lv) == case.nl and sum(nw for _, nw, _ in lv) <= 14 and all(nw >= 1 for _, nw, _ in lv)
        if case.nl >= 13:
            assert sum(nw for _, nw, _ in lv) <= 14 and [nw for _, nw, _ in lv][1:] == [1] * (case.nl - 1)
        sizes = pc.level_sizes(case)
        for l, (nq, nw, ring) in enumerate(lv):
            pitch = (sizes[l][0] + 32 + 15) & ~15
            assert nq == (pitch // 16 if l == 0 else pitch // 4), f"{case.name} level {l}"
            assert (1 <= ring <= min(255, sizes[l][1])) if l + 1 < case.nl else ring == 0, f"{case.name} level {l}"
            if l >= 1:
                (hoisted if nq <= 64 * nw else per_round).append((case.name, l))
        k0s.add(k0)
    assert len(k0s) >= 5, sorted(k0s)
    assert hoisted and per_round, (len(hoisted), len(per_round))


@pytest.mark.parametrize("W,H,nf,nl", [(64, 57, 300, 4), (320, 240, 500, 8), (1000, 150, 400, 6)])
def test_handle_plan_agrees_with_the_host_planner(W, H, nf, nl):
    """The library's planner (built with the device compiler) and tests/native/extract_plan_host.cpp's
    (the host compiler) answer alike: what orb_debug_pyramid_plan, orb_debug_pyramid_plan_levels,
    orb_get_level_info and orb_get_max_keypoints report of a handle is the host planner's plan.
    1000 x 150 with six levels has levels that decode their columns per round."""
    import torch

    host = ctypes.CDLL(str(pathlib.Path(__file__).resolve().parents[1] / "build" / "libextract_plan_host.so"))
    q = plan_host.query(host, plan_host.plan_case(W, H, nf, 1.2, nl))
    ext = orb.ORBextractor(nf, 1.2, nl, orb.FAST_SCORE, 20, device=0, max_batch=1)
    ext.set_phases(1)
    ext.extract_batch_device(torch.from_numpy(np.random.default_rng(W).integers(0, 256, (1, H, W), dtype=np.uint8)).cuda())
    assert q["code"] == 0 and q["stream"] == 1
    assert pb.plan(ext) == (q["stream"], q["k0"], q["rounds"], q["lds"])
    assert pb.plan_levels(ext) == q["levels"] and len(q["levels"]) == nl
    assert ext.mnFeaturesPerLevel.tolist() == q["features_per_level"] and ext.max_keypoints == q["max_keypoints"]
    assert ext.mvScaleFactor.tobytes() == np.asarray(q["scale"], np.float32).tobytes()
    if (W, H) == (1000, 150):
        assert any(nq > 64 * nw for nq, nw, _ in q["levels"][1:])


def test_a_refused_size_leaves_the_earlier_one_intact():
    """96 x 57, then 5000 x 100 (refused: a level wider than 4095), then 96 x 57 again on the same
    handle: the refusal drops the workspace, the third call rebuilds it and gives the first call's bytes."""
    import torch

    case = pc.HEIGHT_SWEEP[0]
    assert (case.W, case.H, case.nf, case.sf, case.nl) == (96, 57, 300, 1.2, 4)
    ext = _extractor(case, 2)
    d = torch.from_numpy(pc.frames(case, 2).copy()).cuda()

    def run():
        kps, desc, counts = (t.cpu().numpy() for t in ext.extract_batch_device(d))
        return [(int(counts[b]), kps[b, :counts[b]].tobytes(), desc[b, :counts[b]].tobytes()) for b in range(2)]

    first = run()
    assert sum(n for n, _, _ in first) > 0
    with pytest.raises(orb.OrbError) as e:
        ext.extract_batch_device(torch.zeros((2, 100, 5000), dtype=torch.uint8, device="cuda"))
    assert e.value.code == _native.ORB_ENOTSUP and "level size out of the supported range" in str(e.value)
    assert pb.plan(ext)[0] == 0  # no geometry, so no plan either
    assert run() == first


def test_input_alignment_and_partial_units():
    """load_unit16 (k_pyr_stream) and k_pyr0's three load widths: frames at every width residue
    inside a buffer of random bytes, at byte, dword and 16-byte alignments of pointer and stride."""
    import torch

    aligns, seen = set(), {16: set(), 4: set(), 1: set()}
    B = 2
    for case in pc.ALIGN_WIDTHS:
        refs = _refs(case, pc.frames(case, B), range(B))
        ext = _extractor(case, B)
        for off, extra in pc.ALIGN_LAYOUTS:
            buf, stride = pc.embed(case, B, off, extra)
            d_buf = torch.from_numpy(buf).cuda()
            d = d_buf[off:off + B * case.H * stride].view(B, case.H, stride)[:, :, :case.W]
            a, s = pc.load_classes(d.data_ptr(), stride, case.H * stride, case.W, case.H, B)
            aligns.add(a)
            seen[a] |= s
            for builder in ("stream", "short"):
                lv = pb.poisoned_build(ext, d, BUILDERS[builder][0])[3]
                pb.assert_levels(lv, refs, f"{case.name} offset {off} stride W+{extra} (align {a}) builder {builder}")
            assert pb.plan(ext)[0] == 1
    assert aligns == {16, 4, 1}
    assert {need for a in (4, 1) for need, _ in seen[a]} == set(range(1, 17))
    for a in (4, 1):
        assert {over for _, over in seen[a]} == {False, True}, a


# one case per builder again with the complement as poison: a byte that is correctly 0xA5 cannot be
# told from an unwritten one
@pytest.mark.parametrize("builder,case", [("stream", pc.WIDTH_SWEEP[9]), ("short", pc.HEIGHT_SWEEP[1]),
                                          ("rows32", pc.WIDTH_SWEEP[30]), ("tail", pc.LEVEL_COUNTS[2]),
                                          ("auto", pc.LEVEL_COUNTS[2])], ids=lambda v: getattr(v, "name", v))
def test_complement_poison(builder, case):
    f = pc.frames(case, BUILDERS[builder][1])
    assert (f[0] == pb.POISON).any() and (f[0] == pb.POISON_ALT).any()
    _check(case, builder, value=pb.POISON_ALT)


@pytest.mark.parametrize("builder,case", [("stream", pc.WIDTH_SWEEP[37]), ("short", pc.HEIGHT_SWEEP[0]),
                                          ("rows32", pc.LEVEL_COUNTS[3]), ("tail", pc.HEIGHT_SWEEP[4]),
                                          ("auto", pc.LEVEL_COUNTS[5])], ids=lambda v: getattr(v, "name", v))
def test_consumers_read_the_same_buffer(builder, case):
    """A whole extraction on the poisoned workspace: keypoints and descriptors of the checked
    frames equal the oracle's, so FAST, the orientation and rBRIEF read the pyramid just checked."""
    (kps, desc, counts, _), _ = _check(case, builder, phases=3)
    f = pc.frames(case, BUILDERS[builder][1])
    ora = Oracle(case.nf, case.sf, case.nl, 1, 20)
    total = 0
    for b in BUILDERS[builder][2]:
        ko, do = ora.extract(f[b])
        n = int(counts[b])
        assert n == len(ko), f"{case.name} builder {builder} frame {b}: {n} keypoints, oracle {len(ko)}"
        assert kps[b, :n].tobytes() == ko.tobytes(), f"{case.name} builder {builder} frame {b}: keypoints differ"
        assert desc[b, :n].tobytes() == do.tobytes(), f"{case.name} builder {builder} frame {b}: descriptors differ"
        total += n
    assert total > 0, "the case must have keypoints for this check to mean anything"


@pytest.mark.parametrize("rgb,cn", [(True, 3), (False, 3), (True, 4)])
def test_colour_ingest(rgb, cn):
    """k_pyr0_color's grid ((pitch / 4 + 63) / 64 x (ph + 3) / 4) at W = 64 .. 79: level 0 against
    the oracle's colour conversion + border, then levels 1 .. 3 as the per-level builder leaves them."""
    import torch

    from test_color_ingest import rgb_to_gray

    B = 2
    for case in pc.ALIGN_WIDTHS:
        rng = np.random.default_rng(100 + case.W)
        col = rng.integers(0, 256, size=(B, case.H, case.W, cn), dtype=np.uint8)
        refs = {b: pc.oracle_levels(case, rgb_to_gray(col[b], rgb)) for b in range(B)}
        ext = _extractor(case, B)
        d = torch.from_numpy(col).cuda()
        ext.extract_batch_device_color(d, rgb=rgb)  # (the workspace exists after the first extraction)
        pb.fill(ext)
        ext.extract_batch_device_color(d, rgb=rgb)
        torch.cuda.synchronize()
        lv = {b: pb.levels(ext, b) for b in range(B)}
        pb.assert_levels(lv, refs, f"{case.name} colour rgb={rgb} cn={cn}")
