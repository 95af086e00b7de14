"""The 16x16 CU (kvz_ctu.hpp recon_cu16) is reconstructed per wavefront role: luma -- 32 row tasks of eight samples around the 16-point passes -- on the wavefront
playing threads 0..63, U and V -- one sample of each per lane, through the 8-point row passes of kvz_recon.hpp, the two intermediates of the inverse path stored
transposed -- on the other one, the stages synchronised per wavefront, every sum with one writer, and "the plane has levels" taken from the wavefront's own
reduction.  Nothing of that may show: every output of the pass equals the oracle's -- the host simulation here (it compiles the same text), the device under
-m gpu -- on whole CTUs and on pictures that put 16x16 CUs at an edge, from QP 4 (the largest levels) to QP 51 (the most planes without levels), with and without
the CABAC coefficient model (QP >= 28).  The instantiations that take the path with per-coefficient factors (scaling lists) or keep recon_tus (sign data hiding,
RDOQ: `medium`) repeat a subset.  A test of the pictures themselves fails when they stop exercising the code: every class of intra mode among the CUs decided at
depth 2 and all eight patterns of planes with levels -- chroma with levels under a luma plane without is what the gating per wavefront can get wrong."""
import ctypes as C

import numpy as np
import pytest

import ctu_common as cc
import scaling_lists_common as slc
import signhide_common as sc
from test_ctu_recon_wide import BORDER, CLASSES, COVER, _frame, _mode_class, _oracle_model
from test_hostsim import hostsim  # noqa: F401  (fixture)

EXTREMES = [(64, 64, kind, key, qp) for qp in (4, 51)
            for kind, key in [("small", 4321), ("large", 4321), ("adversarial", "flat"), ("adversarial", "noise"), ("adversarial", "ramp"), ("adversarial", "blocks")]]
CASES = COVER + BORDER + EXTREMES
_id = lambda c: f"{c[0]}x{c[1]}-{c[2]}-{c[3]}-qp{c[4]}"  # noqa: E731

_WANT = {}


def _want(oracle, case):
    """the oracle's pass on one picture, computed once and shared"""
    if case not in _WANT:
        w, h, _, _, qp = case
        _WANT[case] = cc.run_oracle(oracle, _oracle_model(oracle, qp), w, h, _frame(case))
    return _WANT[case]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_hostsim_cu16_equals_oracle(oracle, hostsim, case):  # noqa: F811
    w, h, _, _, qp = case
    m = _oracle_model(oracle, qp)
    assert bool(m.coeff_cabac) == (qp >= 28)
    a, b = _want(oracle, case), cc.run_hostsim(hostsim.lib, m, w, h, _frame(case))
    assert not cc.compare(a, b), (case, cc.compare(a, b))


# ---- do the pictures exercise the code?
def _zorder(x, y):
    z = 0
    for i in range(4):
        z |= ((x >> i) & 1) << (2 * i) | ((y >> i) & 1) << (2 * i + 1)
    return z


def _depth2_cus(o, w, h):
    """of one pass's outputs, per CU decided at depth 2: its mode class and which of its (Y, U, V) planes have levels"""
    depth, mode, coeff = o["depth"].reshape(h // 8, w // 8), o["mode"].reshape(h // 8, w // 8), o["coeff"].reshape(-1, 6144)
    wc = (w + 63) // 64
    for y8 in range(0, h // 8, 2):
        for x8 in range(0, w // 8, 2):
            if depth[y8, x8] != 2:
                continue
            ctu = coeff[(y8 // 8) * wc + x8 // 8]
            lx, ly = (x8 % 8) * 8, (y8 % 8) * 8
            y = bool(np.any(ctu[_zorder(lx // 4, ly // 4) * 16:][:256]))
            u, v = (bool(np.any(ctu[base + _zorder(lx // 8, ly // 8) * 16:][:64])) for base in (4096, 5120))
            yield _mode_class(int(mode[y8, x8])), (y, u, v)


def test_pictures_exercise_the_16x16_roles(oracle):
    """what the oracle alone DECIDES on the covering pictures: all seven classes of modes among the CUs of depth 2, and all eight patterns of planes with levels"""
    classes, patterns = set(), {}
    for case in COVER:
        for cls, p in _depth2_cus(_want(oracle, case), case[0], case[1]):
            classes.add(cls)
            patterns[p] = patterns.get(p, 0) + 1
    print(sorted(patterns.items()))
    assert classes == CLASSES, CLASSES - classes
    assert len(patterns) == 8, sorted(patterns.items())


def test_zorder_is_the_coefficient_blocks():
    assert slc._zorder(5, 10) == _zorder(5, 10) and slc._zorder(15, 15) == _zorder(15, 15) == 255


# ---- the other instantiations.  Sign data hiding and scaling lists have no oracle pass: their reference is the reference encoder's own output, committed as digests
# (tests/golden/signhide.json, scaling_lists.json).  Sign data hiding keeps recon_tus for its 16x16 CUs, the scaling-list kernels take recon_cu16 with a factor per
# coefficient; `medium` (RDOQ + NxN) keeps recon_tus.
SIGNHIDE_CLIPS = [c for c in sc.CLIPS if c[0] in ("ultrafast-72x88-qp12", "ultrafast-200x136-qp27", "ultrafast-noise-qp32")]  # the ones that decide CUs at depth 2
LISTS_CLIPS = [c for c in slc.CLIPS if c[0] in ("ultrafast-72x88-qp12", "ultrafast-200x136-qp27", "ultrafast-noise-qp37")]
MEDIUM = dict(search_32x32=1, coeff_cabac=1, rdoq=1, search_nxn=1)
MEDIUM_CASE = (128, 128, "small", 4321, 22)


@pytest.fixture(scope="module")
def hiplib_host():
    """libkvz_hip.so for its host-side functions only (the cost model of a QP): nothing here touches a device"""
    import kvazaar_amd
    return C.CDLL(kvazaar_amd.build_library())


def _depths(outs):
    return {int(v) for o in outs for v in np.unique(o["depth"])}


@pytest.mark.parametrize("clip", SIGNHIDE_CLIPS, ids=lambda c: c[0])
def test_hostsim_signhide_pass_keeps_the_reference_encoders_pictures(hiplib_host, clip):
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    outs = sc.sim_pass(sc.load_sim(), sc.table(hiplib_host, [qp] * n, **sc.switches(clip)), w, h, sc.clip_frames(clip))
    assert 2 in _depths(outs) and [sc.sha(o["rec"]) for o in outs] == sc.fixture()[name]["rec"]


@pytest.mark.parametrize("clip", LISTS_CLIPS, ids=lambda c: c[0])
def test_hostsim_scaling_list_pass_keeps_the_reference_encoders_pictures(hiplib_host, clip):
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    outs = slc.sim_pass(slc.load_sim(), slc.table(hiplib_host, [qp] * n, **slc.switches(clip)), [slc.lists("default")], None, w, h, slc.clip_frames(clip))
    assert 2 in _depths(outs) and [slc.sha(o["rec"]) for o in outs] == slc.fixture()[name]["rec"]


def test_hostsim_medium_equals_oracle(oracle, hostsim):  # noqa: F811
    w, h, kind, key, qp = MEDIUM_CASE
    m = _oracle_model(oracle, qp)
    for name, v in MEDIUM.items():
        setattr(m, name, v)
    f = _frame(MEDIUM_CASE)
    a, b = cc.run_oracle_nxn(oracle, m, w, h, f), cc.run_hostsim_nxn(hostsim.lib, m, w, h, f)
    assert 2 in _depths([a]) and not cc.compare(a, b), (MEDIUM_CASE, cc.compare(a, b))


# ---- the device
@pytest.fixture(scope="module")
def hiplib():
    import kvazaar_amd
    lib = kvazaar_amd.load_library()
    assert lib.kvz_hip_device_count() >= 1
    return lib


SIZES = [(64, 64), (128, 128), (24, 200), (200, 24), (136, 72)]  # whole CTUs; then 16x16 CUs at a picture edge
CONTENTS = [("small", 4321), ("large", 4321), ("adversarial", "flat"), ("adversarial", "noise"), ("adversarial", "ramp"), ("adversarial", "blocks")]
GROUPS = [(w, h, qp) for (w, h) in SIZES for qp in (4, 22, 37, 51)]


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS, ids=lambda g: f"{g[0]}x{g[1]}-qp{g[2]}")
def test_hip_cu16_equals_oracle(oracle, hiplib, group):
    """All pictures of one size and QP in one batch, run twice: the second run starts from the first one's border records, reconstruction and coefficient blocks."""
    w, h, qp = group
    model = cc.hip_cost_model(hiplib, qp, cc.coeff_weights(qp))
    assert bool(model.coeff_cabac) == (qp >= 28)
    cases = [(w, h, kind, key, qp) for kind, key in CONTENTS]
    frames = [_frame(c) for c in cases]
    want = [_want(oracle, c) for c in cases]
    b = cc.HipBatch(hiplib, w, h, len(frames))
    try:
        for i, f in enumerate(frames):
            b.upload(i, f)
        for run in range(2):
            b.run(model)
            for i in range(len(frames)):
                got = b.download(i)
                assert not cc.compare(want[i], got), (group, run, CONTENTS[i], cc.compare(want[i], got))
    finally:
        b.close()


def _device_pass(lib, model, sets, w, h, frames):
    b = cc.HipBatch(lib, w, h, len(frames))
    try:
        for i, f in enumerate(frames):
            b.upload(i, f)
        if sets:
            b.set_scaling_lists(sets, None)
        assert b.run(model) == 1
        return [b.download(i) for i in range(len(frames))]
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("clip", SIGNHIDE_CLIPS, ids=lambda c: c[0])
def test_hip_signhide_pass_keeps_the_reference_encoders_pictures(hiplib, clip):
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    outs = _device_pass(hiplib, sc.table(hiplib, [qp], **sc.switches(clip)).models[0], None, w, h, sc.clip_frames(clip))
    assert 2 in _depths(outs) and [sc.sha(o["rec"]) for o in outs] == sc.fixture()[name]["rec"]


@pytest.mark.gpu
@pytest.mark.parametrize("clip", LISTS_CLIPS, ids=lambda c: c[0])
def test_hip_scaling_list_pass_keeps_the_reference_encoders_pictures(hiplib, clip):
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    outs = _device_pass(hiplib, slc.table(hiplib, [qp], **slc.switches(clip)).models[0], [slc.lists("default")], w, h, slc.clip_frames(clip))
    assert 2 in _depths(outs) and [slc.sha(o["rec"]) for o in outs] == slc.fixture()[name]["rec"]


@pytest.mark.gpu
def test_hip_medium_equals_oracle(oracle, hiplib):
    w, h, kind, key, qp = MEDIUM_CASE
    model = cc.hip_cost_model(hiplib, qp, cc.coeff_weights(qp))
    for name, v in MEDIUM.items():
        setattr(model, name, v)
    f = _frame(MEDIUM_CASE)
    want = cc.run_oracle_nxn(oracle, model, w, h, f)
    b = cc.HipBatch(hiplib, w, h, 1)
    try:
        b.upload(0, f)
        b.run(model)
        got = b.download(0)
        got["part"], got["mode4"] = b.download_partitions(0)
        assert not cc.compare(want, got), (MEDIUM_CASE, cc.compare(want, got))
    finally:
        b.close()
