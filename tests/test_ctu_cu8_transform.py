"""The 8x8 CU (kvz_ctu.hpp recon_cu8) runs its four transform passes on contiguous rows: a lane reads its eight (chroma: four) inputs as one wide LDS load and
multiplies them with its row of the matrix as int16 pairs (kvz_recon.hpp fwd_row_point / inv_row_point), the two intermediates of the inverse path are stored
transposed, and what stage 1 knew of a sample travels to stage 5 in registers.  Nothing of that may show: every output of the pass equals the oracle's -- the host
simulation here (it compiles the same text: same layout, same index arithmetic), the device under -m gpu -- on whole CTUs and on pictures whose border cuts the
CTUs at a multiple of 8, from QP 4 (the largest levels) to QP 51, with and without the CABAC coefficient model (QP >= 28).  The instantiations with other readers
of the transform scratch -- sign data hiding, scaling lists, RDOQ + NxN (`medium`: its 8x8 CUs take recon_tus, not recon_cu8) -- repeat a subset.  A test of the
pictures themselves fails when they stop exercising the code: every class of intra mode among the CUs decided at depth 3, every pattern of planes with levels that
stages 4 and 5 tell apart."""
import ctypes as C

import numpy as np
import pytest

import ctu_common as cc
import scaling_lists_common as slc
import signhide_common as sc
from test_ctu_recon_wide import CLASSES, _mode_class
from test_hostsim import hostsim  # noqa: F401  (fixture)

SIZES = [(64, 64), (128, 128), (72, 72), (8, 200), (200, 8), (136, 72), (24, 200)]  # whole CTUs; then borders that cut a CTU at 8
CONTENTS = [("small", 4321), ("large", 4321), ("adversarial", "flat"), ("adversarial", "noise"), ("adversarial", "ramp"), ("adversarial", "blocks")]
QPS = [4, 22, 37, 51]
GROUPS = [(w, h, qp) for (w, h) in SIZES for qp in QPS]
_gid = lambda g: f"{g[0]}x{g[1]}-qp{g[2]}"  # noqa: E731


def _frame(w, h, kind, key):
    if kind == "adversarial":
        return cc.adversarial_frames(w, h)[key]
    return cc.yuv_frames(w, h, 1, key, kind)[0]


def _oracle_model(oracle, qp, **switches):
    """the oracle's model builder on the committed constants of the reference build (tests/golden/model_constants.json)"""
    k = cc.model_constants()
    m = cc.CostModel()
    f = oracle.lib.kvz_oracle_intra_cost_model
    f.restype = None
    f.argtypes = [C.c_int, C.c_float * 128, C.c_uint64, C.POINTER(cc.CostModel)]
    f(qp, (C.c_float * 128)(*k["entropy_fbits"]), cc.coeff_weights(qp), C.byref(m))
    for name, v in switches.items():
        setattr(m, name, v)
    return m


_WANT = {}


def _want(oracle, w, h, qp):
    """the oracle's pass on the six pictures of one size and QP, computed once and shared by the host and the device test"""
    if (w, h, qp) not in _WANT:
        m = _oracle_model(oracle, qp)
        frames = [_frame(w, h, kind, key) for kind, key in CONTENTS]
        _WANT[(w, h, qp)] = (frames, [cc.run_oracle(oracle, m, w, h, f) for f in frames])
    return _WANT[(w, h, qp)]


@pytest.mark.parametrize("group", GROUPS, ids=_gid)
def test_hostsim_cu8_equals_oracle(oracle, hostsim, group):  # noqa: F811
    w, h, qp = group
    m = _oracle_model(oracle, qp)
    assert bool(m.coeff_cabac) == (qp >= 28)
    frames, want = _want(oracle, w, h, qp)
    for (kind, key), f, a in zip(CONTENTS, frames, want):
        b = cc.run_hostsim(hostsim.lib, m, w, h, f)
        assert not cc.compare(a, b), (group, kind, key, cc.compare(a, b))


# ---- the other instantiations.  Sign data hiding and scaling lists have no oracle pass: their reference is the reference encoder's own output, committed as digests
# (tests/golden/signhide.json, scaling_lists.json); the clips taken here are the ones with 8x8 CUs, at small and large levels, with and without the CABAC model.
SIGNHIDE_CLIPS = [c for c in sc.CLIPS if c[0] in ("ultrafast-72x88-qp12", "ultrafast-200x136-qp27", "ultrafast-200x136-qp37")]
LISTS_CLIPS = [c for c in slc.CLIPS if c[0] in ("ultrafast-72x88-qp12", "ultrafast-200x136-qp27", "ultrafast-noise-qp37")]
MEDIUM = dict(search_32x32=1, coeff_cabac=1, rdoq=1, search_nxn=1)
MEDIUM_CASES = [(72, 72, "small", 4321, 22), (64, 64, "adversarial", "noise", 37), (72, 72, "large", 4321, 4)]


@pytest.fixture(scope="module")
def hiplib_host():
    """libkvz_hip.so for its host-side functions only (the cost model of a QP): nothing here touches a device"""
    import kvazaar_amd
    return C.CDLL(kvazaar_amd.build_library())


def _depths(outs):
    return sorted({int(v) for o in outs for v in np.unique(o["depth"])})


@pytest.mark.parametrize("clip", SIGNHIDE_CLIPS, ids=lambda c: c[0])
def test_hostsim_signhide_pass_keeps_the_reference_encoders_pictures(hiplib_host, clip):
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    outs = sc.sim_pass(sc.load_sim(), sc.table(hiplib_host, [qp] * n, **sc.switches(clip)), w, h, sc.clip_frames(clip))
    assert 3 in _depths(outs) and [sc.sha(o["rec"]) for o in outs] == sc.fixture()[name]["rec"]


@pytest.mark.parametrize("clip", LISTS_CLIPS, ids=lambda c: c[0])
def test_hostsim_scaling_list_pass_keeps_the_reference_encoders_pictures(hiplib_host, clip):
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    outs = slc.sim_pass(slc.load_sim(), slc.table(hiplib_host, [qp] * n, **slc.switches(clip)), [slc.lists("default")], None, w, h, slc.clip_frames(clip))
    assert 3 in _depths(outs) and [slc.sha(o["rec"]) for o in outs] == slc.fixture()[name]["rec"]


@pytest.mark.parametrize("case", MEDIUM_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}-{c[3]}-qp{c[4]}")
def test_hostsim_medium_equals_oracle(oracle, hostsim, case):  # noqa: F811
    w, h, kind, key, qp = case
    m = _oracle_model(oracle, qp, **MEDIUM)
    f = _frame(w, h, kind, key)
    a, b = cc.run_oracle_nxn(oracle, m, w, h, f), cc.run_hostsim_nxn(hostsim.lib, m, w, h, f)
    assert not cc.compare(a, b), (case, cc.compare(a, b))


# ---- do the pictures exercise the code?
def _patterns_and_classes(o, w, h):
    """of one pass's outputs: the mode classes of the CUs decided at depth 3 and, per such CU, which of its planes have levels"""
    depth, mode, coeff = o["depth"].reshape(h // 8, w // 8), o["mode"].reshape(h // 8, w // 8), o["coeff"].reshape(-1, 6144)
    wc = (w + 63) // 64
    classes, patterns = set(), set()
    for y8 in range(h // 8):
        for x8 in range(w // 8):
            if depth[y8, x8] != 3:
                continue
            classes.add(_mode_class(int(mode[y8, x8])))
            ctu = coeff[(y8 // 8) * wc + x8 // 8]
            lx, ly = (x8 % 8) * 8, (y8 % 8) * 8
            y = bool(np.any(ctu[slc._zorder(lx // 4, ly // 4) * 16:][:64]))
            u, v = (bool(np.any(ctu[base + slc._zorder(lx // 8, ly // 8) * 16:][:16])) for base in (4096, 5120))
            patterns.add("none" if not (y or u or v) else "luma" if y and not (u or v) else "chroma" if not y else "luma+one" if u != v else "all")
    return classes, patterns


def test_pictures_exercise_the_8x8_stages(oracle):
    """what the oracle alone DECIDES on these pictures: all seven classes of modes among the CUs of depth 3, and every pattern of planes with levels that stages 4
    and 5 of recon_cu8 tell apart (luma is one wavefront's condition, U and V are per-lane conditions of the other)"""
    classes, patterns = set(), set()
    for w, h, qp in GROUPS:
        for o in _want(oracle, w, h, qp)[1]:
            c, p = _patterns_and_classes(o, w, h)
            classes |= c
            patterns |= p
    assert classes == CLASSES, CLASSES - classes
    assert patterns == {"none", "luma", "chroma", "luma+one", "all"}, patterns


def test_border_pictures_cut_ctus_at_8():
    assert all(w % 8 == 0 and h % 8 == 0 for w, h in SIZES) and sum(1 for w, h in SIZES if w % 64 or h % 64) == 5


# ---- the device
@pytest.fixture(scope="module")
def hiplib():
    import kvazaar_amd
    lib = kvazaar_amd.load_library()
    assert lib.kvz_hip_device_count() >= 1
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS, ids=_gid)
def test_hip_cu8_equals_oracle(oracle, hiplib, group):
    """The six pictures of one size and QP in one batch, run twice: the second run starts from the first one's border records, reconstruction and coefficient blocks."""
    w, h, qp = group
    model = cc.hip_cost_model(hiplib, qp, cc.coeff_weights(qp))
    assert bool(model.coeff_cabac) == (qp >= 28)
    frames, want = _want(oracle, w, h, qp)
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
    assert [sc.sha(o["rec"]) for o in outs] == sc.fixture()[name]["rec"]


@pytest.mark.gpu
@pytest.mark.parametrize("clip", LISTS_CLIPS, ids=lambda c: c[0])
def test_hip_scaling_list_pass_keeps_the_reference_encoders_pictures(hiplib, clip):
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    outs = _device_pass(hiplib, slc.table(hiplib, [qp], **slc.switches(clip)).models[0], [slc.lists("default")], w, h, slc.clip_frames(clip))
    assert [slc.sha(o["rec"]) for o in outs] == slc.fixture()[name]["rec"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", MEDIUM_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}-{c[3]}-qp{c[4]}")
def test_hip_medium_equals_oracle(oracle, hiplib, case):
    w, h, kind, key, qp = case
    model = cc.hip_cost_model(hiplib, qp, cc.coeff_weights(qp))
    for name, v in MEDIUM.items():
        setattr(model, name, v)
    f = _frame(w, h, kind, key)
    want = cc.run_oracle_nxn(oracle, model, w, h, f)
    b = cc.HipBatch(hiplib, w, h, 1)
    try:
        b.upload(0, f)
        b.run(model)
        got = b.download(0)
        got["part"], got["mode4"] = b.download_partitions(0)
        assert not cc.compare(want, got), (case, cc.compare(want, got))
    finally:
        b.close()
