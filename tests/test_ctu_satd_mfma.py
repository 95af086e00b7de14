"""The rough search of 8x8 and 16x16 CUs scores its angular modes 2..33 in groups of 32 (mode, block) pairs per wavefront, the Hadamard transforms and the magnitude
sums on the matrix cores (kvz_ctu.hpp angular_group_satd, kvz_mfma.hpp satd8_group_mfma; the routine alone: test_satd_mfma.py).  Nothing of that may show: every
output of the pass equals the oracle's on the device (-m gpu), on whole CTUs and on pictures whose border cuts the CTUs at a multiple of 8, without (QP 22) and
with (QP 37) the CABAC coefficient model; the instantiations that share rough_search -- sign data hiding, scaling lists, `medium` -- repeat one clip each against
their own references.  The host simulation keeps the scalar statement (angular_block_satd<false>) and must not have moved.  A test of the pictures themselves fails
when they stop exercising the code: every class of intra mode among the CUs decided at depth 2 and at depth 3, on the oracle's decisions alone."""
import pytest

import ctu_common as cc
import scaling_lists_common as slc
import signhide_common as sc
from test_ctu_cu8_transform import CONTENTS, LISTS_CLIPS, MEDIUM, SIGNHIDE_CLIPS, _device_pass, _frame, _oracle_model, _want
from test_ctu_recon_wide import CLASSES, _mode_class
from test_hostsim import hostsim  # noqa: F401  (fixture)

# whole CTUs, borders that cut a CTU at 8; 128x128 is there for the exercise check below: on the five smaller sizes alone the oracle decides no mode of negative
# displacement at depth 2
SIZES = [(64, 64), (72, 72), (8, 200), (200, 8), (136, 72), (128, 128)]
QPS = [22, 37]
GROUPS = [(w, h, qp) for (w, h) in SIZES for qp in QPS]
_gid = lambda g: f"{g[0]}x{g[1]}-qp{g[2]}"  # noqa: E731
SIGNHIDE_CLIP = [c for c in SIGNHIDE_CLIPS if c[0] == "ultrafast-200x136-qp27"]
LISTS_CLIP = [c for c in LISTS_CLIPS if c[0] == "ultrafast-200x136-qp27"]
MEDIUM_CASE = (72, 72, "small", 4321, 22)


def test_the_clips_exist():
    assert len(SIGNHIDE_CLIP) == 1 and len(LISTS_CLIP) == 1


@pytest.mark.parametrize("group", GROUPS, ids=_gid)
def test_hostsim_rough_search_equals_oracle(oracle, hostsim, group):  # noqa: F811
    w, h, qp = group
    m = _oracle_model(oracle, qp)
    assert bool(m.coeff_cabac) == (qp >= 28)
    frames, want = _want(oracle, w, h, qp)
    for (kind, key), f, a in zip(CONTENTS, frames, want):
        b = cc.run_hostsim(hostsim.lib, m, w, h, f)
        assert not cc.compare(a, b), (group, kind, key, cc.compare(a, b))


def test_pictures_exercise_the_rough_search(oracle):
    """what the oracle alone DECIDES on these pictures: all classes of modes among the CUs of depth 2 (16x16: four groups a search) and of depth 3 (8x8: one group)"""
    classes = {2: set(), 3: set()}
    for w, h, qp in GROUPS:
        for o in _want(oracle, w, h, qp)[1]:
            depth, mode = o["depth"].reshape(-1), o["mode"].reshape(-1)
            for d in (2, 3):
                classes[d] |= {_mode_class(int(m)) for m in mode[depth == d]}
    assert classes[2] == CLASSES, CLASSES - classes[2]
    assert classes[3] == CLASSES, CLASSES - classes[3]


# ---- the device
@pytest.fixture(scope="module")
def hiplib():
    import kvazaar_amd
    lib = kvazaar_amd.load_library()
    assert lib.kvz_hip_device_count() >= 1
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS, ids=_gid)
def test_hip_rough_search_equals_oracle(oracle, hiplib, group):
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


@pytest.mark.gpu
def test_hip_signhide_pass_keeps_the_reference_encoders_pictures(hiplib):
    clip = SIGNHIDE_CLIP[0]
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    outs = _device_pass(hiplib, sc.table(hiplib, [qp], **sc.switches(clip)).models[0], None, w, h, sc.clip_frames(clip))
    assert [sc.sha(o["rec"]) for o in outs] == sc.fixture()[name]["rec"]


@pytest.mark.gpu
def test_hip_scaling_list_pass_keeps_the_reference_encoders_pictures(hiplib):
    clip = LISTS_CLIP[0]
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    outs = _device_pass(hiplib, slc.table(hiplib, [qp], **slc.switches(clip)).models[0], [slc.lists("default")], w, h, slc.clip_frames(clip))
    assert [slc.sha(o["rec"]) for o in outs] == slc.fixture()[name]["rec"]


@pytest.mark.gpu
def test_hip_medium_equals_oracle(oracle, hiplib):
    """`medium` (32x32 search, RDOQ, NxN): its 8x8 and 16x16 CUs take the same rough search; its reference is the oracle's pass with the same switches"""
    w, h, kind, key, qp = MEDIUM_CASE
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
        assert not cc.compare(want, got), (MEDIUM_CASE, cc.compare(want, got))
    finally:
        b.close()
