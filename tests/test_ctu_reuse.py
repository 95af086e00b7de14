"""A CU's cost on a prepared table (kvz_ctu.hpp cu_cost_prepare / cu_cost_batched): the half of the cost that does not depend on the CU's selection or reconstruction
-- which syntax contexts are used, their states, the price and successor of both values of every data-dependent bin, the most probable modes of the mock encode -- is
worked out beside the selection by twelve lanes of the wavefront that idles there and left in storage that is dead until the 64x64 attempt; thread 0 reads the table with
the CU's flags and sums in one round trip, chooses, and writes the states back.  Nothing of that may show: every output of the pass, CTU costs included, equals the
oracle's -- the host simulation here (it compiles the same text), the device under -m gpu -- with adaptive and frozen contexts (no successor state is written then), in
the instantiations that search 32x32 CUs (`fast`: its table must survive the 32x32 CU's reconstruction) and 4x4 PUs (`medium`), on whole CTUs and on pictures that cut
CUs at an edge, from QP 4 to QP 51.  A test of the pictures themselves fails when the oracle's decisions on them stop exercising the cases: 8x8 CUs in the first
position of a 16x16 with every kind of neighbour, under a 16x16 CU the picture edge cuts (never evaluated), decided modes on and off the most probable ones, the
patterns of planes with levels.  (The file's name is that of the issue, which also tried two reuses of a 16x16 parent's staging by its 8x8 children:
profiles/experiments/README.md.)"""
import numpy as np
import pytest

import ctu_common as cc
import scaling_lists_common as slc
import signhide_common as sc
import test_ctu_chains as chains
import test_ctu_cu16_roles as roles
from test_ctu_recon_wide import _frame, _oracle_model
from test_hostsim import hostsim  # noqa: F401  (fixture)

_id = roles._id
CONTENTS = roles.CONTENTS
FROZEN = dict(adaptive=0)
FAST = dict(search_32x32=1, coeff_cabac=1)
MEDIUM = roles.MEDIUM
SWITCH_CASE = (128, 128, "adversarial", "blocks", 22)  # the picture on which every instantiation decides most CUs at depth 3


def _with(model, switches):
    for name, v in switches.items():
        setattr(model, name, v)
    return model


# ---- the host simulation
@pytest.mark.parametrize("case", chains.CASES + roles.EXTREMES, ids=_id)
def test_hostsim_reuse_equals_oracle(oracle, hostsim, case):  # noqa: F811
    w, h, _, _, qp = case
    m = _oracle_model(oracle, qp)
    assert bool(m.coeff_cabac) == (qp >= 28)
    a = chains._oracle_run(oracle, case) if case in chains.CASES else roles._want(oracle, case)
    b = cc.run_hostsim(hostsim.lib, m, w, h, _frame(case))
    assert not cc.compare(a, b), (case, cc.compare(a, b))


@pytest.mark.parametrize("switches", [FROZEN, FAST], ids=["frozen", "fast"])
def test_hostsim_reuse_other_instantiations_equal_oracle(oracle, hostsim, switches):  # noqa: F811
    """frozen contexts (no successor state is ever written), and `fast`: a 32x32 CU's reconstruction runs through the whole transform scratch between the
    preparation and the cost"""
    w, h, _, _, qp = SWITCH_CASE
    m = _with(_oracle_model(oracle, qp), switches)
    f = _frame(SWITCH_CASE)
    a, b = cc.run_oracle(oracle, m, w, h, f), cc.run_hostsim(hostsim.lib, m, w, h, f)
    assert 3 in roles._depths([a]) and not cc.compare(a, b), (switches, cc.compare(a, b))


def test_hostsim_reuse_medium_equals_oracle(oracle, hostsim):  # noqa: F811
    """`medium`: neighbours are 4x4-granular, and the NxN attempt of an 8x8 CU prices on hooks of its own right behind the CU's cost"""
    w, h, _, _, qp = SWITCH_CASE
    m = _with(_oracle_model(oracle, qp), MEDIUM)
    f = _frame(SWITCH_CASE)
    a, b = cc.run_oracle_nxn(oracle, m, w, h, f), cc.run_hostsim_nxn(hostsim.lib, m, w, h, f)
    assert 3 in roles._depths([a]) and not cc.compare(a, b), cc.compare(a, b)


# ---- do the pictures exercise the code?
def _planes_with_levels(ctu, lx, ly, n):
    """which of the (Y, U, V) planes of the CU of n x n luma samples at CTU-local (lx, ly) have levels, in a CTU's coefficient block"""
    y = bool(np.any(ctu[roles._zorder(lx // 4, ly // 4) * 16:][:n * n]))
    u, v = (bool(np.any(ctu[base + roles._zorder(lx // 8, ly // 8) * 16:][:n * n // 4])) for base in (4096, 5120))
    return y, u, v


def test_pictures_exercise_the_reuse(oracle):
    """what the oracle alone DECIDES on the pictures of test_ctu_chains.CASES.  A children's loop that breaks early leaves no trace in the outputs: a decided
    depth-3 CU says that all four children were evaluated: these counts are minimums of what is evaluated."""
    places = {22: set(), 37: set()}   # (left, above) of the first children of 16x16 CUs inside the picture
    first_children = under_cut_parent = 0
    mpm = {(qp, d): set() for qp in (22, 37) for d in (2, 3)}
    patterns = {(qp, d): set() for qp in (22, 37) for d in (2, 3)}
    for case in chains.CASES:
        w, h, qp = case[0], case[1], case[4]
        o = chains._oracle_run(oracle, case)
        depth, mode, coeff = o["depth"].reshape(h // 8, w // 8), o["mode"].reshape(h // 8, w // 8), o["coeff"].reshape(-1, 6144)
        wc = (w + 63) // 64
        for d in (2, 3):
            n = 8 >> d  # the CU's width in 8x8 cells
            for cy in range(0, h // 8, n):
                for cx in range(0, w // 8, n):
                    if depth[cy, cx] != d:
                        continue
                    x, y, md = 8 * cx, 8 * cy, int(mode[cy, cx])
                    if d == 3:
                        px, py = x & ~15, y & ~15
                        if px + 16 > w or py + 16 > h:
                            under_cut_parent += 1
                        elif (x, y) == (px, py):
                            first_children += 1
                            places[qp].add(("absent" if x == 0 else "left CTU" if x % 64 == 0 else "inside",
                                            "absent" if y == 0 else "across a CTU row" if y % 64 == 0 else "inside"))
                    l = int(mode[cy, cx - 1]) if x > 0 else 1
                    a = int(mode[cy - 1, cx]) if y % 64 else 1
                    preds = chains._mpm(l, a)
                    mpm[qp, d].add("first" if md == preds[0] else "second or third" if md in preds else "none")
                    patterns[qp, d].add(_planes_with_levels(coeff[(cy // 8) * wc + cx // 8], x % 64, y % 64, 64 >> d))
    print(first_children, under_cut_parent, {k: sorted(v) for k, v in patterns.items()})
    for qp in (22, 37):
        assert len(places[qp]) == 9, (qp, sorted(places[qp]))
        for d in (2, 3):
            assert mpm[qp, d] == {"first", "second or third", "none"}, (qp, d, mpm[qp, d])
    assert first_children >= 320 and under_cut_parent >= 640, (first_children, under_cut_parent)
    every = {(y, u, v) for y in (False, True) for u in (False, True) for v in (False, True)}
    assert patterns[37, 2] == every and patterns[37, 3] == every, (sorted(patterns[37, 2]), sorted(patterns[37, 3]))
    assert patterns[22, 3] >= every - {(False, False, True), (False, True, False)}, sorted(patterns[22, 3])
    assert patterns[22, 2] >= {p for p in every if p[0]}, sorted(patterns[22, 2])


# ---- the device
@pytest.fixture(scope="module")
def hiplib():
    import kvazaar_amd
    lib = kvazaar_amd.load_library()
    assert lib.kvz_hip_device_count() >= 1
    return lib


SIZES = [(64, 64), (128, 128), (24, 200), (200, 24), (136, 72), (72, 136), (8, 8)]
GROUPS = [(w, h, qp) for (w, h) in SIZES for qp in (4, 22, 37, 51)]


def _batch_twice(lib, model, w, h, frames, want, download=None):
    """The pictures in one batch, run twice: the second run starts from the first one's border records, reconstruction and coefficient blocks."""
    b = cc.HipBatch(lib, w, h, len(frames))
    try:
        for i, f in enumerate(frames):
            b.upload(i, f)
        for run in range(2):
            b.run(model)
            for i in range(len(frames)):
                got = b.download(i)
                if download:
                    download(b, i, got)
                assert not cc.compare(want[i], got), (w, h, run, i, cc.compare(want[i], got))
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS, ids=lambda g: f"{g[0]}x{g[1]}-qp{g[2]}")
def test_hip_reuse_equals_oracle(oracle, hiplib, group):
    w, h, qp = group
    model = cc.hip_cost_model(hiplib, qp, cc.coeff_weights(qp))
    assert bool(model.coeff_cabac) == (qp >= 28)
    cases = [(w, h, kind, key, qp) for kind, key in CONTENTS]
    _batch_twice(hiplib, model, w, h, [_frame(c) for c in cases], [roles._want(oracle, c) for c in cases])


@pytest.mark.gpu
@pytest.mark.parametrize("switches", [FROZEN, FAST], ids=["frozen", "fast"])
def test_hip_reuse_other_instantiations_equal_oracle(oracle, hiplib, switches):
    w, h, qp = 128, 128, 22
    model = _with(cc.hip_cost_model(hiplib, qp, cc.coeff_weights(qp)), switches)
    frames = [_frame((w, h, kind, key, qp)) for kind, key in CONTENTS]
    want = [cc.run_oracle(oracle, model, w, h, f) for f in frames]
    assert 3 in roles._depths(want)
    _batch_twice(hiplib, model, w, h, frames, want)


@pytest.mark.gpu
def test_hip_reuse_medium_equals_oracle(oracle, hiplib):
    w, h, qp = 128, 128, 22
    model = _with(cc.hip_cost_model(hiplib, qp, cc.coeff_weights(qp)), MEDIUM)
    frames = [_frame((w, h, kind, key, qp)) for kind, key in CONTENTS]
    want = [cc.run_oracle_nxn(oracle, model, w, h, f) for f in frames]
    assert 3 in roles._depths(want)

    def partitions(b, i, got):
        got["part"], got["mode4"] = b.download_partitions(i)
    _batch_twice(hiplib, model, w, h, frames, want, partitions)


@pytest.mark.gpu
@pytest.mark.parametrize("clip", roles.SIGNHIDE_CLIPS, ids=lambda c: c[0])
def test_hip_reuse_signhide_pass_keeps_the_reference_encoders_pictures(hiplib, clip):
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    outs = roles._device_pass(hiplib, sc.table(hiplib, [qp], **sc.switches(clip)).models[0], None, w, h, sc.clip_frames(clip))
    assert 3 in roles._depths(outs) and [sc.sha(o["rec"]) for o in outs] == sc.fixture()[name]["rec"]


@pytest.mark.gpu
@pytest.mark.parametrize("clip", roles.LISTS_CLIPS, ids=lambda c: c[0])
def test_hip_reuse_scaling_list_pass_keeps_the_reference_encoders_pictures(hiplib, clip):
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    outs = roles._device_pass(hiplib, slc.table(hiplib, [qp], **slc.switches(clip)).models[0], [slc.lists("default")], w, h, slc.clip_frames(clip))
    assert 3 in roles._depths(outs) and [slc.sha(o["rec"]) for o in outs] == slc.fixture()[name]["rec"]
