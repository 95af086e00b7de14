"""The cost of an evaluated CU (kvz_ctu.hpp cu_cost_prepare / cu_cost_batched): twelve lanes of the wavefront that idles in the selection phase prepare the price and
the successor state of both values of every bin, thread 0 chooses among them once mode and coded-block flags are known and adds up cu_bits() * lambda and
leaf_rd_cost() in the callees' order.  Every output of the pass, costs included (bit-exact doubles), equals the oracle's -- the host simulation here (it compiles
the same text), the device under -m gpu -- on 64x64 and on 72x40, whose 16x16 CUs at x = 64 and y = 32 cross the picture's edges (the split flag of such a CU is
not coded: it is split without being priced) and whose CTU at x = 64 puts CUs on a CTU's left edge with x > 0 (they derive their predictors for the mock encode
themselves), from QP 4 to QP 51, with the search contexts adapting and frozen (`adaptive = 0`).  A test of the pictures themselves fails when the oracle's own
decisions on them stop covering what the choice distinguishes: the three classes of the decided mode (not a most probable mode, the first predictor, another one)
and the four pairs of chroma flags under both values of the luma flag.  (Written with a change that moved the sums of prices to the preparing lanes as well and
an 8x8 CU's preparation into its SATD phase; that change was slower and is kept as profiles/experiments/cost_sums_prepared_aside_slower.patch, which these tests
pass too.)"""
import numpy as np
import pytest

import ctu_common as cc
from test_ctu_recon_wide import _frame, _oracle_model
from test_hostsim import hostsim  # noqa: F401  (fixture)

SIZES = [(64, 64), (72, 40)]
CONTENTS = [("small", 4321), ("large", 4321), ("adversarial", "noise"), ("adversarial", "flat")]
QPS = (4, 22, 37, 51)
CASES = [(w, h, kind, key, qp, adaptive) for (w, h) in SIZES for kind, key in CONTENTS for qp in QPS for adaptive in (1, 0)]
_id = lambda c: f"{c[0]}x{c[1]}-{c[2]}-{c[3]}-qp{c[4]}-{'adaptive' if c[5] else 'frozen'}"  # noqa: E731

_WANT = {}


def _model(oracle, qp, adaptive):
    m = _oracle_model(oracle, qp)
    m.adaptive = adaptive
    return m


def _want(oracle, case):
    """the oracle's pass on one picture, computed once and shared"""
    if case not in _WANT:
        w, h, _, _, qp, adaptive = case
        _WANT[case] = cc.run_oracle(oracle, _model(oracle, qp, adaptive), w, h, _frame(case[:5]))
    return _WANT[case]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_hostsim_costs_equal_oracle(oracle, hostsim, case):  # noqa: F811
    w, h, _, _, qp, adaptive = case
    m = _model(oracle, qp, adaptive)
    assert bool(m.coeff_cabac) == (qp >= 28) and int(m.adaptive) == adaptive
    a, b = _want(oracle, case), cc.run_hostsim(hostsim.lib, m, w, h, _frame(case[:5]))
    assert not cc.compare(a, b), (case, cc.compare(a, b))
    assert a["cost"].tobytes() == b["cost"].tobytes()  # (compare() looks at it too: said once more, it is what this file is about)


# ---- do the pictures exercise the table?
def _zorder(x, y):
    z = 0
    for i in range(4):
        z |= ((x >> i) & 1) << (2 * i) | ((y >> i) & 1) << (2 * i + 1)
    return z


def _predictors(mode, x, y):
    """intra.c:89-147 kvz_intra_get_dir_luma_predictor on the decided modes of the picture: the CU at (x, y), its left and above neighbours"""
    left = int(mode[y // 8, x // 8 - 1]) if x > 0 else 1
    above = int(mode[y // 8 - 1, x // 8]) if y > 0 and y % 64 != 0 else 1  # DC across a CTU row boundary
    if left == above:
        if left < 2:
            return [0, 1, 26]
        return [left, 2 + ((left + 29) % 32), 2 + ((left - 2 + 1) % 32)]
    third = 0 if 0 not in (left, above) else (1 if 1 not in (left, above) else 26)
    return [left, above, third]


def _decided_cus(o, w, h):
    """of one pass's outputs, per CU decided at depth 2 or 3: its mode class (0 not a most probable mode, 1 the first predictor, 2 another) and (cb_y, cb_u, cb_v)"""
    depth, mode, coeff = o["depth"].reshape(h // 8, w // 8), o["mode"].reshape(h // 8, w // 8), o["coeff"].reshape(-1, 6144)
    wc = (w + 63) // 64
    for y8 in range(h // 8):
        for x8 in range(w // 8):
            d = int(depth[y8, x8])
            if d < 2 or (d == 2 and (x8 % 2 or y8 % 2)):
                continue
            n = 256 if d == 2 else 64
            ctu = coeff[(y8 // 8) * wc + x8 // 8]
            lx, ly = (x8 % 8) * 8, (y8 % 8) * 8
            cb_y = bool(np.any(ctu[_zorder(lx // 4, ly // 4) * 16:][:n]))
            cb_u, cb_v = (bool(np.any(ctu[base + _zorder(lx // 8, ly // 8) * 16:][:n // 4])) for base in (4096, 5120))
            preds = _predictors(mode, x8 * 8, y8 * 8)
            m = int(mode[y8, x8])
            yield (0 if m not in preds else (1 if m == preds[0] else 2)), (cb_y, cb_u, cb_v), d


def test_pictures_exercise_the_cost_table(oracle):
    """what the oracle alone DECIDES on the pictures: all three mode classes, all four pairs of chroma flags under both values of the luma flag, CUs of both sizes
    that are priced from the prepared table, and -- on 72x40 -- 16x16 CUs that cross the right and the bottom edge of the picture, whose split flag is not coded"""
    classes, flags, depths = {}, {}, set()
    for case in CASES:
        for cls, f, d in _decided_cus(_want(oracle, case), case[0], case[1]):
            classes[cls] = classes.get(cls, 0) + 1
            flags[f] = flags.get(f, 0) + 1
            depths.add(d)
    print(sorted(classes.items()), sorted(flags.items()))
    assert set(classes) == {0, 1, 2}, classes
    assert len(flags) == 8, sorted(flags.items())
    assert depths == {2, 3}
    crossing = 0
    for case in CASES:
        w, h = case[0], case[1]
        depth = _want(oracle, case)["depth"].reshape(h // 8, w // 8)
        for y in range(0, h, 16):
            for x in range(0, w, 16):
                if x + 16 > w or y + 16 > h:  # implicitly split: no flag (encode_coding_tree.c:975-986)
                    assert depth[y // 8, x // 8] == 3, (case, x, y)
                    crossing += 1
    assert crossing > 0
    # ... and CUs on a CTU's left edge that is not the picture's: the mock encode derives their predictors without a left neighbour
    assert any(case[0] > 64 for case in CASES)


# ---- the device
@pytest.fixture(scope="module")
def hiplib():
    import kvazaar_amd
    lib = kvazaar_amd.load_library()
    assert lib.kvz_hip_device_count() >= 1
    return lib


GROUPS = [(w, h, qp, adaptive) for (w, h) in SIZES for qp in QPS for adaptive in (1, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS, ids=lambda g: f"{g[0]}x{g[1]}-qp{g[2]}-{'adaptive' if g[3] else 'frozen'}")
def test_hip_costs_equal_oracle(oracle, hiplib, group):
    """All pictures of one size, QP and context mode in one batch, run twice: the second run starts from the first one's border records, reconstruction and
    coefficient blocks."""
    w, h, qp, adaptive = group
    model = cc.hip_cost_model(hiplib, qp, cc.coeff_weights(qp))
    model.adaptive = adaptive
    assert bool(model.coeff_cabac) == (qp >= 28)
    cases = [(w, h, kind, key, qp, adaptive) for kind, key in CONTENTS]
    frames = [_frame(c[:5]) for c in cases]
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
