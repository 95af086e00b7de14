"""Units of 16 and 32 samples run the arithmetic stages of their reconstruction (kvz_ctu.hpp recon_tus: prediction, quantise / dequantise, reconstruct + SSD)
eight samples per lane: a 16x16 CU as 48 lane tasks in one trip of one wavefront, a 32x32 unit as 192 in two.  Every output equals the oracle's -- host
simulation here (it runs the same decomposition: wide_task / predict_row8 / plane_sums, the per-sample arithmetic of kvz_recon.hpp), the device under -m gpu -- and a test of the pictures themselves fails when
they stop exercising that code: every class of intra mode decided at depths 0, 1 and 2, every pattern of planes with levels among the decided 32x32 regions.
Pictures whose CTUs are cut by the border (the list of tests/test_ctu_movers.py) put such units next to the picture's edge."""
import ctypes as C

import numpy as np
import pytest

import ctu_common as cc
from test_hostsim import hostsim  # noqa: F401  (fixture)

# (width, height, kind, seed or adversarial name, QP)
BASE = [(w, h, kind, key, qp) for (w, h) in [(128, 128), (192, 128)] for qp in (22, 37)
        for kind, key in [("small", 4321), ("large", 4321), ("adversarial", "flat"), ("adversarial", "noise"), ("adversarial", "ramp"), ("adversarial", "blocks")]]
EXTRA = [(128, 128, kind, seed, qp) for kind in ("small", "large") for seed in (1, 6) for qp in (22, 27, 32, 37)]  # modes 10 / 26 decided at depth 2
BORDER = [(w, h, kind, 4321, qp) for (w, h) in [(24, 200), (200, 24), (136, 72), (72, 136), (264, 88), (96, 136)] for qp in (22, 37) for kind in ("small", "large")]
COVER = BASE + EXTRA
CASES = COVER + BORDER
_id = lambda c: f"{c[0]}x{c[1]}-{c[2]}-{c[3]}-qp{c[4]}"  # noqa: E731


def _frame(case):
    w, h, kind, key, _ = case
    if kind == "adversarial":
        return cc.adversarial_frames(w, h)[key]
    return cc.yuv_frames(w, h, 1, key, kind)[0]


def _oracle_model(oracle, qp):
    """the oracle's model builder on the committed constants of the reference build (tests/golden/model_constants.json)"""
    k = cc.model_constants()
    m = cc.CostModel()
    f = oracle.lib.kvz_oracle_intra_cost_model
    f.restype = None
    f.argtypes = [C.c_int, C.c_float * 128, C.c_uint64, C.POINTER(cc.CostModel)]
    f(qp, (C.c_float * 128)(*k["entropy_fbits"]), cc.coeff_weights(qp), C.byref(m))
    return m


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_hostsim_recon_wide_equals_oracle(oracle, hostsim, case):  # noqa: F811
    w, h, _, _, qp = case
    m = _oracle_model(oracle, qp)
    assert bool(m.coeff_cabac) == (qp >= 28)
    yuv = _frame(case)
    a, b = cc.run_oracle(oracle, m, w, h, yuv), cc.run_hostsim(hostsim.lib, m, w, h, yuv)
    assert not cc.compare(a, b), (case, cc.compare(a, b))


def _mode_class(mode):
    if mode < 2:
        return ("planar", "dc")[mode]
    if mode in (10, 26):
        return "10/26"
    if mode in (2, 18, 34):
        return "2/18/34"
    if 11 <= mode <= 25:
        return "negative displacement"
    return "other horizontal" if mode < 18 else "other vertical"


CLASSES = {"planar", "dc", "10/26", "2/18/34", "negative displacement", "other horizontal", "other vertical"}


def test_pictures_exercise_the_wide_stages(oracle):
    """what the oracle DECIDES on the covering pictures (whole CTUs): the seven classes of modes at each of the depths whose CUs are reconstructed by the wide
    stages, and among the decided 32x32 regions of depth <= 1 every pattern of planes with levels the reductions have to tell apart"""
    seen = {d: set() for d in (0, 1, 2)}
    patterns = set()
    for case in COVER:
        w, h, _, _, qp = case
        o = cc.run_oracle(oracle, _oracle_model(oracle, qp), w, h, _frame(case))
        depth, mode, coeff = o["depth"].reshape(h // 8, w // 8), o["mode"].reshape(h // 8, w // 8), o["coeff"].reshape(-1, 6144)
        for d in (0, 1, 2):
            seen[d] |= {_mode_class(int(v)) for v in np.unique(mode[depth == d])}
        for cy in range(h // 64):
            for cx in range(w // 64):
                blk = coeff[cy * (w // 64) + cx]
                for q in range(4):  # z-order: the 32x32 quadrants of the CTU
                    if depth[cy * 8 + (q >> 1) * 4, cx * 8 + (q & 1) * 4] > 1:
                        continue
                    y, u, v = (bool(np.any(blk[o0 + q * n:o0 + (q + 1) * n])) for o0, n in ((0, 1024), (4096, 256), (5120, 256)))
                    patterns.add("none" if not (y or u or v) else "luma" if y and not (u or v) else "luma+one" if y and u != v else "all" if y and u and v else "other")
    for d in (0, 1, 2):
        assert seen[d] == CLASSES, (d, CLASSES - seen[d])
    assert {"none", "luma", "luma+one", "all"} <= patterns, patterns


def test_border_pictures_cut_ctus():
    assert all(w % 64 or h % 64 for w, h, *_ in BORDER) and all(w % 8 == 0 and h % 8 == 0 for w, h, *_ in CASES)


@pytest.fixture(scope="module")
def hiplib():
    import kvazaar_amd
    lib = kvazaar_amd.load_library()
    assert lib.kvz_hip_device_count() >= 1
    return lib


_BATCHES = sorted({(c[0], c[1], c[4]) for c in CASES})


@pytest.mark.gpu
@pytest.mark.parametrize("batch", _BATCHES, ids=lambda b: f"{b[0]}x{b[1]}-qp{b[2]}")
def test_hip_recon_wide_equals_oracle(oracle, hiplib, batch):
    """All pictures of one size and QP in one batch, run twice: the second run starts from the first one's border records, reconstruction and coefficient blocks."""
    w, h, qp = batch
    model = cc.hip_cost_model(hiplib, qp, cc.coeff_weights(qp))
    assert bool(model.coeff_cabac) == (qp >= 28)
    frames = [_frame(c) for c in CASES if (c[0], c[1], c[4]) == batch]
    b = cc.HipBatch(hiplib, w, h, len(frames))
    try:
        for i, f in enumerate(frames):
            b.upload(i, f)
        want = [cc.run_oracle(oracle, model, w, h, f) for f in frames]
        for run in range(2):
            b.run(model)
            for i in range(len(frames)):
                got = b.download(i)
                assert not cc.compare(want[i], got), (batch, run, i, cc.compare(want[i], got))
    finally:
        b.close()
