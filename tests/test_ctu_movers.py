"""The code of the CTU program that only moves data (kvz_ctu.hpp: init, load_org, write_rec, commit, finish_info) moves 4 to 16 bytes per lane, and which
width it takes depends on the picture: 16-byte units when the width is a multiple of 16, 8 / 4-byte ones otherwise; CU maps as dwords when it is a multiple
of 32.  These pictures put every edge case of a wide move on the picture's border: one 8x8 CU (8x8), CTUs cut at 8 and at 24 samples in either direction
(24x200, 200x24, 136x72, 72x136), a width that is a multiple of 8 only next to one of 16 and one of 32 (264x88: 264 = 4 x 64 + 8; 136, 200, 24, 72: 8 mod 16;
every CTU of a bottom row sticks out, so the zero fill of the coefficient blocks runs).  QP 22 is the instantiation without the CABAC coefficient cost, QP 37 the
one with it.  Every output equals the oracle's: host simulation here, the device under -m gpu."""
import numpy as np
import pytest

import ctu_common as cc
import flatapi
from test_ctu_pipeline import oracle_model
from test_hostsim import hostsim  # noqa: F401  (fixture)

# (these six are multiples of 8 only in width; the three behind them take the 16-byte units -- 80 without, 96 and 128 with the dword CU maps -- with cut CTUs again)
SIZES = [(8, 8), (24, 200), (200, 24), (136, 72), (72, 136), (264, 88), (80, 40), (96, 136), (128, 72)]
_ids = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


def _frames(w, h):
    return [cc.yuv_frames(w, h, 1, 4321, "small")[0], cc.yuv_frames(w, h, 1, 4321, "large")[0]]


@pytest.mark.parametrize("qp", [22, 37])
@pytest.mark.parametrize("size", SIZES, ids=_ids)
def test_hostsim_movers_equal_oracle(oracle, hostsim, size, qp):  # noqa: F811
    if not flatapi.os.path.exists(flatapi.refshim_path()):
        pytest.skip("oracle/_ref not built")
    w, h = size
    m = oracle_model(oracle, flatapi.load_ref(0), qp)
    assert bool(m.coeff_cabac) == (qp >= 28)
    for i, yuv in enumerate(_frames(w, h)):
        a, b = cc.run_oracle(oracle, m, w, h, yuv), cc.run_hostsim(hostsim.lib, m, w, h, yuv)
        assert not cc.compare(a, b), (size, qp, i, cc.compare(a, b))


@pytest.fixture(scope="module")
def hiplib():
    import kvazaar_amd
    lib = kvazaar_amd.load_library()
    assert lib.kvz_hip_device_count() >= 1
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("qp", [22, 37])
@pytest.mark.parametrize("size", SIZES, ids=_ids)
def test_hip_movers_equal_oracle(oracle, hiplib, size, qp):
    """Both kinds of picture in one batch, run twice: the second run starts from the first one's border records, reconstruction and coefficient blocks."""
    w, h = size
    model = cc.hip_cost_model(hiplib, qp, cc.coeff_weights(qp))
    assert bool(model.coeff_cabac) == (qp >= 28)
    frames = _frames(w, h)
    b = cc.HipBatch(hiplib, w, h, len(frames))
    try:
        for i, f in enumerate(frames):
            b.upload(i, f)
        for run in range(2):
            b.run(model)
            for i, f in enumerate(frames):
                want, got = cc.run_oracle(oracle, model, w, h, f), b.download(i)
                assert not cc.compare(want, got), (size, qp, run, i, cc.compare(want, got))
    finally:
        b.close()


def test_sizes_cover_both_widths():
    assert {w % 16 == 0 for w, _ in SIZES} == {True, False} and {w % 32 == 0 for w, _ in SIZES if w % 16 == 0} == {True, False}
    assert np.all([w % 8 == 0 and h % 8 == 0 for w, h in SIZES])
