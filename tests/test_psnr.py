"""Per-picture distortion, the host side: tests/golden/psnr.json holds, for clips the existing fixtures already pin, the exact sums of squared differences
between the reference encoder's input and its --debug reconstruction and the ` PSNR Y U V` text it printed per picture (tests/golden/make_psnr_golden.py).

  * kvz_hip_psnr (the library loads without a GPU; this function touches no device) + psnr_text turn every recorded sum into the recorded text;
  * the oracle's chains (CTU pass, deblocking / SAO; the low-delay sequence oracle) produce pictures whose sums against the source are the recorded ones;
  * where oracle/_ref exists, the fixture is what the reference encoder gives today.
The device side is tests/test_gpu_psnr.py."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import ctu_common as cc
import flatapi
import inter_common as ic
from test_encoder_parity import _oracle_chain, oracle_model
from test_sao_decision import oracle_sao_chain

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_psnr_golden as pg  # noqa: E402

GOLDEN = json.load(open(os.path.join(HERE, "golden", "psnr.json")))


def _lib():
    import kvazaar_amd
    return ctypes.CDLL(kvazaar_amd.build_library())


def test_fixture_covers_what_it_is_for():
    assert sorted(GOLDEN) == sorted([c[0] for c in pg.INTRA_CLIPS] + ["lowdelay-" + n for n in pg.LOWDELAY_CASES])
    for clip in pg.INTRA_CLIPS:
        assert sorted(GOLDEN[clip[0]]) == [str(i) for i in range(clip[3])]
    qps = {c[6] for c in pg.INTRA_CLIPS if c[7] == "ultrafast"}
    assert min(qps) < 28 <= max(qps)
    assert {(c[8], c[9]) for c in pg.INTRA_CLIPS} >= {(0, 0), (1, 0), (1, 1)}
    sizes = {(c[1], c[2]) for c in pg.INTRA_CLIPS}
    assert (64, 64) in sizes and (1920, 1080) in sizes
    assert all(len(GOLDEN["lowdelay-" + n]) >= 4 for n in pg.LOWDELAY_CASES)
    assert os.path.getsize(os.path.join(HERE, "golden", "psnr.json")) < 16384


def test_kvz_hip_psnr_reproduces_the_encoders_text():
    """every recorded sum through kvz_hip_psnr and psnr_text == the text the reference encoder printed for that picture, character for character"""
    from kvazaar_amd import batch
    lib = _lib()
    dims = {c[0]: (c[1], c[2]) for c in pg.INTRA_CLIPS}
    dims.update({"lowdelay-" + c[0]: (c[1], c[2]) for c in ic.CASES if c[0] in pg.LOWDELAY_CASES})
    n = 0
    for name, pics in GOLDEN.items():
        w, h = dims[name]
        for poc, p in pics.items():
            got = [batch.psnr(lib, s, px) for s, px in zip(p["sse"], (w * h, w * h // 4, w * h // 4))]
            assert batch.psnr_text(got) == p["psnr_text"], (name, poc)
            assert np.array_equal(batch.psnr_of_planes(lib, p["sse"], w, h), got)
            n += 1
    assert n == 17
    assert batch.psnr(lib, 0, 64 * 64) == 999.99
    assert batch.psnr_text([batch.psnr(lib, 0, 4096)] * 3) == " PSNR Y 999.9900 U 999.9900 V 999.9900"
    # the package-level wrappers are the same functions
    import kvazaar_amd
    assert kvazaar_amd.psnr_text is batch.psnr_text
    # beyond 32 bits: a 3840x2160 plane of 0 against 255 is every sample at the maximum error
    assert batch.psnr(lib, 3840 * 2160 * 65025, 3840 * 2160) == 0.0


@pytest.mark.parametrize("clip", pg.INTRA_CLIPS, ids=lambda c: c[0])
def test_oracle_chain_has_the_recorded_distortion(oracle, clip):
    """the pictures the existing digests pin (tests/test_encoder_parity.py, tests/test_sao_decision.py run the same chains) have the recorded sums"""
    name, w, h, n, seed, kind, qp, preset, deblock, sao = clip
    model = oracle_model(oracle, qp)
    for i, f in enumerate(cc.yuv_frames(w, h, n, seed, kind)):
        rec = oracle_sao_chain(oracle, model, w, h, f)[0] if sao else _oracle_chain(oracle, model, w, h, f, qp, deblock)
        assert pg.exact_sse(f, rec, w, h) == GOLDEN[name][str(i)]["sse"], (name, i)


@pytest.mark.parametrize("name", pg.LOWDELAY_CASES)
def test_oracle_lowdelay_sequence_has_the_recorded_distortion(oracle, name):
    case = [c for c in ic.CASES if c[0] == name][0]
    _, w, h, n, qp, preset, dbk, sao, owf, _ = case
    frames = ic.case_frames(case)
    _, rf, _, _ = ic.oracle_encode(oracle, w, h, frames, qp, preset=preset, deblock=bool(dbk), sao=bool(sao), mv_constraint=owf > 0)
    for poc in range(n):
        assert pg.exact_sse(frames[poc], rf[poc], w, h) == GOLDEN["lowdelay-" + name][str(poc)]["sse"], poc


def test_psnr_fixture_matches_reference_build(tmp_path):
    """where oracle/_ref exists, the committed fixture is what the reference encoder reads, writes and prints today (two clips)"""
    if not os.path.exists(os.path.join(flatapi.ROOT, "oracle", "_ref", "kvazaar_ref")):
        pytest.skip("oracle/_ref not built")
    clip = pg.INTRA_CLIPS[3]
    assert pg.intra_entry(clip, str(tmp_path)) == GOLDEN[clip[0]]
    assert pg.lowdelay_entry(pg.LOWDELAY_CASES[0], str(tmp_path)) == GOLDEN["lowdelay-" + pg.LOWDELAY_CASES[0]]
