"""Pictures under different cost models in ONE launch on the MI355X (kvz_hip_picture_models; kvz_hip_intra_frames_models, kvz_hip_batch_loop_filters_models,
kvz_hip_batch_entropy_code[_then]_models).  Every picture stays an ordinary constant-QP picture, so every output has a reference that exists already: the reference
encoder's digests under tests/golden/, and the same picture in a uniform batch at its QP through the single-model entry points."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import ctu_common as cc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as mg  # noqa: E402

RECON = json.load(open(os.path.join(HERE, "golden", "encoder_recon.json")))
ENTROPY = json.load(open(os.path.join(HERE, "golden", "entropy.json")))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def _weights(qp):
    return cc.coeff_weights(qp) if qp < 50 else 0


@pytest.fixture(scope="module")
def lib():
    import kvazaar_amd
    return kvazaar_amd.load_library()


def _table(lib, qps, **switches):
    from kvazaar_amd.batch import PictureModels
    return PictureModels(lib, qps, weights=_weights, **switches)


def _model(lib, qp, **switches):
    m = cc.hip_cost_model(lib, qp, _weights(qp))
    for k, v in switches.items():
        setattr(m, k, v)
    return m


def _batch(lib, w, h, frames):
    b = cc.HipBatch(lib, w, h, len(frames))
    for i, f in enumerate(frames):
        b.upload(i, f)
    return b


def _split(data, sizes):
    out, at = [], 0
    for row in sizes:
        total = int(row.sum())
        out.append((bytes(data[at:at + total]), [int(v) for v in row]))
        at += total
    assert at == len(data)
    return out


def test_mixed_batch_through_pass_deblocking_and_sao_reproduces_the_reference_encoder(lib):
    """[p0 @ 27, p0 @ 37, p1 @ 37, p1 @ 27] of the 200x136 clip -- both sides of fast-residual-cost 28 in one launch -- after the pass, after deblocking, after deblocking + SAO"""
    w, h, n, seed, kind = 200, 136, 2, 3, "small"
    p = cc.yuv_frames(w, h, n, seed, kind)
    qps, pic = [27, 37, 37, 27], [0, 0, 1, 1]
    pm = _table(lib, qps)
    b = _batch(lib, w, h, [p[i] for i in pic])
    try:
        def want(suffix, deblock, only=None):
            return [RECON[mg.clip_key(w, h, n, seed, kind, q, deblock) + suffix][i] for q, i in zip(qps, pic) if only is None or q == only]
        assert b.run(pm) == 1
        outs = [b.download(i) for i in range(4)]
        assert [_sha(o["rec"]) for o in outs] == want("", 0)
        assert [mg.cu_digest(o["depth"].reshape(h // 8, w // 8), o["mode"].reshape(h // 8, w // 8)) for o in outs] == want("/cu", 0)
        b.loop_filters(pm, deblock=True, sao=False)  # the deblock-only use
        assert [_sha(b.download(i)["rec"]) for i in range(4)] == want("", 1)
        b.run(pm)
        b.loop_filters(pm, deblock=True, sao=True)
        got = [_sha(b.download(i)["rec"]) for i in range(4)]
        assert [g for g, q in zip(got, qps) if q == 27] == want("/sao", 1, only=27)  # (the fixture has the final picture of this clip at QP 27)
    finally:
        b.close()


def test_mixed_adversarial_batch_with_sao_reproduces_the_reference_encoder(lib):
    """flat / noise / ramp / blocks at QP 32, then the same four at QP 40, one batch: band offsets and merges, every picture with its own lambda and SAO contexts"""
    w, h = 192, 136
    frames = cc.yuv_frames(w, h, 4, 0, "adversarial")
    pm = _table(lib, [32] * 4 + [40] * 4)
    b = _batch(lib, w, h, frames + frames)
    try:
        b.run(pm)
        b.loop_filters(pm, deblock=True, sao=True)
        got = [_sha(b.download(i)["rec"]) for i in range(8)]
        assert got == RECON[mg.clip_key(w, h, 4, 0, "adversarial", 32, 1) + "/sao"] + RECON[mg.clip_key(w, h, 4, 0, "adversarial", 40, 1) + "/sao"]
    finally:
        b.close()


INSTANTIATIONS = {
    "fast-estimate <false>": (dict(coeff_cabac=0), False),
    "cabac <true>": (dict(), False),                    # coeff_cabac per QP: the estimate below 28, the coder from 28 on, in one launch
    "search32 <false,true>": (dict(search_32x32=1, coeff_cabac=0), False),
    "search32 cabac <true,true>": (dict(search_32x32=1), False),
    "rdoq+nxn": (dict(search_32x32=1, coeff_cabac=1, rdoq=1, search_nxn=1), True),
    "no_wpp": (dict(no_wpp=1), False),
}


@pytest.mark.parametrize("name", list(INSTANTIATIONS))
def test_mixed_launch_equals_uniform_launches(lib, name):
    """16 seeded draws of per-picture QPs 0..51: every downloaded output of every picture of the mixed launch -- and, after the loop filters, its final picture and SAO
    parameters, then its slice data -- equals the same picture's from a uniform launch of the single-model entry points at its QP"""
    switches, nxn = INSTANTIATIONS[name]
    w, h, n = 200, 136, 6
    clip = cc.yuv_frames(w, h, 2, 3, "small") + cc.yuv_frames(w, h, 4, 0, "adversarial")
    rng = np.random.default_rng(1000 + len(name))
    mixed, uniform = _batch(lib, w, h, clip), _batch(lib, w, h, clip)
    try:
        reference = {}  # qp -> per picture (outputs, filtered picture, sao records, slice data) of the uniform batch

        def uniform_at(qp):
            if qp not in reference:
                m = _model(lib, qp, **switches)
                uniform.run(m)
                outs = [uniform.download(i) for i in range(n)]
                if nxn:
                    for i, o in enumerate(outs):
                        o["part"], o["mode4"] = uniform.download_partitions(i)
                uniform.loop_filters(m, deblock=True, sao=True)
                final = [uniform.download(i)["rec"] for i in range(n)]
                sao = [tuple(bytes(x) for x in uniform.sao_params(i)) for i in range(n)]
                coded = _split(*uniform.entropy_code(m, sao=True))
                reference[qp] = [(outs[i], final[i], sao[i], coded[i]) for i in range(n)]
            return reference[qp]
        for draw in range(16):
            qps = [int(q) for q in rng.integers(0, 52, n)]
            if draw == 0:
                qps[:2] = [27, 28]
            pm = _table(lib, qps, **switches)
            mixed.run(pm)
            outs = [mixed.download(i) for i in range(n)]
            if nxn:
                for i, o in enumerate(outs):
                    o["part"], o["mode4"] = mixed.download_partitions(i)
            mixed.loop_filters(pm, deblock=True, sao=True)
            final = [mixed.download(i)["rec"] for i in range(n)]
            sao = [tuple(bytes(x) for x in mixed.sao_params(i)) for i in range(n)]
            coded = _split(*mixed.entropy_code(pm, sao=True))
            for i, qp in enumerate(qps):
                ref = uniform_at(qp)[i]
                assert not cc.compare(outs[i], ref[0]), (draw, i, qp, cc.compare(outs[i], ref[0]))
                assert final[i].tobytes() == ref[1].tobytes(), (draw, i, qp, "loop filters")
                assert sao[i] == ref[2], (draw, i, qp, "sao parameters")
                assert coded[i] == ref[3], (draw, i, qp, "slice data")
    finally:
        mixed.close()
        uniform.close()


def _check_slice_data(got, names):
    want = [g for name in names for g in ENTROPY[name]]
    assert len(got) == len(want)
    for i, ((data, row), g) in enumerate(zip(got, want)):
        assert row == g["sizes"], i
        assert hashlib.sha256(data).hexdigest()[:24] == g["sha"], i


def test_slice_data_of_mixed_batches_equals_the_reference_encoders(lib):
    """noise-qp12 + noise-qp37 in one 192x136 batch, ultrafast-qp22 + ultrafast-qp32 in one 416x240 batch; the second through kvz_hip_batch_entropy_code_then_models,
    which starts the first batch's next pass -- under a table of its own -- beside the coder"""
    import entropy_common as ec
    cases = {c[0]: c for c in ec.CASES}
    noise = cc.yuv_frames(192, 136, 4, 0, "adversarial")
    a = _batch(lib, 192, 136, noise + noise)
    pa = _table(lib, [12] * 4 + [37] * 4)
    _, w, h, n22, seed22, kind22, qp22, _, _ = cases["ultrafast-qp22"]
    _, w32, h32, n32, seed32, kind32, qp32, _, _ = cases["ultrafast-qp32"]
    assert (w32, h32) == (w, h) == (416, 240) and (qp22, qp32) == (22, 32)
    c = _batch(lib, w, h, cc.yuv_frames(w, h, n22, seed22, kind22) + cc.yuv_frames(w, h, n32, seed32, kind32))
    pc = _table(lib, [22] * n22 + [32] * n32)
    try:
        a.run(pa)
        _check_slice_data(_split(*a.entropy_code(pa)), ["noise-qp12", "noise-qp37"])
        c.run(pc)
        pa_swapped = _table(lib, [37] * 4 + [12] * 4)  # a's next pass: the halves the other way round
        got = _split(*c.entropy_code(pc, then=(a, pa_swapped)))
        _check_slice_data(got, ["ultrafast-qp22", "ultrafast-qp32"])
        a.sync()  # the pass _then_models queued
        _check_slice_data(_split(*a.entropy_code(pa_swapped)), ["noise-qp37", "noise-qp12"])
    finally:
        a.close()
        c.close()


def test_then_models_refuses_a_bad_next_table_with_nothing_queued(lib):
    from kvazaar_amd.batch import BatchError
    frames = cc.yuv_frames(64, 64, 2, 9, "small")
    a, b = _batch(lib, 64, 64, frames), _batch(lib, 64, 64, frames)
    try:
        pm = _table(lib, [22, 30])
        a.run(pm)
        bad = _table(lib, [22, 30])
        bad.index[1] = 5
        with pytest.raises(BatchError, match=r"\(-3\)"):
            a.entropy_code(pm, then=(b, bad))
        b.sync()
        import ctypes as C
        flags = np.zeros(2, np.uint32)
        lib.kvz_hip_batch_debug_flags.argtypes = [C.c_void_p, C.c_void_p]
        lib.kvz_hip_batch_debug_flags.restype = C.c_uint
        assert lib.kvz_hip_batch_debug_flags(b.handle, flags.ctypes.data) == 0 and not flags.any()  # no pass has ever run on b
        with pytest.raises(BatchError):
            b.run(bad)
        with pytest.raises(BatchError):
            b.loop_filters(bad)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("qp", [22, 32])
def test_a_table_of_one_model_is_the_single_model_entry_point(lib, qp):
    """byte for byte: pass outputs, CTU costs, the filtered picture, SAO parameters, slice data"""
    w, h, n = 200, 136, 3
    frames = cc.yuv_frames(w, h, n, 11, "small")
    one, tab = _batch(lib, w, h, frames), _batch(lib, w, h, frames)
    try:
        m, pm = _model(lib, qp), _table(lib, [qp] * n)
        assert pm.struct.n_models == 1 and bytes(pm.models[0]) == bytes(m)
        one.run(m)
        tab.run(pm)
        for i in range(n):
            assert not cc.compare(one.download(i), tab.download(i)), i
        one.loop_filters(m, deblock=True, sao=True)
        tab.loop_filters(pm, deblock=True, sao=True)
        for i in range(n):
            assert one.download(i)["rec"].tobytes() == tab.download(i)["rec"].tobytes(), i
            assert [bytes(x) for x in one.sao_params(i)] == [bytes(x) for x in tab.sao_params(i)], i
        assert _split(*one.entropy_code(m, sao=True)) == _split(*tab.entropy_code(pm, sao=True))
        # ... and the single-model call on a batch that has run tables still is what it was
        tab.run(m)
        one.run(m)
        for i in range(n):
            assert not cc.compare(one.download(i), tab.download(i)), i
    finally:
        one.close()
        tab.close()
