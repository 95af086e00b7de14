"""A cost model per CTU on the MI355X (kvz_hip_ctu_models: kvz_hip_intra_frames_ctu_models, the CU-QP step behind it, kvz_hip_batch_loop_filters_ctu_models) against
tests/golden/ctu_qp.json -- what the reference encoder wrote under --roi maps (tests/golden/make_ctu_qp_golden.py) -- and against the entry points a uniform map must
reproduce.  Every comparison is byte-exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import ctu_common as cc
import ctu_qp_common as cq

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(cq.HERE, "golden"))
import make_golden as mg  # noqa: E402

FIXTURE = cq.fixture()


@pytest.fixture(scope="module")
def lib():
    import kvazaar_amd
    return kvazaar_amd.load_library()


def _batch(lib, w, h, frames):
    b = cc.HipBatch(lib, w, h, len(frames))
    for i, f in enumerate(frames):
        b.upload(i, f)
    return b


def _slices(data, sizes):
    out, at = [], 0
    for row in sizes:
        total = int(row.sum())
        out.append({"sha": cq.sha(np.frombuffer(bytes(data[at:at + total]), np.uint8)), "sizes": [int(v) for v in row]})
        at += total
    assert at == len(data)
    return out


def _cu(o, w, h):
    return mg.cu_digest(o["depth"].reshape(h // 8, w // 8), o["mode"].reshape(h // 8, w // 8))


@pytest.mark.parametrize("name", list(cq.CLIPS))
def test_pass_cu_qps_and_loop_filters_reproduce_the_reference_encoder(lib, name):
    """pass -> CU QPs -> deblocking, and pass -> deblocking + SAO, of every clip of the fixture"""
    w, h = cq.CLIPS[name][:2]
    want, frames, cm = FIXTURE[name], cq.clip_frames(name), cq.models(lib, name)
    b = _batch(lib, w, h, frames)
    try:
        assert b.run(cm) == 1
        outs = [b.download(i) for i in range(2)]
        assert [cq.sha(o["rec"]) for o in outs] == want["rec"]
        assert [_cu(o, w, h) for o in outs] == want["cu"]
        qps = [b.download_cu_qps(i) for i in range(2)]
        assert [[int(v) for v in words] for _, words in qps] == want["ctu_qp"]
        assert [cq.sha(plane) for plane, _ in qps] == want["cu_qp"]
        b.loop_filters(cm, deblock=True, sao=False)
        assert [cq.sha(b.download(i)["rec"]) for i in range(2)] == want["deblock"]
        assert _slices(*b.entropy_code(cm)) == want["entropy"]  # the slice data of the reference bitstream, cu_qp_delta included
        assert b.run(cm) == 1  # (the deblocked pictures are the batch's reconstruction now: the pass again)
        b.loop_filters(cm, deblock=True, sao=True)
        assert [cq.sha(b.download(i)["rec"]) for i in range(2)] == want["sao"]
    finally:
        b.close()


@pytest.mark.parametrize("name", ["3x3", "3x3-nowpp", "fast-5x2"])
def test_a_map_that_repeats_each_pictures_model_is_the_launch_with_a_model_per_picture(lib, name):
    """pass, deblocking and deblocking + SAO under a uniform map == kvz_hip_intra_frames_models / kvz_hip_batch_loop_filters_models, pictures at two QPs"""
    from kvazaar_amd.batch import CtuModels, PictureModels
    w, h, _, qp = cq.CLIPS[name][:4]
    frames, qps = cq.clip_frames(name), [qp, qp + 4]
    ctus = cq.grid(name)[0] * cq.grid(name)[1]
    cm = CtuModels(lib, qps, [[q] * ctus for q in qps], weights=cq.weights, **cq.switches(name))
    pm = PictureModels(lib, qps, weights=cq.weights, **cq.switches(name))
    a, b = _batch(lib, w, h, frames), _batch(lib, w, h, frames)
    try:
        assert a.run(cm) == 1 and b.run(pm) == 1
        for i in range(2):
            assert not cc.compare(a.download(i), b.download(i)), i
            plane, words = a.download_cu_qps(i)
            assert set(plane.tolist()) == {qps[i]} and {int(v) & 0xffff for v in words} == {qps[i] | qps[i] << 8}
        for sao in (False, True):
            if sao:
                assert a.run(cm) == 1 and b.run(pm) == 1
            a.loop_filters(cm, deblock=True, sao=sao)
            b.loop_filters(pm, deblock=True, sao=sao)
            assert [cq.sha(a.download(i)["rec"]) for i in range(2)] == [cq.sha(b.download(i)["rec"]) for i in range(2)], sao
    finally:
        a.close()
        b.close()


def test_pictures_with_maps_and_uniform_pictures_in_one_launch_each_come_out_as_if_alone(lib):
    """[3x3 p0 under its map, p0 uniform at 37, p1 uniform at 22, 3x3 p1 under its map]: two sizes of map QPs beside uniform pictures, both coefficient pricings"""
    from kvazaar_amd.batch import CtuModels, PictureModels
    name = "3x3"
    w, h, _, qp = cq.CLIPS[name][:4]
    p, maps, want = cq.clip_frames(name), cq.ctu_qps(name), FIXTURE[name]
    cm = CtuModels(lib, [qp, 37, 22, qp], [maps[0], [37] * 9, [22] * 9, maps[1]], weights=cq.weights)
    pm = PictureModels(lib, [37, 22], weights=cq.weights)
    b, u = _batch(lib, w, h, [p[0], p[0], p[1], p[1]]), _batch(lib, w, h, [p[0], p[1]])
    try:
        assert b.run(cm) == 1 and u.run(pm) == 1
        outs = [b.download(i) for i in range(4)]
        assert [cq.sha(outs[0]["rec"]), cq.sha(outs[3]["rec"])] == want["rec"] and [_cu(outs[0], w, h), _cu(outs[3], w, h)] == want["cu"]
        assert not cc.compare(outs[1], u.download(0)) and not cc.compare(outs[2], u.download(1))
        assert [[int(v) for v in b.download_cu_qps(i)[1]] for i in (0, 3)] == want["ctu_qp"]
        b.loop_filters(cm, deblock=True, sao=False)
        u.loop_filters(pm, deblock=True, sao=False)
        got = [cq.sha(b.download(i)["rec"]) for i in range(4)]
        assert [got[0], got[3]] == want["deblock"] and got[1:3] == [cq.sha(u.download(i)["rec"]) for i in range(2)]
        coded = _slices(*b.entropy_code(cm))
        assert [coded[0], coded[3]] == want["entropy"]
    finally:
        b.close()
        u.close()


def _refusals(lib, name):
    """(what is wrong, a CtuModels the library must refuse, words of its message)"""
    from kvazaar_amd.batch import CtuModels
    qp, ctus = cq.CLIPS[name][3], cq.grid(name)[0] * cq.grid(name)[1]
    good = lambda: cq.models(lib, name)  # noqa: E731
    size = good()
    size.struct.struct_size += 4
    null = good()
    null.struct.model_of_ctu = None
    index = good()
    index.index[ctus + 1] = index.pictures.struct.n_models
    inner = good()
    inner.pictures.struct.struct_size -= 4
    table = good()
    table.struct.pictures = None
    switched = []
    for switch in ("signhide", "rdoq", "search_nxn"):
        bad = good()
        for m in bad.pictures.models:  # (with what picture_models_known wants beside the switch)
            setattr(m, switch, 1)
            m.coeff_cabac = m.search_32x32 = 1
        switched.append((switch, bad, "rdoq / search_nxn / signhide"))
    span = CtuModels(lib, [qp, qp], [[qp - 13] * ctus, [qp - 13] * (ctus - 1) + [qp + 13]], weights=cq.weights)
    return [("struct_size", size, "kvz_hip_ctu_models.struct_size"), ("a NULL map", null, "model index per CTU"), ("a NULL table", table, "needs a table"),
            ("a map index", index, f"model_of_ctu[1][1] = {index.pictures.struct.n_models}"), ("the table's struct_size", inner, "kvz_hip_picture_models.struct_size"),
            ("a span of 26", span, "span more than 25")] + switched


def test_every_refusal_leaves_the_batch_usable(lib, capfd):
    name = "3x3"
    w, h = cq.CLIPS[name][:2]
    b = _batch(lib, w, h, cq.clip_frames(name))
    try:
        good, want = cq.models(lib, name), FIXTURE[name]["rec"]
        for what, bad, words in _refusals(lib, name):
            capfd.readouterr()
            assert b.launch(bad) == -1, what
            assert words in capfd.readouterr().err, what
            assert b.run(good) == 1 and [cq.sha(b.download(i)["rec"]) for i in range(2)] == want, what  # a correct launch after each
        b.loop_filters(good, deblock=True, sao=False)
        assert [cq.sha(b.download(i)["rec"]) for i in range(2)] == FIXTURE[name]["deblock"]
        from kvazaar_amd.batch import BatchError, ScalingLists
        assert b.run(good) == 1
        with pytest.raises(BatchError):
            b.loop_filters(cq.models(lib, name, zero=True), deblock=True, sao=False)  # another map than the pass's: its lambdas and the pass's CU QPs do not belong together
        assert "not the map of the batch's last pass" in capfd.readouterr().err
        b.set_scaling_lists([ScalingLists.default(lib)])
        assert b.launch(cq.models(lib, name)) == -1 and "scaling lists" in capfd.readouterr().err
        b.clear_scaling_lists()
        qp = cq.CLIPS[name][3]
        assert b.run(cc.hip_cost_model(lib, qp, cq.weights(qp))) == 1
        with pytest.raises(BatchError):
            b.loop_filters(cq.models(lib, name), deblock=True, sao=False)  # no pass with a map has run: the CU QPs come from it
        assert "last pass was no kvz_hip_intra_frames_ctu_models" in capfd.readouterr().err
        assert b.run(cq.models(lib, name)) == 1
        assert [cq.sha(b.download(i)["rec"]) for i in range(2)] == FIXTURE[name]["rec"]
    finally:
        b.close()


def test_the_other_schedule_is_refused(lib, capfd, monkeypatch):
    monkeypatch.setenv("KVZ_HIP_SCHED", "wave")
    b = _batch(lib, 64, 64, cq.clip_frames("one-ctu"))
    monkeypatch.delenv("KVZ_HIP_SCHED")
    try:
        assert b.launch(cq.models(lib, "one-ctu")) == -1 and "KVZ_HIP_SCHED=wave" in capfd.readouterr().err
    finally:
        b.close()


def test_a_plain_launch_after_a_launch_with_a_map_is_the_plain_encode(lib):
    """no map state is left behind: kvz_hip_intra_frames on the same batch gives the reference's encode without --roi"""
    from kvazaar_amd.batch import BatchError
    name = cq.ZERO_MAP
    w, h, _, qp = cq.CLIPS[name][:4]
    b = _batch(lib, w, h, cq.clip_frames(name))
    try:
        zero = cq.models(lib, name, zero=True)  # the all-zero map: the plain encode's pictures, a delta of 0 in every CTU that has a coefficient
        assert b.run(zero) == 1
        assert [cq.sha(b.download(i)["rec"]) for i in range(2)] == FIXTURE[name]["plain_rec"] and _slices(*b.entropy_code(zero)) == FIXTURE[name]["entropy_zero_map"]
        assert b.run(cq.models(lib, name)) == 1
        assert b.run(cc.hip_cost_model(lib, qp, cq.weights(qp))) == 1
        assert [cq.sha(b.download(i)["rec"]) for i in range(2)] == FIXTURE[name]["plain_rec"]
        with pytest.raises(BatchError):
            b.entropy_code(cq.models(lib, name))  # ... nor are its coded deltas
        with pytest.raises(BatchError):
            b.download_cu_qps(0)  # the CU QPs of the earlier pass are not this pass's
    finally:
        b.close()
