"""Sign data hiding (kvz_hip_intra_cost_model::signhide, kvazaar's --signhide) on the MI355X: the sign-hiding instantiations of the CTU pass, deblocking and the
entropy coder behind it, against the reference encoder run with --signhide (tests/golden/signhide.json) and, output by output, against the host simulation of the
same sources (tests/hostsim/hostsim_signhide.cpp).  That the other instantiations compute what they computed is what the existing GPU tests show."""
import json
import os
import sys

import numpy as np
import pytest

import ctu_common as cc
import signhide_common as sc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as mg  # noqa: E402

RECON = json.load(open(os.path.join(HERE, "golden", "encoder_recon.json")))
ENTROPY = json.load(open(os.path.join(HERE, "golden", "entropy.json")))


@pytest.fixture(scope="module")
def lib():
    import kvazaar_amd
    return kvazaar_amd.load_library()


@pytest.fixture(scope="module")
def sim():
    return sc.load_sim()


@pytest.fixture(scope="module")
def gold():
    return sc.fixture()


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


def _chain(lib, model, w, h, frames, qp=None):
    """pass -> (deblocking, with qp) -> entropy coder on a fresh batch: (outputs before the filters, deblocked pictures or None, [(slice data, sizes)])"""
    b = _batch(lib, w, h, frames)
    try:
        assert b.run(model) == 1
        outs = [b.download(i) for i in range(len(frames))]
        deb = None
        if qp is not None:
            b.deblock(qp)
            deb = [b.download(i)["rec"] for i in range(len(frames))]
        data, sizes = b.entropy_code(model)
        return outs, deb, _split(data, sizes)
    finally:
        b.close()


@pytest.fixture(scope="module")
def device(lib):
    """every fixture clip through the chain, once, by the SINGLE-model entry points (kvz_hip_intra_frames, kvz_hip_batch_deblock, kvz_hip_batch_entropy_code)"""
    out = {}
    for clip in sc.CLIPS:
        name, w, h, n, seed, kind, qp, preset, no_wpp = clip
        model = sc.table(lib, [qp], **sc.switches(clip)).models[0]
        assert model.signhide == 1
        out[name] = _chain(lib, model, w, h, sc.clip_frames(clip), qp)
    return out


@pytest.mark.parametrize("clip", sc.CLIPS, ids=lambda c: c[0])
def test_device_pass_reproduces_the_reference_encoder_and_the_host_simulation(lib, sim, gold, device, clip):
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    outs, deb, coded = device[name]
    assert [sc.sha(o["rec"]) for o in outs] == gold[name]["rec"]
    assert [mg.cu_digest(o["depth"].reshape(h // 8, w // 8), o["mode"].reshape(h // 8, w // 8)) for o in outs] == gold[name]["cu"]
    want = sc.sim_pass(sim, sc.table(lib, [qp] * n, **sc.switches(clip)), w, h, sc.clip_frames(clip))
    bad = [(i, cc.compare(o, s)) for i, (o, s) in enumerate(zip(outs, want)) if cc.compare(o, s)]  # rec, levels, depth, mode, CTU costs
    assert not bad, bad


@pytest.mark.parametrize("clip", sc.CLIPS, ids=lambda c: c[0])
def test_device_chain_reproduces_the_reference_slice_data(gold, device, clip):
    """pass -> deblocking -> entropy coder, all on the device: the slice data and the entry-point sizes are the reference bitstream's (one of the clips without WPP)"""
    name = clip[0]
    outs, deb, coded = device[name]
    if "deblock" in gold[name]:
        assert [sc.sha(d) for d in deb] == gold[name]["deblock"]
    for i, (data, sizes) in enumerate(coded):
        assert sizes == gold[name]["entropy"][i]["sizes"], i
        assert sc.sha(np.frombuffer(data, np.uint8)) == gold[name]["entropy"][i]["sha"], i


def test_mixed_launch_gives_every_picture_its_uniform_batch_result(lib, gold):
    """with and without the switch, QP 27 and QP 37 (the fast estimate and the CABAC coefficient cost), in ONE launch through PictureModels: every picture's outputs
    and slice data equal those of a uniform batch, the hidden ones are the fixture's and the plain ones the EXISTING goldens"""
    w, h, n, seed, kind = 200, 136, 2, 3, "small"
    p = cc.yuv_frames(w, h, n, seed, kind)
    qps, hide, pic = [27, 37, 27, 37, 37, 27], [1, 0, 0, 1, 1, 0], [0, 0, 1, 1, 0, 0]
    pm = sc.table(lib, qps, signhide=hide)
    assert pm.struct.n_models == 4
    outs, _, coded = _chain(lib, pm, w, h, [p[i] for i in pic])
    uniform = {}
    for q, s in sorted(set(zip(qps, hide))):
        uniform[q, s] = _chain(lib, sc.table(lib, [q], signhide=s).models[0], w, h, p)
    for i, (q, s, k) in enumerate(zip(qps, hide, pic)):
        assert not cc.compare(outs[i], uniform[q, s][0][k]), (i, q, s)
        assert coded[i] == uniform[q, s][2][k], (i, q, s)
        name = f"ultrafast-200x136-qp{q}"
        assert sc.sha(outs[i]["rec"]) == (gold[name]["rec"][k] if s else RECON[mg.clip_key(w, h, n, seed, kind, q, 0)][k]), (i, q, s)
        if s:
            assert coded[i][1] == gold[name]["entropy"][k]["sizes"] and sc.sha(np.frombuffer(coded[i][0], np.uint8)) == gold[name]["entropy"][k]["sha"], i
        elif q == 27:  # entropy.json has this clip at QP 27
            assert coded[i][1] == ENTROPY["partial-ctus-qp27"][k]["sizes"] and sc.sha(np.frombuffer(coded[i][0], np.uint8)) == ENTROPY["partial-ctus-qp27"][k]["sha"], i


def test_refusals_leave_the_batch_usable(lib, gold, capfd):
    """signhide with rdoq, with search_nxn, and under KVZ_HIP_SCHED=wave: -1 before anything is queued; the launch that follows on the same batch is correct"""
    clip = sc.CLIPS[0]
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    frames = sc.clip_frames(clip)
    good = sc.table(lib, [qp], signhide=1).models[0]

    def check(b):
        assert b.run(good) == 1
        assert [sc.sha(b.download(i)["rec"]) for i in range(n)] == gold[name]["rec"]
    b = _batch(lib, w, h, frames)
    try:
        for sw in (dict(rdoq=1, coeff_cabac=1, search_32x32=1), dict(search_nxn=1, coeff_cabac=1, search_32x32=1)):
            assert b.launch(sc.table(lib, [qp], signhide=1, **sw).models[0]) == -1
            assert b.launch(sc.table(lib, [qp] * n, signhide=[1, 0], **sw)) == -1
            assert "signhide together with" in capfd.readouterr().err
            b.sync()
            check(b)
    finally:
        b.close()
    old = os.environ.get("KVZ_HIP_SCHED")
    os.environ["KVZ_HIP_SCHED"] = "wave"  # read when a batch is created
    try:
        b = _batch(lib, w, h, frames)
    finally:
        if old is None:
            del os.environ["KVZ_HIP_SCHED"]
        else:
            os.environ["KVZ_HIP_SCHED"] = old
    try:
        assert b.launch(good) == -1
        assert "ticket schedule" in capfd.readouterr().err
        plain = sc.table(lib, [qp]).models[0]  # the schedule itself works: the picture without the switch
        assert b.run(plain) >= 1
        assert [sc.sha(b.download(i)["rec"]) for i in range(n)] == RECON[mg.clip_key(w, h, n, seed, kind, qp, 0)]
    finally:
        b.close()
