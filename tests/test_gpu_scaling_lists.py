"""Per-coefficient scaling lists (kvz_hip_batch_set_scaling_lists, kvazaar's --scaling-list) on the MI355X: the LISTS instantiations of the CTU pass, and the loop
filters and the entropy coder behind them, against the reference encoder run with --scaling-list default (tests/golden/scaling_lists.json) and, output by output,
against the host simulation of the same sources (tests/hostsim/hostsim_scaling_lists.cpp) -- also for a custom set, for which no encoder-level truth exists.
That a batch without lists computes what it computed is what the existing GPU tests show."""
import json
import os
import sys

import numpy as np
import pytest

import ctu_common as cc
import inter_common as ic
import scaling_lists_common as slc
from kvazaar_amd.batch import BatchError

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as mg  # noqa: E402

RECON = json.load(open(os.path.join(HERE, "golden", "encoder_recon.json")))


@pytest.fixture(scope="module")
def lib():
    import kvazaar_amd
    return kvazaar_amd.load_library()


@pytest.fixture(scope="module")
def sim():
    return slc.load_sim()


@pytest.fixture(scope="module")
def gold():
    return slc.fixture()


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


def _run(lib, model, sets, index, w, h, frames):
    """one pass on a fresh batch that was given `sets` / `index` (no sets: a batch without lists) -> the outputs per picture"""
    b = _batch(lib, w, h, frames)
    try:
        if sets:
            b.set_scaling_lists(sets, index)
        assert b.run(model) == 1
        return [b.download(i) for i in range(len(frames))]
    finally:
        b.close()


def _model(lib, clip):
    return slc.table(lib, [clip[6]], **slc.switches(clip)).models[0]


@pytest.fixture(scope="module")
def device(lib):
    """every fixture clip under the default lists AND under the custom set in ONE launch each (the clip's pictures twice; the single-model entry point)"""
    out = {}
    for clip in slc.CLIPS:
        name, w, h, n, seed, kind, qp, preset, no_wpp = clip
        frames = slc.clip_frames(clip)
        outs = _run(lib, _model(lib, clip), [slc.lists("default"), slc.lists("custom")], [0] * n + [1] * n, w, h, frames + frames)
        out[name] = (outs[:n], outs[n:])
    return out


@pytest.mark.parametrize("clip", slc.CLIPS, ids=lambda c: c[0])
def test_device_pass_reproduces_the_reference_encoder(gold, device, clip):
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    outs = device[name][0]
    assert [slc.sha(o["rec"]) for o in outs] == gold[name]["rec"]
    assert [mg.cu_digest(o["depth"].reshape(h // 8, w // 8), o["mode"].reshape(h // 8, w // 8)) for o in outs] == gold[name]["cu"]
    assert slc.coverage(outs, w, h, qp) == gold[name]["coverage"]  # the levels land where the simulation's did, transform size by transform size


@pytest.mark.parametrize("clip", slc.CLIPS, ids=lambda c: c[0])
def test_device_equals_the_host_simulation_for_both_sets(lib, sim, device, clip):
    """rec, levels, depth, mode and CTU costs of every picture, under the default lists and under the custom set (its own DC terms, every entry different)"""
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    pm = slc.table(lib, [qp] * n, **slc.switches(clip))
    for k, set_name in enumerate(("default", "custom")):
        want = slc.sim_pass(sim, pm, [slc.lists(set_name)], None, w, h, slc.clip_frames(clip))
        bad = [(set_name, i, cc.compare(o, s)) for i, (o, s) in enumerate(zip(device[name][k], want)) if cc.compare(o, s)]
        assert not bad, bad
    assert [slc.sha(o["rec"]) for o in device[name][0]] != [slc.sha(o["rec"]) for o in device[name][1]]


def test_device_chain_reproduces_the_reference_deblocking_and_slice_data(lib, gold):
    """pass -> kvz_hip_batch_loop_filters (deblocking) -> kvz_hip_batch_entropy_code on the pinned clip: the reference's deblocked pictures and its bitstream's slice data"""
    clip = [c for c in slc.CLIPS if c[0] == slc.PINNED][0]
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    model = _model(lib, clip)
    b = _batch(lib, w, h, slc.clip_frames(clip))
    try:
        b.set_scaling_lists([slc.lists("default")])
        assert b.run(model) == 1
        b.loop_filters(model, deblock=True, sao=False)
        assert [slc.sha(b.download(i)["rec"]) for i in range(n)] == gold[name]["deblock"]
        data, sizes = b.entropy_code(model)
        for i, (bytes_, row) in enumerate(_split(data, sizes)):
            assert row == gold[name]["entropy"][i]["sizes"], i
            assert slc.sha(np.frombuffer(bytes_, np.uint8)) == gold[name]["entropy"][i]["sha"], i
    finally:
        b.close()


def test_mixed_launch_gives_every_picture_its_uniform_result(lib, gold):
    """six 200x136 pictures at QPs 22, 27 and 37 under the default set, the custom set or no lists, in ONE launch through PictureModels: each equals its launch
    alone, the flat ones a launch on a batch WITHOUT lists and the existing goldens, the default one the fixture.  The launch mixes the two coefficient cost models:
    kvz_hip_intra_cost_model_init sets coeff_cabac for QP >= 28 (`ultrafast`), asserted below, so the QP 22 / 27 pictures are priced by the fast estimate through the
    run-time switch of the CABAC instantiation while their launches alone take the other one"""
    frames, pm, sets, index = slc.mixed_batch(lib)
    assert [int(pm.model_of(k).coeff_cabac) for k in range(6)] == [0, 0, 0, 0, 1, 1]
    outs = _run(lib, pm, sets, index, 200, 136, frames)
    for k, (i, qp, s) in enumerate(slc.MIXED):
        alone = _run(lib, slc.table(lib, [qp]).models[0], [] if s == slc.FLAT else [sets[s]], None, 200, 136, [frames[k]])[0]
        assert not cc.compare(outs[k], alone), (k, qp, s)
        if s == slc.FLAT:
            assert slc.sha(outs[k]["rec"]) == RECON[mg.clip_key(200, 136, 2, 3, "small", qp, 0)][i]
    assert slc.sha(outs[3]["rec"]) == gold["ultrafast-200x136-qp27"]["rec"][1]


def test_fast_estimate_with_searched_32x32_cus_equals_the_host_simulation(lib, sim):
    """search_32x32 WITHOUT the CABAC coefficient cost below QP 28 (kvazaar: --pu-depth-intra 1-3 at `ultrafast`): the one LISTS instantiation no preset reaches,
    intra_ctu_ticket_kernel_lists<false, true>.  The 200x136 clip at QP 22 under the default set, the custom set and no lists in one launch"""
    w, h = 200, 136
    p = cc.yuv_frames(w, h, 2, 3, "small")
    frames, index = [p[0], p[1], p[0], p[1]], [0, 1, slc.FLAT, 0]
    pm = slc.table(lib, [22] * 4, search_32x32=1)
    assert all(pm.model_of(i).search_32x32 == 1 and pm.model_of(i).coeff_cabac == 0 for i in range(4))  # what selects that kernel
    sets = [slc.lists("default"), slc.lists("custom")]
    got, want = _run(lib, pm, sets, index, w, h, frames), slc.sim_pass(sim, pm, sets, index, w, h, frames)
    bad = [(i, cc.compare(o, s)) for i, (o, s) in enumerate(zip(got, want)) if cc.compare(o, s)]
    assert not bad, bad
    assert 1 in {int(v) for o in got for v in np.unique(o["depth"])}  # 32x32 CUs do occur
    flat = _run(lib, pm.model_of(0), [], None, w, h, [p[0]])[0]  # ... and the flat picture is the one of a batch without lists (the existing <false, true> kernel)
    assert not cc.compare(got[2], flat)
    assert slc.sha(got[0]["rec"]) != slc.sha(flat["rec"])


def test_random_cases_equal_the_host_simulation(lib, sim):
    """16 seeded pictures of at most 136x136 in four launches: per launch a geometry, a preset and four pictures, each with its own content, QP and set (default,
    custom or none)"""
    rng = np.random.default_rng(20261019)
    sets = [slc.lists("default"), slc.lists("custom")]
    for launch in range(4):
        w, h = int(rng.integers(1, 18)) * 8, int(rng.integers(1, 18)) * 8
        preset = ("ultrafast", "faster", "fast", "ultrafast")[launch]
        kinds = [k for k in ic.FUZZ_CONTENT if k != "motion" or (w > 40 and h > 40)]
        frames, qps, index = [], [], []
        for _ in range(4):
            c = dict(w=w, h=h, n=1, kind=kinds[int(rng.integers(0, len(kinds)))], seed=int(rng.integers(1, 1 << 30)), noise=float(rng.uniform(0, 3)), pan=(0.0, 0.0))
            frames += ic.fuzz_frames(c)
            qps.append(int(rng.integers(0, 52)))
            index.append((0, 1, slc.FLAT)[int(rng.integers(0, 3))])
        pm = slc.table(lib, qps, **slc.PRESETS[preset])
        got, want = _run(lib, pm, sets, index, w, h, frames), slc.sim_pass(sim, pm, sets, index, w, h, frames)
        bad = [(launch, w, h, preset, qps[i], index[i], cc.compare(o, s)) for i, (o, s) in enumerate(zip(got, want)) if cc.compare(o, s)]
        assert not bad, bad


def test_refusals_leave_the_batch_usable_and_clear_restores_it(lib, gold, capfd):
    """a refused set_scaling_lists keeps the previous state, a refused launch queues nothing: the next launch on the same batch is right; after clear_scaling_lists
    the batch gives the flat goldens again (and takes the models it refused)"""
    clip = slc.CLIPS[0]
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    model = _model(lib, clip)
    flat = RECON[mg.clip_key(w, h, n, seed, kind, qp, 0)]
    b = _batch(lib, w, h, slc.clip_frames(clip))
    try:
        assert b.run(model) == 1 and [slc.sha(b.download(i)["rec"]) for i in range(n)] == flat  # before any lists
        b.set_scaling_lists([slc.lists("default")])
        bad = slc.lists("default")
        bad.struct.coeff[1][0][5] = 12
        with pytest.raises(BatchError):
            b.set_scaling_lists([bad])
        assert "13 .. 255" in capfd.readouterr().err
        with pytest.raises(BatchError):
            b.set_scaling_lists([slc.lists("default")], [0, 1])
        assert "set_of_picture" in capfd.readouterr().err
        for sw in (dict(rdoq=1, coeff_cabac=1, search_32x32=1), dict(search_nxn=1, coeff_cabac=1, search_32x32=1), dict(signhide=1)):
            assert b.launch(slc.table(lib, [qp], **sw).models[0]) == -1
            assert "scaling lists" in capfd.readouterr().err
            assert b.launch(slc.table(lib, [qp] * n, **sw)) == -1
            assert "scaling lists" in capfd.readouterr().err
        b.sync()
        assert b.run(model) == 1 and [slc.sha(b.download(i)["rec"]) for i in range(n)] == gold[name]["rec"]  # the state the refused calls left alone
        b.clear_scaling_lists()
        assert b.run(model) == 1 and [slc.sha(b.download(i)["rec"]) for i in range(n)] == flat
        assert b.run(slc.table(lib, [qp], signhide=1).models[0]) == 1  # no lists: nothing to refuse
        b.set_scaling_lists([slc.lists("custom"), slc.lists("default")], [1, slc.FLAT])  # ... and lists again, on the same batch
        assert b.run(model) == 1
        assert [slc.sha(b.download(i)["rec"]) for i in range(n)] == [gold[name]["rec"][0], flat[1]]
    finally:
        b.close()
    old = os.environ.get("KVZ_HIP_SCHED")
    os.environ["KVZ_HIP_SCHED"] = "wave"  # read when a batch is created
    try:
        b = _batch(lib, w, h, slc.clip_frames(clip))
    finally:
        if old is None:
            del os.environ["KVZ_HIP_SCHED"]
        else:
            os.environ["KVZ_HIP_SCHED"] = old
    try:
        with pytest.raises(BatchError):
            b.set_scaling_lists([slc.lists("default")])
        assert "ticket schedule" in capfd.readouterr().err
        assert b.run(model) >= 1 and [slc.sha(b.download(i)["rec"]) for i in range(n)] == flat  # the schedule itself works, without lists
    finally:
        b.close()
