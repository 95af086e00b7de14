"""Per-coefficient scaling lists in the inter CTU pass (kvz_hip_dev_inter_ctu_pass_lists, InterPictures.set_scaling_lists; kvazaar's --scaling-list on B pictures) on
the MI355X: the LISTS builds of the inter kernel, and the loop filters and the B-slice coder behind them, against the reference encoder run with --gop lp-g4d3t1
--scaling-list default (tests/golden/inter_scaling_lists.json) and, output by output, against the host simulation of the same sources
(tests/hostsim/hostsim_inter_lists.cpp) -- also for a custom set, for which no encoder-level truth exists.  That a launch without lists computes what it computed is
what the existing GPU tests show."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import inter_common as ic
import inter_lists_common as ilc
import scaling_lists_common as slc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FLAT_GOLDEN = json.load(open(os.path.join(HERE, "golden", "inter_recon.json")))


@pytest.fixture(scope="module")
def lib():
    import kvazaar_amd
    return kvazaar_amd.load_library()


@pytest.fixture(scope="module")
def sim():
    return ilc.load_sim()


@pytest.fixture(scope="module")
def gold():
    return ilc.fixture()


@pytest.fixture(scope="module")
def flat_pan(oracle):
    """the `pan` clip encoded WITHOUT lists by the oracle: inputs of launches that need no chain (a B picture from the flat previous picture)"""
    clip = ilc.clip_named("pan")
    name, w, h, n, qp, preset, dbk, sao, owf, _ = clip
    frames = ic.case_frames(clip)
    rs, rf, cu, qps = ic.oracle_encode(oracle, w, h, frames, qp, preset=preset, deblock=bool(dbk), sao=bool(sao), mv_constraint=owf > 0)
    for a in (rs, rf, cu):
        a.setflags(write=False)
    return dict(clip=clip, frames=frames, rs=rs, rf=rf, cu=cu, qps=[int(q) for q in qps], w=w, h=h)


def _picture(seq, k):
    return dict(src=seq["frames"][k], ref=seq["rf"][k - 1], ref_cu=seq["cu"][k - 1])


def _launch(lib, pics, w, h):
    """the pictures resident on the device, the levels' buffer zeroed (a CTU that reaches beyond the picture is not written whole)"""
    from kvazaar_amd import inter
    ip = inter.InterPictures(lib, w, h, len(pics), with_levels=True)
    for i, p in enumerate(pics):
        ip.upload(i, p["src"], p["ref"], np.ascontiguousarray(p["ref_cu"]).reshape(-1))
    ip.dev.copy_in(ip.d_coeff, np.zeros(len(pics) * ip.ctus * 6144, np.int16))
    return ip


def _outputs(ip):
    """-> (rec [n, fs], cu [n, h/4, w/4], levels [n, ctus * 6144]) of the last pass"""
    rec, cu = zip(*[ip.download(i) for i in range(ip.n)])
    return np.stack(rec), np.stack(cu), ip.dev.get(ip.d_coeff, (ip.n, ip.ctus * 6144), np.int16)


def _device_pass(lib, pics, prm, pictures, sets, index, w, h):
    ip = _launch(lib, pics, w, h)
    try:
        if sets:
            ip.set_scaling_lists(sets, index)
        ip.run(prm, pictures=pictures)
        return _outputs(ip)
    finally:
        ip.close()


def _assert_equal(got, want, where):
    """device outputs == simulation outputs: samples, CU decisions, levels"""
    rec, cu, coeff = got
    assert ic.first_difference(cu, want[1]) is None, where
    assert np.array_equal(rec, want[0]), where
    assert np.array_equal(coeff, want[2]), where


# ---------------------------------------------------------------------------------------------------- 1. the chain against the reference encoder
@pytest.mark.parametrize("name", [c[0] for c in ilc.CLIPS])
def test_device_chain_equals_the_reference_encoder(lib, gold, name):
    """picture 0 from HipBatch with set_scaling_lists and its loop filters; every B picture through InterPictures with set_scaling_lists from the device's own previous
    picture: pass, loop_filters, entropy_code, advance == kvazaar --gop lp-g4d3t1 --scaling-list default: every final picture, every CU decision, and the slice data of
    the pinned clip"""
    import ctu_common as cc
    from kvazaar_amd import inter
    clip, g = ilc.clip_named(name), gold[name]
    _, w, h, n, base_qp, preset, dbk, sao, owf, _ = clip
    frames, qps, lists = ic.case_frames(clip), ilc.picture_qps(clip), slc.lists("default")
    assert qps == g["qps"]
    model = slc.table(lib, [qps[0]], coeff_cabac=int(ilc.prices_with_cabac(clip, qps[0]))).models[0]
    b = cc.HipBatch(lib, w, h, 1)
    try:
        b.upload(0, frames[0])
        b.set_scaling_lists([lists])
        assert b.run(model) == 1
        o = b.download(0)
        b.loop_filters(model, deblock=bool(dbk), sao=bool(sao))
        final = b.download(0)["rec"]
    finally:
        b.close()
    cu = ilc.intra_cu_records(o["depth"], o["mode"], w, h)
    assert ilc.sha(final) == g["rec"][0] and inter.cu_digest(cu) == g["cu"][0], (name, 0)
    ip = inter.InterPictures(lib, w, h, 1, with_levels=True)
    try:
        ip.set_scaling_lists([lists])
        ip.upload(0, frames[1], final, cu.reshape(-1))
        for k in range(1, n):
            if k > 1:
                ip.advance()
                ip.upload_source(0, frames[k])
            prm = ilc.params_of(clip, qps[k], k)
            ip.run(prm)
            ip.loop_filters(prm)
            rec, got_cu = ip.download(0)
            assert ilc.sha(rec) == g["rec"][k] and inter.cu_digest(got_cu) == g["cu"][k], (name, k)
            if name == ilc.PINNED:
                data, sizes = ip.entropy_code(prm)
                assert [int(v) for v in sizes[0]] == g["entropy"][k]["sizes"] and ilc.sha(np.frombuffer(bytes(data), np.uint8)) == g["entropy"][k]["sha"], (name, k)
    finally:
        ip.close()


# ---------------------------------------------------------------------------------------------------- 2. the device against the simulation
@pytest.mark.parametrize("build,qp", [("lists fast", 25), ("lists cabac", 30)])
def test_device_equals_the_simulation_under_both_sets_in_both_builds(lib, sim, flat_pan, build, qp, monkeypatch, capfd):
    """two B pictures of the pan clip, one under the default lists and one under the custom set, in one launch: picture QP below fast-residual-cost 28 (the
    `_lists_fast` build) and above (`_lists_cabac`); samples, CU records and levels are the simulation's"""
    s, clip = flat_pan, flat_pan["clip"]
    sets, index, pics = [slc.lists("default"), slc.lists("custom")], [0, 1, 1, 0], [_picture(s, 1), _picture(s, 1), _picture(s, 2), _picture(s, 3)]
    from kvazaar_amd.inter import InterPictureParams
    table = InterPictureParams([qp] * 4, [1, 1, 2, 3])
    monkeypatch.setenv("KVZ_HIP_INTER_VERBOSE", "1")
    capfd.readouterr()
    got = _device_pass(lib, pics, ilc.params_of(clip, 45, 9), table, sets, index, s["w"], s["h"])
    assert f"{build} build" in capfd.readouterr().err
    rc, *want = ilc.sim_pass(sim, pics, ilc.params_of(clip, 45, 9), table, sets, index, s["w"], s["h"])
    assert rc == 0
    _assert_equal(got, want, build)
    assert not np.array_equal(got[2][0], got[2][1])  # the two sets give different levels for the same picture


@pytest.mark.parametrize("qp", [44, 51])
def test_noise_at_the_left_side_qps_equals_the_simulation(lib, sim, oracle, qp):
    """uniform noise handed to the pass at QP 44 (16x16 on the clip-and-shift-left side of the dequantiser) and 51 (every size), `veryfast` and `ultrafast`, under
    both sets in one launch; the reference picture comes from the flat oracle encode"""
    w, h = 136, 72
    frames = ic.hard_clip("noise", w, h, 2, 60 + qp, (3.0, -2.0))
    rs, rf, cu, _ = ic.oracle_encode(oracle, w, h, frames, 22, preset="veryfast", deblock=True, sao=True)
    pics, sets = [dict(src=frames[1], ref=rf[0], ref_cu=cu[0])] * 2, [slc.lists("default"), slc.lists("custom")]
    for name in ("pan", "ultrafast-8mod16"):
        prm = ilc.params_of(ilc.clip_named(name), qp, 1)
        got = _device_pass(lib, pics, prm, None, sets, [0, 1], w, h)
        rc, *want = ilc.sim_pass(sim, pics, prm, None, sets, [0, 1], w, h)
        assert rc == 0 and np.count_nonzero(want[2]) > 100
        _assert_equal(got, want, (qp, name))


def test_mixed_launch_equals_every_picture_alone(lib, sim, flat_pan):
    """six pictures at three QPs, two POCs and the sets default / custom / 0xffff in one launch through InterPictureParams + set_of_picture: each picture equals its
    launch alone, the flat ones equal a launch without sets, and the launch is the simulation's"""
    from kvazaar_amd.inter import InterPictureParams
    s, clip = flat_pan, flat_pan["clip"]
    sets = [slc.lists("default"), slc.lists("custom")]
    mixed = [(1, 25, 0), (2, 30, 1), (1, 36, ilc.FLAT), (2, 25, 1), (1, 30, ilc.FLAT), (2, 36, 0)]  # (picture of the clip = POC, QP, set)
    pics = [_picture(s, k) for k, _, _ in mixed]
    table, index = InterPictureParams([q for _, q, _ in mixed], [k for k, _, _ in mixed]), [st for _, _, st in mixed]
    got = _device_pass(lib, pics, ilc.params_of(clip, 45, 9), table, sets, index, s["w"], s["h"])
    rc, *want = ilc.sim_pass(sim, pics, ilc.params_of(clip, 45, 9), table, sets, index, s["w"], s["h"])
    assert rc == 0
    _assert_equal(got, want, "mixed")
    for i, (k, qp, st) in enumerate(mixed):
        alone = _device_pass(lib, [pics[i]], ilc.params_of(clip, qp, k), None, [] if st == ilc.FLAT else [sets[st]], None, s["w"], s["h"])
        assert all(np.array_equal(a[0], b[i]) for a, b in zip(alone, got)), (i, k, qp, st)


def test_clear_restores_the_flat_goldens_and_refusals_leave_the_object_usable(lib, flat_pan, gold, capfd):
    """one InterPictures object through: lists -> a refused launch (entry 12; a set index past the table) -> the next launch is right -> clear_scaling_lists -> the flat
    goldens of tests/golden/inter_recon.json (the reference encoder without lists) again"""
    from kvazaar_amd import inter
    s, clip = flat_pan, flat_pan["clip"]
    k = 1
    prm = ilc.params_of(clip, s["qps"][k], k)
    ip = _launch(lib, [_picture(s, k)], s["w"], s["h"])
    try:
        ip.set_scaling_lists([slc.lists("default")])
        ip.run(prm)
        with_lists = _outputs(ip)
        assert not np.array_equal(with_lists[0][0], s["rs"][k])
        bad = slc.lists("default")
        bad.struct.coeff[1][3][5] = 12
        ip.set_scaling_lists([bad])
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            ip.run(prm)
        assert "13 .. 255" in capfd.readouterr().err
        ip.set_scaling_lists([slc.lists("default")], [1])
        with pytest.raises(RuntimeError):
            ip.run(prm)
        assert "set_of_picture" in capfd.readouterr().err
        wrong_size = slc.lists("default")
        wrong_size.struct.struct_size += 4
        ip.set_scaling_lists([wrong_size])
        with pytest.raises(RuntimeError):
            ip.run(prm)
        assert "struct_size" in capfd.readouterr().err
        ip.set_scaling_lists([slc.lists("default")])
        ip.run(prm)
        again = _outputs(ip)
        assert all(np.array_equal(a, b) for a, b in zip(again, with_lists))
        ip.clear_scaling_lists()
        ip.run(prm)
        rec, cu = ip.download(0)
        assert np.array_equal(rec, s["rs"][k])
        ip.loop_filters(prm)
        rec, cu = ip.download(0)
        assert ilc.sha(rec) == FLAT_GOLDEN["pan"]["rec"][k] and inter.cu_digest(cu) == FLAT_GOLDEN["pan"]["cu"][k]
        assert ilc.sha(rec) != gold["pan"]["rec"][k]
    finally:
        ip.close()


def test_random_cases_equal_the_host_simulation(lib, sim, oracle):
    """16 seeded pictures of at most 136x136 in four launches: per launch a geometry, a preset and four pictures, each with its own content, QP, POC and set (default,
    custom or none); the reference pictures are flat I pictures from the oracle"""
    from kvazaar_amd.inter import InterPictureParams
    rng = np.random.default_rng(20261020)
    sets = [slc.lists("default"), slc.lists("custom")]
    for launch in range(4):
        w, h = int(rng.integers(1, 18)) * 8, int(rng.integers(1, 18)) * 8
        preset = ("veryfast", "faster", "ultrafast", "veryfast")[launch]
        kinds = [k for k in ic.FUZZ_CONTENT if k != "motion" or (w > 40 and h > 40)]
        pics, qps, pocs, index = [], [], [], []
        for _ in range(4):
            c = dict(w=w, h=h, n=2, kind=kinds[int(rng.integers(0, len(kinds)))], seed=int(rng.integers(1, 1 << 30)), noise=float(rng.uniform(0, 3)),
                     pan=(float(rng.uniform(-4, 4)), float(rng.uniform(-4, 4))))
            frames = ic.fuzz_frames(c)
            rs, rf, cu, _ = ic.oracle_encode(oracle, w, h, frames[:1], int(rng.integers(10, 40)), preset=preset, deblock=True, sao=None)
            pics.append(dict(src=frames[1], ref=rf[0], ref_cu=cu[0]))
            qps.append(int(rng.integers(0, 52)))
            pocs.append(int(rng.integers(1, 4)))
            index.append((0, 1, ilc.FLAT)[int(rng.integers(0, 3))])
        clip = ("random", w, h, 2, 22, preset, 1, ic.PRESETS[preset]["sao"], 0, None)
        table = InterPictureParams(qps, pocs)
        got = _device_pass(lib, pics, ilc.params_of(clip, 45, 9), table, sets, index, w, h)
        rc, *want = ilc.sim_pass(sim, pics, ilc.params_of(clip, 45, 9), table, sets, index, w, h)
        assert rc == 0
        _assert_equal(got, want, (launch, w, h, preset, qps, pocs, index))
