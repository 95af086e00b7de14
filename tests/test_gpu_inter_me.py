"""The inter CTU pass's choice of integer motion search (kvz_hip_inter_params me_algorithm / me_max_steps / me_early_termination: kvazaar's --me, --me-steps,
--me-early-termination) on the MI355X: the ME builds of the inter kernel, and the loop filters and the B-slice coder behind them, against the reference encoder run
with the switches (tests/golden/inter_me.json) and, output by output, against the host simulation of the same sources (tests/hostsim/hostsim_inter_me.cpp)."""
import numpy as np
import pytest

import inter_common as ic
import inter_lists_common as ilc
import inter_me_common as mec
import scaling_lists_common as slc

pytestmark = pytest.mark.gpu

CHAINS = mec.cases()  # every case of the fixture runs as a whole chain on the device


@pytest.fixture(scope="module")
def lib():
    import kvazaar_amd
    return kvazaar_amd.load_library()


@pytest.fixture(scope="module")
def sim():
    return mec.load_sim()


@pytest.fixture(scope="module")
def gold():
    return mec.fixture()


@pytest.fixture(scope="module")
def seq(oracle):
    """the small clip encoded by the oracle with the default search: inputs of launches that need no chain (a B picture from the previous final picture)"""
    clip = mec.clip_named(mec.DEVICE_CLIP)
    name, w, h, n, qp, preset, dbk, sao, owf, _ = clip
    frames = ic.case_frames(clip)
    rs, rf, cu, qps = ic.oracle_encode(oracle, w, h, frames, qp, preset=preset, deblock=bool(dbk), sao=bool(sao), mv_constraint=owf > 0)
    for a in (rs, rf, cu):
        a.setflags(write=False)
    return dict(clip=clip, frames=frames, rs=rs, rf=rf, cu=cu, qps=[int(q) for q in qps], w=w, h=h)


def _picture(s, k):
    return dict(src=s["frames"][k], ref=s["rf"][k - 1], ref_cu=s["cu"][k - 1])


def _launch(lib, pics, w, h):
    """the pictures resident on the device, the levels' buffer zeroed (a CTU that reaches beyond the picture is not written whole)"""
    from kvazaar_amd import inter
    ip = inter.InterPictures(lib, w, h, len(pics), with_levels=True)
    for i, p in enumerate(pics):
        ip.upload(i, p["src"], p["ref"], np.ascontiguousarray(p["ref_cu"]).reshape(-1))
    ip.dev.copy_in(ip.d_coeff, np.zeros(len(pics) * ip.ctus * 6144, np.int16))
    return ip


def _outputs(ip):
    rec, cu = zip(*[ip.download(i) for i in range(ip.n)])
    return np.stack(rec), np.stack(cu), ip.dev.get(ip.d_coeff, (ip.n, ip.ctus * 6144), np.int16)


def _device_pass(lib, pics, prm, pictures, w, h):
    ip = _launch(lib, pics, w, h)
    try:
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


# ---------------------------------------------------------------------------------------------------- 1. the device against the simulation
@pytest.mark.parametrize("build,qp", [("me fast", 23), ("me cabac", 30)])
@pytest.mark.parametrize("option", [o for o in mec.ALL if o != "hexbs"] + ["full"])
def test_device_equals_the_simulation(lib, sim, seq, option, build, qp, monkeypatch, capfd):
    """the two B pictures of the small clip in one launch under every option: picture QP below fast-residual-cost 28 (the `_me_fast` build) and above (`_me_cabac`);
    samples, CU records and levels are the simulation's"""
    from kvazaar_amd.inter import InterPictureParams
    s, clip = seq, seq["clip"]
    pics, table = [_picture(s, 1), _picture(s, 2)], InterPictureParams([qp, qp], [1, 2])
    prm = mec.params_of(clip, 45, 9, "full32" if option == "full" else option)
    if option == "full":
        prm.me_algorithm = 2
    monkeypatch.setenv("KVZ_HIP_INTER_VERBOSE", "1")
    capfd.readouterr()
    got = _device_pass(lib, pics, prm, table, s["w"], s["h"])
    assert f"{build} build" in capfd.readouterr().err
    rc, *want = mec.sim_pass(sim, pics, prm, table, s["w"], s["h"])
    assert rc == 0
    _assert_equal(got, want, (option, build))


# ---------------------------------------------------------------------------------------------------- 2. the chain against the reference encoder
_first = {}


def _first_picture(lib, clip):
    """picture 0 of the clip from HipBatch and its loop filters -> (final picture, CU records), once per clip"""
    import ctu_common as cc
    name, w, h, n, base_qp, preset, dbk, sao, owf, _ = clip
    if name not in _first:
        frames, qps = ic.case_frames(clip), ilc.picture_qps(clip)
        model = slc.table(lib, [qps[0]], coeff_cabac=int(ilc.prices_with_cabac(clip, qps[0]))).models[0]
        b = cc.HipBatch(lib, w, h, 1)
        try:
            b.upload(0, frames[0])
            assert b.run(model) == 1
            o = b.download(0)
            b.loop_filters(model, deblock=bool(dbk), sao=bool(sao))
            final = b.download(0)["rec"]
        finally:
            b.close()
        _first[name] = (frames, qps, final, ilc.intra_cu_records(o["depth"], o["mode"], w, h))
    return _first[name]


@pytest.mark.parametrize("clip_name,option", CHAINS, ids=[mec.key(*c) for c in CHAINS])
def test_device_chain_equals_the_reference_encoder(lib, gold, clip_name, option):
    """picture 0 from HipBatch and its loop filters; every B picture through InterPictures from the device's own previous picture: pass, loop_filters, entropy_code,
    advance == kvazaar --gop lp-g4d3t1 with the option's switches: every final picture and the slice data of every B picture"""
    from kvazaar_amd import inter
    clip, g = mec.clip_named(clip_name), gold[mec.key(clip_name, option)]
    _, w, h, n, base_qp, preset, dbk, sao, owf, _ = clip
    frames, qps, final, cu = _first_picture(lib, clip)
    assert qps == g["qps"] and ilc.sha(final) == g["rec"][0]
    ip = inter.InterPictures(lib, w, h, 1, with_levels=True)
    try:
        ip.upload(0, frames[1], final, cu.reshape(-1))
        for k in range(1, n):
            if k > 1:
                ip.advance()
                ip.upload_source(0, frames[k])
            prm = mec.params_of(clip, qps[k], k, option)
            ip.run(prm)
            ip.loop_filters(prm)
            rec, _ = ip.download(0)
            assert ilc.sha(rec) == g["rec"][k], (clip_name, option, k)
            data, sizes = ip.entropy_code(prm)
            assert [int(v) for v in sizes[0]] == g["slices"][k]["sizes"] and ilc.sha(np.frombuffer(bytes(data), np.uint8)) == g["slices"][k]["sha"], (clip_name, option, k)
    finally:
        ip.close()


# ---------------------------------------------------------------------------------------------------- 3. mixed launches, zero members
def test_pictures_at_different_qps_and_pocs_share_a_launch_under_tz(lib, sim, seq):
    """four pictures at three QPs (both sides of fast-residual-cost: the launch takes the `_me_cabac` build, some pictures price with the fast estimate) and two
    POCs through InterPictureParams: the launch is the simulation's, and each picture equals its launch alone"""
    from kvazaar_amd.inter import InterPictureParams
    s, clip = seq, seq["clip"]
    mixed = [(1, 23), (2, 30), (1, 36), (2, 23)]  # (picture of the clip = POC, QP)
    pics, table = [_picture(s, k) for k, _ in mixed], InterPictureParams([q for _, q in mixed], [k for k, _ in mixed])
    prm = mec.params_of(clip, 45, 9, "tz")
    got = _device_pass(lib, pics, prm, table, s["w"], s["h"])
    rc, *want = mec.sim_pass(sim, pics, prm, table, s["w"], s["h"])
    assert rc == 0
    _assert_equal(got, want, "mixed")
    for i, (k, qp) in enumerate(mixed):
        alone = _device_pass(lib, [pics[i]], mec.params_of(clip, qp, k, "tz"), None, s["w"], s["h"])
        assert all(np.array_equal(a[0], b[i]) for a, b in zip(alone, got)), (i, k, qp)


def test_zero_members_are_the_default_launch(lib, seq, monkeypatch, capfd):
    """three zero members: the default builds, and the bytes of the oracle's encode"""
    s, clip = seq, seq["clip"]
    monkeypatch.setenv("KVZ_HIP_INTER_VERBOSE", "1")
    for k in (1, 2):
        prm = mec.params_of(clip, s["qps"][k], k, "hexbs")
        capfd.readouterr()
        rec, cu, _ = _device_pass(lib, [_picture(s, k)], prm, None, s["w"], s["h"])
        err = capfd.readouterr().err
        assert "cabac build" in err and "me cabac" not in err and "me fast" not in err, err
        assert np.array_equal(rec[0], s["rs"][k]) and ic.first_difference(cu, s["cu"][k][None]) is None, k


def test_the_struct_from_before_the_members_is_still_taken(lib, seq):
    """struct_size 60 (the struct that ends with no_tmvp: a binding compiled before the three members): the pass, the loop filters and the coder take it, the
    members behind it are not read, and the launch is the default one"""
    from kvazaar_amd.inter import InterParams
    s, clip, k = seq, seq["clip"], 1
    old = mec.params_of(clip, s["qps"][k], k, "tz-et-off")
    old.struct_size = InterParams.me_algorithm.offset
    new = mec.params_of(clip, s["qps"][k], k, "hexbs")
    ip = _launch(lib, [_picture(s, k)], s["w"], s["h"])
    try:
        ip.run(old)
        assert np.array_equal(ip.download(0)[0], s["rs"][k])
        ip.loop_filters(old)
        data_old = bytes(ip.entropy_code(old)[0])
        ip.run(new)
        ip.loop_filters(new)
        assert data_old == bytes(ip.entropy_code(new)[0]) and len(data_old) > 0
        group_rc = __import__("kvazaar_amd").inter.InterGroup(lib, [ip]).run(old)
        assert group_rc == 0 and np.array_equal(ip.download(0)[0], s["rs"][k])
    finally:
        ip.close()


# ---------------------------------------------------------------------------------------------------- 4. what is refused
def test_refusals_leave_the_outputs_untouched_and_the_object_usable(lib, sim, seq, capfd):
    """one InterPictures object through every refusal -- a bad member, a member together with tiles, with scaling lists, in a joint launch -- with its outputs filled
    with a pattern: each returns -1 with a message before anything is queued, the pattern stands, and the next launch on the object is the simulation's"""
    from kvazaar_amd import inter
    s, clip = seq, seq["clip"]
    w, h, k = s["w"], s["h"], 1
    ip = _launch(lib, [_picture(s, k)], w, h)
    try:
        pattern = [np.full(ip.fs, 0xa5, np.uint8), np.full(ip.cells * inter.CU_DTYPE.itemsize, 0x5a, np.uint8), np.full(ip.ctus * 6144, 0x1234, np.int16)]

        def fill():
            for d, a in zip((ip.d_rec, ip.d_cu, ip.d_coeff), pattern):
                ip.dev.copy_in(d, a)

        def untouched():
            return (np.array_equal(ip.dev.get(ip.d_rec, (ip.fs,), np.uint8), pattern[0]) and np.array_equal(ip.dev.get(ip.d_cu, (pattern[1].size,), np.uint8), pattern[1])
                    and np.array_equal(ip.dev.get(ip.d_coeff, (ip.ctus * 6144,), np.int16), pattern[2]))

        def prm(option="hexbs", **kw):
            p = mec.params_of(clip, s["qps"][k], k, option)
            for name, v in kw.items():
                setattr(p, name, v)
            return p

        for p, message in ((prm(me_algorithm=8), "me_algorithm 8 outside 0..7"), (prm(me_algorithm=-1), "me_algorithm -1 outside 0..7"), (prm(me_max_steps=-1), "me_max_steps -1 is negative"),
                           (prm(me_early_termination=3), "me_early_termination 3 outside 0..2"), (prm("tz", ref_width=w, ref_height=h), "tiles"),
                           (prm("steps1", ref_width=w, ref_height=h, no_wpp=1, no_tmvp=1), "tiles")):
            fill()
            capfd.readouterr()
            with pytest.raises(RuntimeError, match="returned -1"):
                ip.run(p)
            assert message in capfd.readouterr().err and untouched(), message
        # ... together with scaling lists
        fill()
        ip.set_scaling_lists([slc.lists("default")])
        capfd.readouterr()
        with pytest.raises(RuntimeError, match="returned -1"):
            ip.run(prm("et-on"))
        assert "scaling lists" in capfd.readouterr().err and untouched()
        ip.clear_scaling_lists()
        # ... in a joint launch
        group = inter.InterGroup(lib, [ip])
        capfd.readouterr()
        assert group.run(prm("dia")) == -1
        assert "a joint launch" in capfd.readouterr().err and untouched()
        group.close()
        # the object still works: a chosen search, then the default one
        ip.dev.copy_in(ip.d_coeff, np.zeros(ip.ctus * 6144, np.int16))
        ip.run(prm("tz"))
        rc, *want = mec.sim_pass(sim, [_picture(s, k)], prm("tz"), None, w, h)
        assert rc == 0
        _assert_equal(_outputs(ip), want, "after the refusals")
        ip.run(prm())
        assert np.array_equal(ip.download(0)[0], s["rs"][k])
    finally:
        ip.close()
