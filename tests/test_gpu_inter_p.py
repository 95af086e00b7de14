"""P pictures (kvazaar's --no-bipred) on the MI355X: the P builds of the inter kernel (kvz_hip_dev_inter_ctu_pass_slices with KVZ_HIP_SLICE_P), the loop filters and
the P-slice coder behind them, against the reference encoder run with --no-bipred (tests/golden/inter_p.json) and, output by output, against the host simulation of
the same sources (tests/hostsim/hostsim_inter_p.cpp).  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import inter_common as ic
import inter_lists_common as ilc
import inter_p_common as pc
import scaling_lists_common as slc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import kvazaar_amd
    return kvazaar_amd.load_library()


@pytest.fixture(scope="module")
def sim():
    return pc.load_sim()


@pytest.fixture(scope="module")
def gold():
    return pc.fixture()


@pytest.fixture(scope="module")
def seq(oracle):
    """pan11 encoded by the oracle as B pictures: inputs of launches that are compared with today's B calls"""
    clip = pc.clip_named("pan11")
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


def _assert_equal(got, want, where):
    """device outputs == simulation outputs byte for byte: samples, CU records, levels"""
    rec, cu, coeff = got
    assert ic.first_difference(cu, want[1]) is None, where
    assert cu.tobytes() == np.ascontiguousarray(want[1]).tobytes(), where
    assert np.array_equal(rec, want[0]), where
    assert np.array_equal(coeff, want[2]), where


_first, _chains = {}, {}


def _first_picture(lib, clip, gop):
    """picture 0 of the clip from HipBatch and its loop filters -> (frames, qps, final picture, CU records), once per clip"""
    import ctu_common as cc
    name, w, h, n, base_qp, preset, dbk, sao, owf, _ = clip
    if name not in _first:
        frames, qps = ic.case_frames(clip), pc.picture_qps(clip, gop)
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


def _device_chain(lib, clip_name):
    """The clip on the device, once per clip: picture 0 from HipBatch and its loop filters; every P picture through InterPictures from the device's own previous
    picture: run, loop_filters and entropy_code with slice_type="P", advance.
    -> dict: qps, frames, final [n], cu [n], inputs [n] of (ref, ref_cu), outputs [n] of the pass's (rec, cu, coeff), slices [n] of (bytes, sizes)"""
    from kvazaar_amd import inter
    if clip_name in _chains:
        return _chains[clip_name]
    clip, gop = pc.clip_named(clip_name), pc.gop_of(clip_name)
    _, w, h, n, base_qp, preset, dbk, sao, owf, _ = clip
    frames, qps, final, cu = _first_picture(lib, clip, gop)
    out = dict(qps=qps, frames=frames, final=[final], cu=[cu], inputs=[None], outputs=[None], slices=[None])
    ip = inter.InterPictures(lib, w, h, 1, with_levels=True)
    try:
        ip.upload(0, frames[1], final, cu.reshape(-1))
        for k in range(1, n):
            if k > 1:
                ip.advance()
                ip.upload_source(0, frames[k])
            ip.dev.copy_in(ip.d_coeff, np.zeros(ip.ctus * 6144, np.int16))
            prm = pc.params_of(clip, qps[k], k)
            ip.run(prm, slice_type="P")
            out["inputs"].append((out["final"][k - 1], out["cu"][k - 1]))
            out["outputs"].append(_outputs(ip))
            ip.loop_filters(prm, slice_type="P")
            out["final"].append(ip.download(0)[0])
            out["cu"].append(out["outputs"][k][1][0])
            data, sizes = ip.entropy_code(prm, slice_type="P")
            out["slices"].append((bytes(data), [int(v) for v in sizes[0]]))
    finally:
        ip.close()
    _chains[clip_name] = out
    return out


# ---------------------------------------------------------------------------------------------------- 1. the chain against the reference encoder and the simulation
@pytest.mark.parametrize("clip_name", pc.names())
def test_device_chain_equals_the_reference_encoder(lib, gold, clip_name):
    """pass -> loop_filters(slice_type="P") -> entropy_code(slice_type="P"), picture k from the device's own picture k - 1 == kvazaar --no-bipred: every final
    picture and the slice data of every P picture"""
    chain, g = _device_chain(lib, clip_name), gold[clip_name]
    assert chain["qps"] == g["qps"]
    for k, final in enumerate(chain["final"]):
        assert ilc.sha(final) == g["rec"][k], (clip_name, k, "picture")
        if k > 0:
            data, sizes = chain["slices"][k]
            assert sizes == g["slices"][k]["sizes"] and ilc.sha(np.frombuffer(data, np.uint8)) == g["slices"][k]["sha"], (clip_name, k, "slice data")


@pytest.mark.parametrize("clip_name", pc.names())
def test_device_pass_equals_the_simulation(lib, sim, clip_name):
    """every P launch of the chain: the pass's reconstruction, CU records and levels are the host simulation's of the same launch, byte for byte; records move by
    list 0 alone"""
    chain, clip = _device_chain(lib, clip_name), pc.clip_named(clip_name)
    _, w, h, n, *_ = clip
    for k in range(1, n):
        ref, ref_cu = chain["inputs"][k]
        rc, *want = pc.sim_pass(sim, [dict(src=chain["frames"][k], ref=ref, ref_cu=ref_cu)], pc.params_of(clip, chain["qps"][k], k), None, w, h, pc.P)
        assert rc == 0
        _assert_equal(chain["outputs"][k], want, (clip_name, k))
        cu = chain["outputs"][k][1]
        assert (cu["mv_dir"][cu["type"] == 2] == 1).all(), (clip_name, k)


# ---------------------------------------------------------------------------------------------------- 2. one launch, pictures of three clips
def test_p_pictures_of_three_clips_share_a_launch(lib, gold, monkeypatch, capfd):
    """pictures 1 and 2 of three 136x72 clips in ONE launch at their own QP and POC through pictures=, each from its own chain's previous picture: pass, loop filters
    and coder give every picture what its own launch gave (the chain's outputs, the fixture's pictures and slice data).  The shared launch holds QPs on both sides
    of fast-residual-cost and takes the `_p_cabac` build; the launches alone reach `_p_fast` too"""
    from kvazaar_amd.inter import InterPictureParams
    clips = [pc.clip_named(nm) for nm in pc.SHARED_LAUNCH]
    assert len({(c[1], c[2], c[5], c[6], c[7], c[8]) for c in clips}) == 1  # one size, one preset, the same switches: one set of launch parameters
    _, w, h, *_ = clips[0]
    chains = [_device_chain(lib, nm) for nm in pc.SHARED_LAUNCH]
    members = [(ci, k) for ci in range(len(clips)) for k in (1, 2)]
    pics = [dict(src=chains[ci]["frames"][k], ref=chains[ci]["inputs"][k][0], ref_cu=chains[ci]["inputs"][k][1]) for ci, k in members]
    table = InterPictureParams([chains[ci]["qps"][k] for ci, k in members], [k for ci, k in members])
    assert min(table.qps) < 28 <= max(table.qps)
    prm = pc.params_of(clips[0], 45, 9)
    monkeypatch.setenv("KVZ_HIP_INTER_VERBOSE", "1")
    ip = _launch(lib, pics, w, h)
    try:
        capfd.readouterr()
        ip.run(prm, pictures=table, slice_type="P")
        assert "p cabac build" in capfd.readouterr().err
        rec, cu, coeff = _outputs(ip)
        for i, (ci, k) in enumerate(members):
            own = chains[ci]["outputs"][k]
            assert rec[i].tobytes() == own[0][0].tobytes() and cu[i].tobytes() == own[1][0].tobytes() and coeff[i].tobytes() == own[2][0].tobytes(), (pc.SHARED_LAUNCH[ci], k)
        ip.loop_filters(prm, pictures=table, slice_type="P")
        data, sizes = ip.entropy_code(prm, pictures=table, slice_type="P")
        data, at = bytes(data), 0
        for i, (ci, k) in enumerate(members):
            g = gold[pc.SHARED_LAUNCH[ci]]
            assert ilc.sha(ip.download(i)[0]) == g["rec"][k], (pc.SHARED_LAUNCH[ci], k, "picture")
            own, own_sizes = chains[ci]["slices"][k]
            assert [int(v) for v in sizes[i]] == own_sizes and data[at:at + len(own)] == own, (pc.SHARED_LAUNCH[ci], k, "slice data")
            at += len(own)
        assert at == len(data)
        # ... and a picture below fast-residual-cost alone: the other build
        i = int(np.argmin(table.qps))
        alone = _launch(lib, [pics[i]], w, h)
        try:
            capfd.readouterr()
            alone.run(pc.params_of(clips[0], int(table.qps[i]), int(table.pocs[i])), slice_type="P")
            assert "p fast build" in capfd.readouterr().err
            assert alone.download(0)[0].tobytes() == rec[i].tobytes()
        finally:
            alone.close()
    finally:
        ip.close()


# ---------------------------------------------------------------------------------------------------- 3. B through the new entry points; nothing leaks from P to B
def test_slice_type_b_is_todays_calls_and_follows_a_p_launch_unchanged(lib, seq, monkeypatch, capfd):
    """KVZ_HIP_SLICE_B through the three new entry points == run, loop_filters and entropy_code as they are called today: the default kernel builds, the same samples,
    records, levels, final pictures and slice data -- also straight after a P launch on the same thread, whose tables and scratch the B launch must not inherit"""
    from kvazaar_amd import inter
    s, clip = seq, seq["clip"]
    w, h = s["w"], s["h"]
    monkeypatch.setenv("KVZ_HIP_INTER_VERBOSE", "1")
    for k in (1, 2):
        prm = pc.params_of(clip, s["qps"][k], k)
        ip = _launch(lib, [_picture(s, k)], w, h)
        try:
            ip.run(prm)
            today = _outputs(ip)
            assert np.array_equal(today[0][0], s["rs"][k])
            ip.loop_filters(prm)
            today_final, today_data = ip.download(0)[0], ip.entropy_code(prm)
            today_data = (bytes(today_data[0]), today_data[1].copy())
            # a P launch, its loop filters and its coder in between
            ip.run(prm, slice_type="P")
            assert not np.array_equal(ip.download(0)[0], today[0][0])
            ip.loop_filters(prm, slice_type="P")
            assert bytes(ip.entropy_code(prm, slice_type="P")[0]) != today_data[0]
            # B by number through the _slices entry points
            ip.dev.copy_in(ip.d_coeff, np.zeros(ip.ctus * 6144, np.int16))
            capfd.readouterr()
            ip.run(prm, slice_type=inter.SLICE_TYPES["B"])
            err = capfd.readouterr().err
            assert "build" in err and "p fast" not in err and "p cabac" not in err, err
            assert all(a.tobytes() == b.tobytes() for a, b in zip(_outputs(ip), today)), k
            ip.loop_filters(prm, slice_type="B")
            assert ip.download(0)[0].tobytes() == today_final.tobytes(), k
            data, sizes = ip.entropy_code(prm, slice_type=inter.SLICE_TYPES["B"])
            assert bytes(data) == today_data[0] and np.array_equal(sizes, today_data[1]), k
            # ... and today's calls after all that
            ip.run(prm)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(_outputs(ip), today)), k
            ip.loop_filters(prm)
            assert ip.download(0)[0].tobytes() == today_final.tobytes() and bytes(ip.entropy_code(prm)[0]) == today_data[0], k
        finally:
            ip.close()


def test_slice_type_i_is_slice_is_b_zero_in_the_loop_filters(lib, seq):
    """kvz_hip_dev_loop_filters_inter_slices with KVZ_HIP_SLICE_I == loop_filters(slice_is_b=False) of today; P deblocks as I does and differs at most by its SAO"""
    s, clip, k = seq, seq["clip"], 1
    prm = pc.params_of(clip, s["qps"][k], k)
    ip = _launch(lib, [_picture(s, k)], s["w"], s["h"])
    try:
        finals = {}
        for name, kw in (("today", dict(slice_is_b=False)), ("I", dict(slice_type="I")), ("P", dict(slice_type="P")), ("B", dict(slice_type="B"))):
            ip.run(prm)
            ip.loop_filters(prm, **kw)
            finals[name] = ip.download(0)[0]
        assert finals["I"].tobytes() == finals["today"].tobytes() and finals["B"].tobytes() != finals["I"].tobytes()
        prm.sao = 0
        for name, kw in (("I", dict(slice_type="I")), ("P", dict(slice_type="P"))):
            ip.run(prm)
            ip.loop_filters(prm, **kw)
            finals[name + " deblock"] = ip.download(0)[0]
        assert finals["I deblock"].tobytes() == finals["P deblock"].tobytes()
    finally:
        ip.close()


# ---------------------------------------------------------------------------------------------------- 4. what is refused
def test_refusals_leave_the_outputs_untouched_and_the_object_usable(lib, sim, seq, capfd):
    """one InterPictures object through every refusal of the three entry points, its outputs filled with a pattern: each returns -1 with a message before anything is
    queued, the pattern stands, and the next P launch on the object is the simulation's"""
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

        def prm(**kw):
            p = pc.params_of(clip, s["qps"][k], k)
            for name, v in kw.items():
                setattr(p, name, v)
            return p

        for p, slice_type, message in ((prm(), 3, "slice type 3 is none of"), (prm(), -1, "slice type -1 is none of"), (prm(), "I", "slice type I"),
                                       (prm(ref_width=w, ref_height=h), "P", "together with tiles"), (prm(tile_x=8), "P", "together with tiles"),
                                       (prm(me_algorithm=1), "P", "together with me_algorithm"), (prm(me_early_termination=2), "P", "together with me_algorithm")):
            fill()
            capfd.readouterr()
            with pytest.raises(RuntimeError, match="returned -1"):
                ip.run(p, slice_type=slice_type)
            err = capfd.readouterr().err
            assert message in err and "kvz_hip_dev_inter_ctu_pass_slices" in err and untouched(), (message, err)
        # P with a tile origin per picture
        fill()
        xy = ip.dev.empty(8)
        ip.dev.copy_in(xy, np.zeros(2, np.int32))
        capfd.readouterr()
        p = prm()  # (alive across the call)
        rc = lib.kvz_hip_dev_inter_ctu_pass_slices(ip.d_src, ip.d_ref, ip.d_ref_cu, ip.d_rec, ip.d_cu, ip.d_coeff, w, h, 1, C.addressof(p), xy, 1, None, pc.P)
        ip.dev.free(xy)
        assert rc == -1 and "together with tiles" in capfd.readouterr().err and untouched()
        # the loop filters and the coder
        for slice_type in (3, -1):
            with pytest.raises(RuntimeError, match="returned -1"):
                ip.loop_filters(prm(), slice_type=slice_type)
            assert "kvz_hip_dev_loop_filters_inter_slices" in capfd.readouterr().err and untouched()
        for slice_type, message in ((3, "slice type 3 is none of"), ("I", "slice type I")):
            with pytest.raises(RuntimeError, match="failed"):
                ip.entropy_code(prm(), slice_type=slice_type)
            err = capfd.readouterr().err
            assert message in err and "kvz_hip_dev_entropy_code_inter_slices" in err and untouched(), err
        # P pictures take no scaling lists: the binding says so before the library is asked
        ip.set_scaling_lists([slc.lists("default")])
        with pytest.raises(ValueError, match="scaling lists"):
            ip.run(prm(), slice_type="P")
        ip.clear_scaling_lists()
        assert untouched()
        # the object still works
        ip.dev.copy_in(ip.d_coeff, np.zeros(ip.ctus * 6144, np.int16))
        ip.run(prm(), slice_type="P")
        rc, *want = pc.sim_pass(sim, [_picture(s, k)], prm(), None, w, h, pc.P)
        assert rc == 0
        _assert_equal(_outputs(ip), want, "after the refusals")
    finally:
        ip.close()
