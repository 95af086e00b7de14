"""Batches of different picture sizes in ONE launch of the all-intra CTU pass on the MI355X (kvz_hip_batch_group).  Every picture stays an ordinary picture of its
own size and QP, so every output has a truth that exists already: the reference encoder's digests under tests/golden/ and the unchanged oracle."""
import ctypes as C

import numpy as np
import pytest

import ctu_common as cc
import joint_common as jc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import kvazaar_amd
    return kvazaar_amd.load_library()


class Group:
    """the batches of `specs` with their pictures uploaded, their tables, and the group"""

    def __init__(self, lib, specs, **switches):
        from kvazaar_amd.batch import BatchGroup
        self.specs = specs
        self.batches = []
        for s in specs:
            b = cc.HipBatch(lib, s.w, s.h, len(s.frames))
            for i, f in enumerate(s.frames):
                b.upload(i, f)
            self.batches.append(b)
        self.tables = [jc.table(lib, s.qps, **switches) for s in specs]
        self.group = BatchGroup(lib, self.batches)

    def outputs(self):
        return [[b.download(i) for i in range(b.n)] for b in self.batches]

    def digests(self):
        return [[(jc.sha(o["rec"]), jc.cu_digest(o, b.w, b.h), jc.sha(o["coeff"]), jc.sha(o["cost"])) for o in outs] for b, outs in zip(self.batches, self.outputs())]

    def close(self):
        self.group.close()
        for b in self.batches:
            b.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _check(oracle, g, outs, suffix="", no_wpp=False, cu=True, **switches):
    for s, o in zip(g.specs, outs):
        if s.clip is not None:
            assert [jc.sha(p["rec"]) for p in o] == s.want(suffix, 0, no_wpp), (s.w, s.h)
            if cu:
                assert [jc.cu_digest(p, s.w, s.h) for p in o] == s.want("/cu"), (s.w, s.h)
        else:
            for i, p in enumerate(o):
                want = cc.run_oracle(oracle, jc.oracle_model(oracle, s.qps[i], **switches), s.w, s.h, s.frames[i])
                assert not cc.compare(p, want), (s.w, s.h, i, cc.compare(p, want))


def test_joint_pass_then_each_batchs_own_deblocking_and_coder(oracle, lib):
    """three fixture sizes at four QPs, a lone 8x8 CTU and 48x40 in one launch; then, per batch, what follows a pass"""
    with Group(lib, jc.main_group() + jc.small_specs()) as g:
        g.group.run(g.tables)
        assert g.group.kernel_ms() > 0
        _check(oracle, g, g.outputs())
        coded = g.batches[2].entropy_code(g.tables[2])
        for s, b, pm in zip(g.specs[:3], g.batches, g.tables):
            b.loop_filters(pm, deblock=True, sao=False)
            assert [jc.sha(b.download(i)["rec"]) for i in range(b.n)] == s.want("", 1), (s.w, s.h)
        data, sizes = coded
        got, at = [], 0
        for row in sizes:
            got.append((bytes(data[at:at + int(row.sum())]), [int(v) for v in row]))
            at += int(row.sum())
        jc.check_slice_data([got[0], got[3]], jc.ENTROPY["partial-ctus-qp27"])


def test_a_solo_pass_between_two_joint_passes(oracle, lib):
    """a batch counts its own passes: a solo pass under other QPs between two joint ones disturbs neither"""
    with Group(lib, jc.main_group() + jc.small_specs()) as g:
        g.group.run(g.tables)
        first = g.digests()
        b, s = g.batches[2], g.specs[2]
        other = jc.clip_spec(200, 136, 2, 3, "small", [37, 27, 27, 37], [0, 0, 1, 1])
        b.run(jc.table(lib, other.qps))
        solo = [b.download(i) for i in range(4)]
        assert [jc.sha(p["rec"]) for p in solo] == other.want() and [jc.cu_digest(p, 200, 136) for p in solo] == other.want("/cu")
        g.batches[0].run(jc.table(lib, [30, 30]))  # ... and one that leaves a batch's pass count odd against the others'
        g.group.run(g.tables)
        assert g.digests() == first
        _check(oracle, g, g.outputs())


BUILDS = {"search32+cabac": dict(search_32x32=1, coeff_cabac=1), "no_wpp": dict(no_wpp=1)}


@pytest.mark.parametrize("name", list(BUILDS))
def test_joint_builds(oracle, lib, name):
    sw = BUILDS[name]
    if name == "no_wpp":
        specs = jc.main_group() + [jc.clip_spec(200, 136, 2, 3, "small", [32, 32]), jc.clip_spec(64, 136, 1, 3, "small", [22])] + jc.small_specs()
    else:
        specs = jc.main_group(qp_200=(27, 27, 27, 27))
    with Group(lib, specs, **sw) as g:
        g.group.run(g.tables)
        outs = g.outputs()
        if name == "no_wpp":
            for s, o in zip(specs, outs):  # everything against the oracle; the two clips with a digest against it too
                for i, p in enumerate(o):
                    want = cc.run_oracle(oracle, jc.oracle_model(oracle, s.qps[i], no_wpp=1), s.w, s.h, s.frames[i])
                    assert not cc.compare(p, want), (s.w, s.h, i, cc.compare(p, want))
            for s, o in zip(specs[3:5], outs[3:5]):
                assert [jc.sha(p["rec"]) for p in o] == s.want("", 0, no_wpp=True)
        else:
            _check(oracle, g, outs, "/fast", cu=False)


@pytest.mark.parametrize("sw", [dict(search_32x32=1), dict(search_32x32=1, signhide=1)], ids=["search32", "signhide+search32"])
def test_joint_builds_no_preset_reaches_equal_the_host_simulation(lib, sw):
    """search_32x32 without the CABAC coefficient model -- intra_ctu_joint_kernel<false, true, false> -- and, hiding signs, <true, true, true>: three 136x136 pictures
    (3x3 CTUs, the right column and the bottom row partial: every hand-off kind) in two batches, byte for byte against the host simulation, which takes its build as
    the library does"""
    p = cc.yuv_frames(136, 136, 3, 11, "small")
    specs = [jc.Spec(136, 136, p[:2], [22, 27]), jc.Spec(136, 136, p[2:], [22])]
    with Group(lib, specs, **sw) as g:
        assert not any(t.model_of(i).coeff_cabac for t in g.tables for i in range(len(t.qps)))  # what selects those kernels
        g.group.run(g.tables)
        rc, want = jc.sim_joint(jc.load_sim(), specs, g.tables)
        assert rc == 0
        got = g.outputs()
        bad = [(k, i, cc.compare(o, w)) for k, (a, b) in enumerate(zip(got, want)) for i, (o, w) in enumerate(zip(a, b)) if cc.compare(o, w)]
        assert not bad, bad
        assert 1 in {int(v) for a in got for o in a for v in np.unique(o["depth"])}  # 32x32 CUs do occur


def test_sign_hiding_in_some_batches_of_a_group(lib):
    a, b = jc.clip_spec(64, 64, 2, 9, "small", [22, 22]), jc.clip_spec(200, 136, 2, 3, "small", [27, 27])
    specs, hide = [a, b, a, b], [1, 0, 0, 1]
    with Group(lib, specs) as g:
        g.tables = [jc.table(lib, s.qps, signhide=h) for s, h in zip(specs, hide)]
        g.group.run(g.tables)
        hidden = {64: jc.SIGNHIDE["ultrafast-64x64-qp22"]["rec"], 200: jc.SIGNHIDE["ultrafast-200x136-qp27"]["rec"]}
        for s, h, o in zip(specs, hide, g.outputs()):
            assert [jc.sha(p["rec"]) for p in o] == (hidden[s.w] if h else s.want()), (s.w, h)


def test_more_tickets_than_resident_workgroups(lib):
    """832x480 x 20, 416x240 x 8, 200x136 x 2: 2 080 + 224 + 24 CTUs against 2 048 workgroup slots -- workgroups draw a second ticket, of another geometry"""
    big = jc.clip_spec(832, 480, 1, 5, "large", [22] * 20, [0] * 20)
    mid = jc.clip_spec(416, 240, 3, 1234, "small", [22] * 8, [i % 3 for i in range(8)])
    small = jc.clip_spec(200, 136, 2, 3, "small", [27, 27])
    with Group(lib, [big, mid, small]) as g:
        g.group.run(g.tables)
        for s, b in zip(g.specs, g.batches):
            assert [jc.sha(b.download(i)["rec"]) for i in range(b.n)] == s.want(), (s.w, s.h)


def test_ordering_against_uploads_and_downloads(lib):
    """the joint pass is every batch's pass: an upload queued behind it replaces the pictures after it has read them, a download queued behind it returns its data"""
    from kvazaar_amd.batch import PinnedResults, pinned_bytes, pinned_free
    a, b = jc.clip_spec(64, 64, 2, 9, "small", [22, 22]), jc.clip_spec(200, 136, 2, 3, "small", [27, 27])
    with Group(lib, [a, b]) as g:
        bb = g.batches[1]
        ptr, view = pinned_bytes(lib, 2 * b.frames[0].size)
        results = PinnedResults(bb)
        try:
            view[:] = np.concatenate([b.frames[1], b.frames[0]])  # the OTHER pictures: the clip's two the other way round
            old, new = b.want(), b.want()[::-1]
            assert g.group.launch(g.tables) == 1
            bb.upload_all_async(ptr)  # no sync in between
            for x in g.batches:
                x.sync()
            assert [jc.sha(bb.download(i)["rec"]) for i in range(2)] == old
            g.group.run(g.tables)  # waits for the upload
            assert [jc.sha(bb.download(i)["rec"]) for i in range(2)] == new
            assert [jc.sha(g.batches[0].download(i)["rec"]) for i in range(2)] == a.want()
            for i, f in enumerate(b.frames):
                bb.upload(i, f)  # the first arrangement again
            assert g.group.launch(g.tables) == 1
            results.download_async()  # right behind the joint launch
            for x in g.batches:
                x.sync()
            assert [jc.sha(r) for r in results.array("rec").reshape(2, -1)] == old
        finally:
            results.close()
            pinned_free(lib, ptr)


def _flags(lib, b):
    flags = np.zeros(b.n * b.ctus_per_frame, np.uint32)
    lib.kvz_hip_batch_debug_flags.argtypes = [C.c_void_p, C.c_void_p]
    lib.kvz_hip_batch_debug_flags.restype = C.c_uint
    return lib.kvz_hip_batch_debug_flags(b.handle, flags.ctypes.data), flags


def test_refusals_and_the_python_view(lib, capfd):
    from kvazaar_amd.batch import BatchError, BatchGroup, ScalingLists
    a, b = jc.clip_spec(64, 64, 2, 9, "small", [22, 22]), jc.clip_spec(72, 88, 2, 1, "small", [12, 12])
    with Group(lib, [a, b]) as g:
        def refused(tables):
            capfd.readouterr()
            rc = g.group.launch(tables)
            err = capfd.readouterr().err
            return rc == -1 and "kvz_hip_batch_group_intra_frames" in err
        assert refused([jc.table(lib, s.qps, rdoq=1, coeff_cabac=1, search_32x32=1) for s in g.specs])
        assert refused([jc.table(lib, s.qps, search_nxn=1, coeff_cabac=1, search_32x32=1) for s in g.specs])
        assert refused([jc.table(lib, a.qps, search_32x32=1), jc.table(lib, b.qps)])
        assert refused([jc.table(lib, a.qps), jc.table(lib, b.qps, no_wpp=1)])
        bad = jc.table(lib, [22, 30])
        bad.index[1] = 5
        assert refused([bad, g.tables[1]])
        g.batches[1].set_scaling_lists([ScalingLists.default(lib)])
        assert refused(g.tables)
        g.batches[1].clear_scaling_lists()
        with pytest.raises(BatchError):
            g.group.run([jc.table(lib, a.qps), jc.table(lib, b.qps, no_wpp=1)])
        with pytest.raises(ValueError):
            g.group.launch([jc.table(lib, [22, 22, 22]), g.tables[1]])  # a table of three pictures for a batch of two
        with pytest.raises(ValueError):
            g.group.launch(g.tables[:1])
        for x in g.batches:  # NOTHING was queued on any batch: no pass has ever run on them
            x.sync()
            epoch, flags = _flags(lib, x)
            assert epoch == 0 and not flags.any()
        with pytest.raises(RuntimeError):
            BatchGroup(lib, [g.batches[0], g.batches[1], g.batches[0]])
        with pytest.raises(RuntimeError):
            BatchGroup(lib, [])
        assert "kvz_hip_batch_group_create" in capfd.readouterr().err
        # a CostModel in place of a table: one model for all of that batch's pictures
        g.group.run([cc.hip_cost_model(lib, 22, jc.weights(22)), g.tables[1]])
        for s, x in zip(g.specs, g.batches):
            assert [jc.sha(x.download(i)["rec"]) for i in range(x.n)] == s.want()
            assert _flags(lib, x)[0] == 1
    closed = cc.HipBatch(lib, 64, 64, 1)
    closed.close()
    with pytest.raises(ValueError):
        BatchGroup(lib, [closed])


def test_batches_of_two_devices_are_refused(lib, capfd):
    from kvazaar_amd.batch import BatchGroup
    lib.kvz_hip_device_count.restype = C.c_int
    if lib.kvz_hip_device_count() < 2:
        pytest.skip("one device: a batch on another device cannot be created")
    a, b = cc.HipBatch(lib, 64, 64, 1, device=0), cc.HipBatch(lib, 64, 64, 1, device=1)
    try:
        with pytest.raises(RuntimeError):
            BatchGroup(lib, [a, b])
        assert "device" in capfd.readouterr().err
    finally:
        a.close()
        b.close()
