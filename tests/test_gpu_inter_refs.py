"""P pictures with reference lists of 1 to 4 pictures (kvazaar's --no-bipred --ref N) on the MI355X: the REFS builds of the inter kernel
(kvz_hip_dev_inter_ctu_pass_refs), the loop filters and the coder behind them, against the reference encoder run with --no-bipred --ref N
(tests/golden/inter_refs.json) and, output by output, against the host simulation of the same sources (tests/hostsim/hostsim_inter_refs.cpp).  The sequences stay
resident: every finished picture moves into its sequence's pool on the device (InterPictures.advance_pool).  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import inter_common as ic
import inter_lists_common as ilc
import inter_p_common as pc
import inter_refs_common as rc
import scaling_lists_common as slc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import kvazaar_amd
    return kvazaar_amd.load_library()


@pytest.fixture(scope="module")
def sim():
    return rc.load_sim()


@pytest.fixture(scope="module")
def gold():
    return rc.fixture()


def _outputs(ip):
    rec, cu = zip(*[ip.download(i) for i in range(ip.n)])
    return np.stack(rec), np.stack(cu), ip.dev.get(ip.d_coeff, (ip.n, ip.ctus * 6144), np.int16)


def _zero_levels(ip):
    """(a CTU that reaches beyond the picture is not written whole)"""
    ip.dev.copy_in(ip.d_coeff, np.zeros(ip.n * ip.ctus * 6144, np.int16))


_first, _chains = {}, {}


def _first_picture(lib, case):
    """picture 0 of the case from HipBatch and its loop filters -> (frames, qps, final picture, CU records), once per case"""
    import ctu_common as cc
    key, clip, gop, ref = case
    name, w, h, n, base_qp, preset, dbk, sao, owf, _ = clip
    if key not in _first:
        frames, qps = rc.case_frames(clip), rc.picture_qps(clip, gop)
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
        _first[key] = (frames, qps, final, ilc.intra_cu_records(o["depth"], o["mode"], w, h))
    return _first[key]


def _pool_table(ip, slot_poc, ref_pocs_of, lists):
    """InterReferences over the whole pool of `ip` (one sequence): slot_poc {slot: POC}; an empty slot gets a POC nothing asks for"""
    from kvazaar_amd.inter import InterReferences
    pocs = [slot_poc.get(s, -1 - s) for s in range(ip.pool)]
    return InterReferences(pocs, [ref_pocs_of.get(p, []) for p in pocs], [len(l) for l in lists], lists)


def _device_chain(lib, name):
    """The case on the device, once per case: picture 0 from HipBatch and its loop filters into slot 0 of the pool; every P picture through InterPictures from the
    pool -- run, loop_filters and entropy_code with the picture's list, then advance_pool into a slot the next picture's list does not name.  Nothing but the
    source pictures is uploaded after picture 0.
    -> dict: qps, frames, lists, final [n], cu [n], outputs [n] of the pass's (rec, cu, coeff), slices [n] of (bytes, sizes)"""
    from kvazaar_amd import inter
    if name in _chains:
        return _chains[name]
    case = rc.case_named(name)
    key, clip, gop, ref = case
    _, w, h, n, base_qp, preset, dbk, sao, owf, _ = clip
    frames, qps, final, cu = _first_picture(lib, case)
    out = dict(qps=qps, frames=frames, lists=[[]], final=[final], cu=[cu], outputs=[None], slices=[None])
    ip = inter.InterPictures(lib, w, h, 1, with_levels=True, pool=ref)
    try:
        ip.upload_pool(0, 0, final, cu.reshape(-1))
        slot_poc, ref_pocs_of = {0: 0}, {0: []}
        for k in range(1, n):
            pocs = inter.reference_pocs(k, ref, gop)
            slot_of = {p: s for s, p in slot_poc.items()}
            references = _pool_table(ip, slot_poc, ref_pocs_of, [[ip.pool_frame(slot_of[p], 0) for p in pocs]])
            table = inter.InterPictureParams([qps[k]], [k], references=references)
            ip.upload_source(0, frames[k])
            _zero_levels(ip)
            prm = pc.params_of(clip, qps[k], k)
            ip.run(prm, pictures=table, slice_type="P")
            out["outputs"].append(_outputs(ip))
            ip.loop_filters(prm, pictures=table, slice_type="P")
            out["final"].append(ip.download(0)[0])
            out["cu"].append(out["outputs"][k][1][0])
            data, sizes = ip.entropy_code(prm, pictures=table, slice_type="P")
            out["slices"].append((bytes(data), [int(v) for v in sizes[0]]))
            out["lists"].append(pocs)
            keep = set(inter.reference_pocs(k + 1, ref, gop)) - {k}
            free = [s for s in range(ip.pool) if slot_poc.get(s) not in keep]
            ip.advance_pool(free[0])
            slot_poc[free[0]], ref_pocs_of[k] = k, pocs
    finally:
        ip.close()
    _chains[name] = out
    return out


# ---------------------------------------------------------------------------------------------------- 1. the chain against the reference encoder and the simulation
@pytest.mark.parametrize("name", rc.names())
def test_device_chain_equals_the_reference_encoder(lib, gold, name):
    """pass -> loop filters -> coder with the picture's list, picture k from the device's own earlier pictures in the resident pool == kvazaar --no-bipred --ref N:
    every final picture and the slice data of every P picture, up to ten pictures through advance_pool"""
    chain, g = _device_chain(lib, name), gold[name]
    assert chain["qps"] == g["qps"] and chain["lists"] == g["lists"]
    for k, final in enumerate(chain["final"]):
        assert ilc.sha(final) == g["rec"][k], (name, k, "picture")
        if k > 0:
            data, sizes = chain["slices"][k]
            assert sizes == g["slices"][k]["sizes"] and ilc.sha(np.frombuffer(data, np.uint8)) == g["slices"][k]["sha"], (name, k, "slice data")


@pytest.mark.parametrize("name", rc.SMALLEST)
def test_device_pass_equals_the_simulation(lib, sim, name):
    """every P launch of the chain: the pass's reconstruction, CU records and levels are the host simulation's of the same launch, byte for byte"""
    from kvazaar_amd.inter import InterPictureParams
    chain, clip = _device_chain(lib, name), rc.case_named(name)[1]
    _, w, h, n, *_ = clip
    ref_pocs_of = {k: chain["lists"][k] for k in range(n)}
    for k in range(1, n):
        pocs = chain["lists"][k]
        references = rc.references_of([(p, ref_pocs_of[p]) for p in pocs], [list(range(len(pocs)))])
        rc_, *want = rc.sim_pass(sim, [chain["frames"][k]], [chain["final"][p] for p in pocs], [chain["cu"][p] for p in pocs], pc.params_of(clip, chain["qps"][k], k),
                                 InterPictureParams([chain["qps"][k]], [k]), references, w, h)
        assert rc_ == 0
        rec, cu, coeff = chain["outputs"][k]
        assert ic.first_difference(cu, want[1]) is None, (name, k)
        assert cu.tobytes() == np.ascontiguousarray(want[1]).tobytes() and np.array_equal(rec, want[0]) and np.array_equal(coeff, want[2]), (name, k)


# ---------------------------------------------------------------------------------------------------- 2. one launch, lists of three lengths
def test_pictures_with_lists_of_three_lengths_share_a_launch(lib, monkeypatch, capfd):
    """pictures 1, 2 and 3 of the alternating clip (lists of one, two and three entries) in ONE launch at their own QP and POC over one pool: pass, loop filters and
    coder give every picture what a launch of its own over its own pool gives.  The shared launch holds QPs on both sides of fast-residual-cost and takes the
    `refs cabac` build; the picture below it alone takes `refs fast`"""
    from kvazaar_amd import inter
    name = "alt-gop0-ref3"
    chain, clip = _device_chain(lib, name), rc.case_named(name)[1]
    _, w, h, *_ = clip
    ks, qps = (3, 1, 2), (22, 33, 27)
    prm = pc.params_of(clip, 45, 9)
    monkeypatch.setenv("KVZ_HIP_INTER_VERBOSE", "1")

    def launch(members):
        """members: [(k, qp)] -> (pass outputs, final pictures, slice data, sizes); sequence i's pool holds its list's frames in REVERSE list order"""
        n = len(members)
        ip = inter.InterPictures(lib, w, h, n, with_levels=True, pool=3)
        try:
            frame_pocs, frame_refs, lists = [-1 - f for f in range(3 * n)], [[] for _ in range(3 * n)], []
            for i, (k, q) in enumerate(members):
                pocs = chain["lists"][k]
                ip.upload_source(i, chain["frames"][k])
                for j, p in enumerate(pocs):
                    slot = 2 - j
                    ip.upload_pool(slot, i, chain["final"][p], chain["cu"][p].reshape(-1))
                    frame_pocs[ip.pool_frame(slot, i)], frame_refs[ip.pool_frame(slot, i)] = p, chain["lists"][p]
                lists.append([ip.pool_frame(2 - j, i) for j in range(len(pocs))])
            table = inter.InterPictureParams([q for _, q in members], [k for k, _ in members],
                                             references=inter.InterReferences(frame_pocs, frame_refs, [len(l) for l in lists], lists))
            _zero_levels(ip)
            capfd.readouterr()
            ip.run(prm, pictures=table, slice_type="P")
            build = capfd.readouterr().err
            outputs = _outputs(ip)
            ip.loop_filters(prm, pictures=table, slice_type="P")
            finals = [ip.download(i)[0] for i in range(n)]
            data, sizes = ip.entropy_code(prm, pictures=table, slice_type="P")
            return outputs, finals, bytes(data), [[int(v) for v in row] for row in sizes], build
        finally:
            ip.close()

    joint = launch(list(zip(ks, qps)))
    assert "refs cabac build" in joint[4], joint[4]
    at = 0
    for i, member in enumerate(zip(ks, qps)):
        alone = launch([member])
        assert ("refs fast build" if member[1] < 28 else "refs cabac build") in alone[4], alone[4]
        assert all(a[i].tobytes() == b[0].tobytes() for a, b in zip(joint[0], alone[0])), member
        assert joint[1][i].tobytes() == alone[1][0].tobytes() and joint[3][i] == alone[3][0] and joint[2][at:at + len(alone[2])] == alone[2], member
        at += len(alone[2])
    assert at == len(joint[2])
    # the picture at the chain's own QP is the chain's
    assert all(a[2].tobytes() == b[0].tobytes() for a, b in zip(joint[0], chain["outputs"][2]))
    cu = joint[0][1][0]
    assert (cu["mv_ref"][cu["type"] == 2][:, 0] > 0).any()  # (the launch did use entries behind the first)


# ---------------------------------------------------------------------------------------------------- 3. no lists: the twins
def test_no_references_is_the_slices_twin(lib):
    """refs == NULL through the three new entry points is kvz_hip_dev_*_slices: the same samples, records, levels, final picture and slice data"""
    from kvazaar_amd import inter
    name = "alt-gop0-ref3"
    chain, clip = _device_chain(lib, name), rc.case_named(name)[1]
    _, w, h, *_ = clip
    k = 2
    prm, table = pc.params_of(clip, chain["qps"][k], k), inter.InterPictureParams([chain["qps"][k]], [k])
    ip = inter.InterPictures(lib, w, h, 1, with_levels=True)
    try:
        ip.upload(0, chain["frames"][k], chain["final"][k - 1], chain["cu"][k - 1].reshape(-1))
        _zero_levels(ip)
        ip.run(prm, pictures=table, slice_type="P")
        want = _outputs(ip)
        ip.loop_filters(prm, pictures=table, slice_type="P")
        want_final, (want_data, want_sizes) = ip.download(0)[0], ip.entropy_code(prm, pictures=table, slice_type="P")
        want_data, want_sizes = bytes(want_data), want_sizes.copy()
        _zero_levels(ip)
        assert lib.kvz_hip_dev_inter_ctu_pass_refs(ip.d_src, ip.d_ref, ip.d_ref_cu, ip.d_rec, ip.d_cu, ip.d_coeff, w, h, 1, C.addressof(prm), None, 0, table.ptr, pc.P, None) == 0
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_outputs(ip), want))
        lib.kvz_hip_dev_cu_dbk_from_info(ip.d_cu, ip.cells, ip.d_dbk)
        assert lib.kvz_hip_dev_loop_filters_inter_refs(ip.d_src, ip.d_rec, w, h, 1, ip.d_dbk, prm.qp, table.qps.ctypes.data, pc.P, prm.deblock, 0, 0, prm.sao, prm.no_wpp, None, None, None, None) == 0
        assert ip.download(0)[0].tobytes() == want_final.tobytes()
        sizes = np.zeros_like(want_sizes)
        total = lib.kvz_hip_dev_entropy_code_inter_refs(ip.d_cu, ip.d_ref_cu, ip.d_coeff, w, h, 1, C.addressof(prm), ip._entropy_out.ctypes.data, ip._entropy_out.nbytes, sizes.ctypes.data,
                                                        table.ptr, pc.P, None)
        assert total == len(want_data) and bytes(ip._entropy_out[:total]) == want_data and np.array_equal(sizes, want_sizes)
    finally:
        ip.close()


# ---------------------------------------------------------------------------------------------------- 4. what is refused
def test_refusals_leave_the_outputs_untouched_and_the_object_usable(lib, capfd):
    """one InterPictures object through refusals of the three entry points, its outputs filled with a pattern: each returns -1 with a message before anything is
    queued, the pattern stands, and the next launch on the object is the chain's"""
    from kvazaar_amd import inter
    name = "alt-gop0-ref3"
    chain, clip = _device_chain(lib, name), rc.case_named(name)[1]
    _, w, h, *_ = clip
    k = 2
    pocs = chain["lists"][k]
    ip = inter.InterPictures(lib, w, h, 1, with_levels=True, pool=2)
    try:
        ip.upload_source(0, chain["frames"][k])
        for j, p in enumerate(pocs):
            ip.upload_pool(j, 0, chain["final"][p], chain["cu"][p].reshape(-1))
        pattern = [np.full(ip.fs, 0xa5, np.uint8), np.full(ip.cells * inter.CU_DTYPE.itemsize, 0x5a, np.uint8), np.full(ip.ctus * 6144, 0x1234, np.int16)]

        def fill():
            for d, a in zip((ip.d_rec, ip.d_cu, ip.d_coeff), pattern):
                ip.dev.copy_in(d, a)

        def untouched():
            return (np.array_equal(ip.dev.get(ip.d_rec, (ip.fs,), np.uint8), pattern[0]) and np.array_equal(ip.dev.get(ip.d_cu, (pattern[1].size,), np.uint8), pattern[1])
                    and np.array_equal(ip.dev.get(ip.d_coeff, (ip.ctus * 6144,), np.int16), pattern[2]))

        def refs(frame_pocs=tuple(pocs), lists=((0, 1),), **kw):
            r = inter.InterReferences(list(frame_pocs), [chain["lists"][p] if 0 <= p < len(chain["lists"]) else [] for p in frame_pocs], [len(l) for l in lists], [list(l) for l in lists])
            for field, v in kw.items():
                setattr(r.struct, field, v)
            return r

        prm = pc.params_of(clip, chain["qps"][k], k)
        five = refs()
        five.n_refs[0] = 5
        cases = [(refs(struct_size=44), "P", k, "struct_size 44 is not this library's"), (refs(n_pictures=2), "P", k, "n_pictures 2 is not the call's 1"), (five, "P", k, "a list of 5 references"),
                 (refs(lists=((0, 2),)), "P", k, "frame 2 is outside the pool of 2"), (refs(frame_pocs=(1, 1)), "P", k, "both have POC 1"),
                 (refs(), "P", 1, "not below the picture's"), (refs(), "B", k, "KVZ_HIP_SLICE_P only")]
        for r, slice_type, poc, message in cases:
            table = inter.InterPictureParams([chain["qps"][k]], [poc], references=r)
            fill()
            capfd.readouterr()
            with pytest.raises(RuntimeError, match="returned -1"):
                ip.run(prm, pictures=table, slice_type=slice_type)
            err = capfd.readouterr().err
            assert message in err and "kvz_hip_dev_inter_ctu_pass_refs" in err and untouched(), (message, err)
            with pytest.raises(RuntimeError, match="failed"):
                ip.entropy_code(prm, pictures=table, slice_type=slice_type)
            err = capfd.readouterr().err
            assert message in err and "kvz_hip_dev_entropy_code_inter_refs" in err and untouched(), (message, err)
            if "not below" not in message:  # (the filters read no POC)
                with pytest.raises(RuntimeError, match="returned -1"):
                    ip.loop_filters(prm, pictures=table, slice_type=slice_type)
                err = capfd.readouterr().err
                assert message in err and "kvz_hip_dev_loop_filters_inter_refs" in err and untouched(), (message, err)
        # lists without a POC per picture; lists together with a chosen integer search
        good = refs()
        fill()
        rc_ = lib.kvz_hip_dev_inter_ctu_pass_refs(ip.d_src, ip.d_ref, ip.d_ref_cu, ip.d_rec, ip.d_cu, ip.d_coeff, w, h, 1, C.addressof(prm), None, 0, None, pc.P, good.ptr)
        assert rc_ == -1 and "need `pictures`" in capfd.readouterr().err and untouched()
        me = pc.params_of(clip, chain["qps"][k], k)
        me.me_algorithm = 1
        with pytest.raises(RuntimeError, match="returned -1"):
            ip.run(me, pictures=inter.InterPictureParams([chain["qps"][k]], [k], references=good), slice_type="P")
        assert "together with me_algorithm" in capfd.readouterr().err and untouched()
        # the object still works
        _zero_levels(ip)
        ip.run(prm, pictures=inter.InterPictureParams([chain["qps"][k]], [k], references=good), slice_type="P")
        assert capfd.readouterr().err == ""
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_outputs(ip), chain["outputs"][k]))
    finally:
        ip.close()
