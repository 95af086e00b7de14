"""Pictures with a QP and a POC of their own in ONE launch of the inter path on the MI355X (kvz_hip_inter_pictures; kvz_hip_dev_inter_ctu_pass_pictures,
kvz_hip_dev_loop_filters_inter_pictures, kvz_hip_dev_entropy_code_inter_pictures).  Every picture stays an ordinary constant-QP picture, so its reference exists
already: the oracle's encode of its own sequence alone (tests/inter_mixed_common.py; the oracle is pinned to the reference encoder).  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest

import entropy_common as ec
import inter_common as ic
import inter_mixed_common as mx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import kvazaar_amd
    return kvazaar_amd.load_library()


def _launch(lib, pics, with_levels=False, w=mx.W, h=mx.H):
    from kvazaar_amd import inter
    ip = inter.InterPictures(lib, w, h, len(pics), with_levels=with_levels)
    for i, p in enumerate(pics):
        ip.upload(i, p["src"], p["ref"], np.ascontiguousarray(p["ref_cu"]).reshape(-1))
    return ip


def _table(pics):
    from kvazaar_amd.inter import InterPictureParams
    return InterPictureParams([p["qp"] for p in pics], [p["poc"] for p in pics])


def _assert_launch_equals_the_oracle(ip, pics):
    for i, p in enumerate(pics):
        rec, cu = ip.download(i)
        where = (i, p["qp"], p["poc"])
        assert ic.first_difference(cu[None], np.asarray(p["cu"])[None]) is None, where
        assert np.array_equal(rec, p["rec"]), where


def test_mixed_pass_with_every_workgroup_crossing_pictures_equals_the_oracle(lib):
    """the ten pictures of the CPU test (sequences at --qp 17 .. 37, POC 1 .. 3), seven copies each: 70 pictures of 20 CTUs, 1400 tickets for the one workgroup per
    CU the share leaves -- every workgroup draws CTUs of many pictures, QPs and POCs.  Every copy of every picture is its own sequence's"""
    base = mx.veryfast_pictures()
    pics = [p for _ in range(7) for p in base]
    assert len(pics) >= 64
    lib.kvz_hip_dev_inter_slots_per_cu.restype = C.c_int
    ip = _launch(lib, pics)
    lib.kvz_hip_dev_inter_set_share(int(lib.kvz_hip_dev_inter_slots_per_cu()))  # one workgroup per CU
    try:
        ip.run(mx.launch_params("veryfast"), pictures=_table(pics))
    finally:
        lib.kvz_hip_dev_inter_set_share(1)
    _assert_launch_equals_the_oracle(ip, pics)
    ip.close()


@pytest.mark.parametrize("which,build", [("fast", "fast"), ("cabac", "cabac"), ("mixed", "cabac")])
def test_both_kernel_builds_and_the_cabac_builds_fast_path(lib, which, build, monkeypatch, capfd):
    """all picture QPs below fast-residual-cost 28 (the `_fast` build), all from 28 on (the `_cabac` build), and both in one launch: the `_cabac` build, whose
    pictures below 28 run with coeff_cabac == 0 -- what no single-QP launch does"""
    base = mx.veryfast_pictures()
    pics = [p for p in base if which == "mixed" or (p["qp"] < 28) == (which == "fast")] * 3
    qps = {p["qp"] for p in pics}
    assert (min(qps) < 28) == (which != "cabac") and (max(qps) >= 28) == (which != "fast")
    monkeypatch.setenv("KVZ_HIP_INTER_VERBOSE", "1")
    ip = _launch(lib, pics)
    capfd.readouterr()
    ip.run(mx.launch_params("veryfast"), pictures=_table(pics))
    assert f"{build} build" in capfd.readouterr().err
    _assert_launch_equals_the_oracle(ip, pics)
    ip.close()


def test_chain_of_three_sequences_out_of_phase_pass_filters_coder(lib):
    """pass -> cu_dbk_from_info -> loop_filters_inter_pictures -> entropy_code_inter_pictures over two B pictures of sequences at --qp 22, 27, 32 that stand one
    picture apart: the launches hold POC (1, 2, 1) and then (2, 3, 2), every sequence predicting from the device's own previous picture.  The filtered pictures, the
    SAO decisions and the slice bytes are those of each sequence's own encode"""
    from kvazaar_amd import inter
    seqs = [mx.sequence(qp, seed=i) for i, qp in ((1, 22), (2, 27), (3, 32))]
    first = (1, 2, 1)
    w, h, n = mx.W, mx.H, len(seqs)
    ctus, rows = 20, (h + 63) // 64
    prm = mx.launch_params("veryfast")
    ip = inter.InterPictures(lib, w, h, n, with_levels=True)
    for i, (s, k) in enumerate(zip(seqs, first)):
        ip.upload(i, s["frames"][k], s["rf"][k - 1], np.ascontiguousarray(s["cu"][k - 1]).reshape(-1))
    for step in range(2):
        pics = [mx.picture(s, k + step) for s, k in zip(seqs, first)]
        if step:
            ip.advance()
            for i, p in enumerate(pics):
                ip.upload_source(i, p["src"])
        table = _table(pics)
        assert len(set(table.qps.tolist())) == 3 and len(set(table.pocs.tolist())) == 2
        ip.run(prm, pictures=table)
        _assert_launch_equals_the_oracle(ip, pics)
        # the loop filters with the decisions brought back (InterPictures.loop_filters keeps them on the device)
        ip.d_dbk = ip.d_dbk or ip.dev.empty(n * ip.cells * 20)
        lib.kvz_hip_dev_cu_dbk_from_info(ip.d_cu, n * ip.cells, ip.d_dbk)
        luma, chroma, merge = np.zeros((n * ctus, 15), np.int32), np.zeros((n * ctus, 15), np.int32), np.zeros(n * ctus, np.uint8)
        rc = lib.kvz_hip_dev_loop_filters_inter_pictures(ip.d_src, ip.d_rec, w, h, n, ip.d_dbk, table.qps.ctypes.data, 1, 1, 0, 0, 1, 0, luma.ctypes.data, chroma.ctypes.data, merge.ctypes.data)
        assert rc == 0
        for i, p in enumerate(pics):
            where = (step, i, p["qp"], p["poc"])
            rec, _ = ip.download(i)
            assert np.array_equal(rec, p["final"]), where
            parts = p["seq"]["parts"]
            got = ec.pack_sao_records(np.ascontiguousarray(luma[i * ctus:(i + 1) * ctus]), np.ascontiguousarray(chroma[i * ctus:(i + 1) * ctus]), ctus)
            want = ec.pack_sao_records(np.ascontiguousarray(parts["sao_luma"][p["k"]]), np.ascontiguousarray(parts["sao_chroma"][p["k"]]), ctus)
            assert np.array_equal(got, want), where
            assert np.array_equal(merge[i * ctus:(i + 1) * ctus], parts["merge"][p["k"]]), where
        data, sizes = ip.entropy_code(prm, pictures=table)
        assert sizes.shape == (n, rows)
        mx.assert_slice_data(pics, data, sizes)
    ip.close()


def test_null_pictures_through_the_new_entry_points_is_the_old_entry_points(lib):
    """pictures == NULL: kvz_hip_dev_inter_ctu_pass_pictures and kvz_hip_dev_entropy_code_inter_pictures are kvz_hip_dev_inter_ctu_pass_tiles and
    kvz_hip_dev_entropy_code_inter, byte for byte (reconstruction, CU records, levels, slice data); the loop filters with a QP array that holds one QP are
    kvz_hip_dev_loop_filters_inter at that QP"""
    from kvazaar_amd import inter
    s = mx.sequence(27, seed=2)
    pics = [mx.picture(s, 2)] * 3
    w, h, n = mx.W, mx.H, len(pics)
    prm = mx.launch_params("veryfast")
    prm.qp, prm.poc = pics[0]["qp"], 2
    outs = []
    for new in (False, True):
        ip = _launch(lib, pics, with_levels=True)
        zeros = np.zeros(n * ip.ctus * 6144, np.int16)
        lib.kvz_hip_dev_upload(ip.d_coeff, zeros.ctypes.data, zeros.nbytes)
        if new:
            rc = lib.kvz_hip_dev_inter_ctu_pass_pictures(ip.d_src, ip.d_ref, ip.d_ref_cu, ip.d_rec, ip.d_cu, ip.d_coeff, w, h, n, C.addressof(prm), None, 0, None)
            assert rc == 0
        else:
            ip.run(prm)
        levels = ip.dev.get(ip.d_coeff, (n * ip.ctus * 6144,), np.int16)
        before = [ip.download(i) for i in range(n)]
        ip.loop_filters(prm, pictures=inter.InterPictureParams([prm.qp] * n, [2] * n) if new else None)
        after = [ip.download(i)[0] for i in range(n)]
        if new:
            sizes = np.zeros((n, (h + 63) // 64), np.uint32)
            from kvazaar_amd.batch import entropy_capacity, pinned_bytes, pinned_free
            cap = entropy_capacity(n, w, h)
            ptr, buf = pinned_bytes(lib, cap)
            total = lib.kvz_hip_dev_entropy_code_inter_pictures(ip.d_cu, ip.d_ref_cu, ip.d_coeff, w, h, n, C.addressof(prm), buf.ctypes.data, cap, sizes.ctypes.data, None)
            assert total >= 0
            data = bytes(buf[:total])
            pinned_free(lib, ptr)
        else:
            data, sizes = ip.entropy_code(prm)
            data = bytes(data)
        outs.append((levels, before, after, data, sizes.copy()))
        ip.close()
    (l0, b0, a0, d0, s0), (l1, b1, a1, d1, s1) = outs
    assert np.array_equal(l0, l1) and d0 == d1 and np.array_equal(s0, s1)
    for i in range(n):
        assert np.array_equal(b0[i][0], b1[i][0]) and b0[i][1].tobytes() == b1[i][1].tobytes() and np.array_equal(a0[i], a1[i]), i
    assert np.array_equal(a0[0], pics[0]["final"])  # ... and the oracle's picture


def test_refusals_return_minus_one_and_launch_nothing(lib, capfd):
    """a refused table: -1 and a message, and the output buffers are untouched"""
    from kvazaar_amd.inter import InterPictureParams, InterPicturesStruct
    pics = [mx.picture(mx.sequence(22, seed=1), 1)] * 2
    w, h, n = mx.W, mx.H, len(pics)
    prm = mx.launch_params("veryfast")
    ip = _launch(lib, pics, with_levels=True)
    mark = np.full(n * ip.fs, 0x5a, np.uint8)
    lib.kvz_hip_dev_upload(ip.d_rec, mark.ctypes.data, mark.nbytes)

    def table(qps=(23, 30), pocs=(1, 2), size=None, null=None):
        t = InterPictureParams(qps, pocs)
        if size is not None:
            t.struct.struct_size = size
        if null:
            setattr(t.struct, null, None)
        return t
    cases = [(table(size=C.sizeof(InterPicturesStruct) - 4), "struct_size"), (table(qps=(23, 30, 31), pocs=(1, 2, 3)), "n_pictures 3 is not the call's 2"), (table(null="qp"), "qp is NULL"),
             (table(null="poc"), "poc is NULL"), (table(qps=(23, 52)), "QP 52 outside 0..51"), (table(qps=(-1, 30)), "QP -1 outside 0..51"), (table(pocs=(1, 0)), "POC 0 below 1")]
    sizes = np.zeros((n, (h + 63) // 64), np.uint32)
    out = np.zeros(1 << 16, np.uint8)
    capfd.readouterr()
    for t, message in cases:
        rc = lib.kvz_hip_dev_inter_ctu_pass_pictures(ip.d_src, ip.d_ref, ip.d_ref_cu, ip.d_rec, ip.d_cu, ip.d_coeff, w, h, n, C.addressof(prm), None, 0, t.ptr)
        err = capfd.readouterr().err
        assert rc == -1 and message in err and "kvz_hip_dev_inter_ctu_pass_pictures" in err, (message, err)
        total = lib.kvz_hip_dev_entropy_code_inter_pictures(ip.d_cu, ip.d_ref_cu, ip.d_coeff, w, h, n, C.addressof(prm), out.ctypes.data, out.nbytes, sizes.ctypes.data, t.ptr)
        err = capfd.readouterr().err
        assert total == -1 and message in err and "kvz_hip_dev_entropy_code_inter_pictures" in err, (message, err)
    ip.d_dbk = ip.dev.empty(n * ip.cells * 20)
    for qps, message in ((None, "QP array is NULL"), (np.array([23, 52], np.int32), "QP 52 outside 0..51")):
        rc = lib.kvz_hip_dev_loop_filters_inter_pictures(ip.d_src, ip.d_rec, w, h, n, ip.d_dbk, qps.ctypes.data if qps is not None else None, 1, 1, 0, 0, 1, 0, None, None, None)
        err = capfd.readouterr().err
        assert rc == -1 and message in err and "kvz_hip_dev_loop_filters_inter_pictures" in err, (message, err)
    ip.sync()
    assert np.array_equal(ip.dev.get(ip.d_rec, (n * ip.fs,), np.uint8), mark) and not sizes.any() and not out.any()
    ip.close()
