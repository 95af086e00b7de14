"""Per-picture distortion on the MI355X: kvz_hip_dev_picture_sse against numpy, exact; the batch and inter chains against tests/golden/psnr.json (the reference
encoder's own sums and the PSNR text it printed, tests/golden/make_psnr_golden.py); the ordering of kvz_hip_batch_sse_async against
kvz_hip_batch_upload_all_async; bad arguments.  The host side is tests/test_psnr.py."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import ctu_common as cc
import inter_common as ic
from kvazaar_amd import dev as devapi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_psnr_golden as pg  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(HERE, "golden", "psnr.json")))


@pytest.fixture(scope="module")
def dev():
    import kvazaar_amd
    d = devapi.Dev(kvazaar_amd.load_library())
    d.lib.kvz_hip_dev_picture_sse.restype = C.c_int
    d.lib.kvz_hip_dev_picture_sse.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return d


def numpy_sse(a, b, w, h, n):
    """uint64 [n, 3], exact: a squared difference is at most 65 025 and a 3840x2160 plane has 8.3 M samples, 5.4e11 < 2^63"""
    fs, ys, cs = w * h * 3 // 2, w * h, w * h // 4
    out = np.zeros((n, 3), np.uint64)
    for f in range(n):
        d = a[f * fs:(f + 1) * fs].astype(np.int32) - b[f * fs:(f + 1) * fs].astype(np.int32)
        d *= d
        out[f] = [d[:ys].sum(dtype=np.int64), d[ys:ys + cs].sum(dtype=np.int64), d[ys + cs:].sum(dtype=np.int64)]
    return out


def device_sse(dev, a, b, w, h, n):
    da, db, do = dev.put(a), dev.put(b), dev.empty(24 * n)
    try:
        dev.copy_in(do, np.full(3 * n, 0xdeadbeefdeadbeef, np.uint64))  # the call zeroes what it adds into
        assert dev.lib.kvz_hip_dev_picture_sse(da, db, w, h, n, do) == 0
        return dev.get(do, (n, 3), np.uint64)
    finally:
        dev.free(da, db, do)


SIZES = [(8, 8), (64, 64), (264, 136), (416, 240), (1920, 1080), (3840, 2160)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("n", [1, 3, 130])
def test_dev_picture_sse_equals_numpy(dev, size, n):
    """random pairs, structured pairs (a ramp against its reverse: large differences with a pattern), identical inputs: integer for integer"""
    w, h = size
    fs = w * h * 3 // 2
    rng = np.random.default_rng(1000 * n + w)
    a = rng.integers(0, 256, n * fs, dtype=np.uint8)
    b = rng.integers(0, 256, n * fs, dtype=np.uint8)
    assert np.array_equal(device_sse(dev, a, b, w, h, n), numpy_sse(a, b, w, h, n))
    del b
    assert not device_sse(dev, a, a, w, h, n).any()
    del a
    ramp = np.resize((np.arange(251) * 7 % 256).astype(np.uint8), n * fs)  # (period 251: no plane starts where another does)
    back = ramp[::-1].copy()
    assert np.array_equal(device_sse(dev, ramp, back, w, h, n), numpy_sse(ramp, back, w, h, n))


def test_dev_picture_sse_beyond_32_bits(dev):
    """0 against 255 at 3840x2160: 5.4e11 in the luma plane"""
    w, h, n = 3840, 2160, 2
    fs = w * h * 3 // 2
    a, b = np.zeros(n * fs, np.uint8), np.full(n * fs, 255, np.uint8)
    got = device_sse(dev, a, b, w, h, n)
    assert got.tolist() == [[w * h * 65025, w * h // 4 * 65025, w * h // 4 * 65025]] * n
    assert int(got[0, 0]) > 2 ** 32


@pytest.mark.parametrize("size", [(8, 8), (264, 136), (1920, 1080)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_dev_picture_sse_ends_of_the_grid(dev, size):
    """a difference in the last byte of the last plane of the last picture only, and in the first byte of the first only"""
    w, h = size
    n, fs = 3, w * h * 3 // 2
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, n * fs, dtype=np.uint8)
    for at, where in ((n * fs - 1, (n - 1, 2)), (0, (0, 0))):
        b = a.copy()
        b[at] = np.uint8((int(a[at]) + 9) % 256)
        want = np.zeros((n, 3), np.uint64)
        want[where] = (int(a[at]) - int(b[at])) ** 2
        assert np.array_equal(device_sse(dev, a, b, w, h, n), want), at


def test_dev_picture_sse_bad_arguments(dev):
    """-1 and nothing launched: the output keeps its contents"""
    w, h, n = 64, 64, 2
    fs = w * h * 3 // 2
    a = np.arange(n * fs, dtype=np.int64).astype(np.uint8)
    da, db, do = dev.put(a), dev.put(a[::-1].copy()), dev.put(np.full(3 * n, 77, np.uint64))
    f = dev.lib.kvz_hip_dev_picture_sse
    try:
        for args in ((da, db, w, h, 0, do), (da, db, w, h, -1, do), (da, db, 60, h, n, do), (da, db, w, 60, n, do), (da, db, 0, h, n, do), (None, db, w, h, n, do),
                     (da, None, w, h, n, do), (da, db, w, h, n, None)):
            assert f(*args) == -1, args
        dev.lib.kvz_hip_dev_sync()
        assert (dev.get(do, (3 * n,), np.uint64) == 77).all()
        assert f(da, db, w, h, n, do) == 0  # ... and the same buffers in a good call
        assert np.array_equal(dev.get(do, (n, 3), np.uint64), numpy_sse(a, a[::-1], w, h, n))
    finally:
        dev.free(da, db, do)


def _intra_chain(b, model, clip, wait=True):
    name, w, h, n, seed, kind, qp, preset, deblock, sao = clip
    assert b.launch(model) >= 0
    if sao:
        b.loop_filters(model, deblock=bool(deblock), sao=True, wait=wait)
    elif deblock:
        b.deblock(qp, wait=wait)


@pytest.mark.parametrize("clip", pg.INTRA_CLIPS, ids=lambda c: c[0])
def test_batch_sse_and_psnr_are_the_reference_encoders(clip):
    """upload, kvz_hip_intra_frames, deblocking / loop filters as the clip says: HipBatch.sse() == the sums of the reference encoder's own files, and
    psnr_text(HipBatch.psnr()) == the text it printed"""
    import kvazaar_amd
    from kvazaar_amd.batch import HipBatch, cost_model
    lib = kvazaar_amd.load_library()
    name, w, h, n, seed, kind, qp, preset, deblock, sao = clip
    model = cost_model(lib, qp)
    b = HipBatch(lib, w, h, n)
    try:
        for i, f in enumerate(cc.yuv_frames(w, h, n, seed, kind)):
            b.upload(i, f)
        _intra_chain(b, model, clip)
        sse, psnr = b.sse(), b.psnr()
        assert sse.dtype == np.uint64 and sse.shape == (n, 3) and psnr.dtype == np.float64 and psnr.shape == (n, 3)
        for i in range(n):
            assert sse[i].tolist() == GOLDEN[name][str(i)]["sse"], (name, i)
            assert kvazaar_amd.psnr_text(psnr[i]) == GOLDEN[name][str(i)]["psnr_text"], (name, i)
            assert kvazaar_amd.psnr(sse[i][0], w * h) == psnr[i][0]
    finally:
        b.close()


@pytest.mark.parametrize("name", pg.LOWDELAY_CASES)
def test_inter_sse_and_psnr_are_the_reference_encoders(oracle, name):
    """the low-delay sequence picture after picture: the I picture through the batch (`veryfast`: deblocking + SAO), the B pictures through InterPictures (pass,
    loop_filters, sse() before advance()), each predicted from the device's own previous picture"""
    import kvazaar_amd
    from kvazaar_amd import inter
    from kvazaar_amd.batch import HipBatch, cost_model
    lib = kvazaar_amd.load_library()
    case = [c for c in ic.CASES if c[0] == name][0]
    _, w, h, n, qp, preset, dbk, sao, owf, _ = case
    assert preset == "veryfast" and dbk and sao
    frames = ic.case_frames(case)
    gold = GOLDEN["lowdelay-" + name]
    qps = [inter.lowdelay_picture_qp(qp, k) for k in range(n)]
    b = HipBatch(lib, w, h, 1)
    try:
        b.upload(0, frames[0])
        model = cost_model(lib, qps[0])
        b.run(model)
        b.loop_filters(model, deblock=True, sao=True)
        assert b.sse()[0].tolist() == gold["0"]["sse"]
        assert kvazaar_amd.psnr_text(b.psnr()[0]) == gold["0"]["psnr_text"]
        ref = b.download(0)["rec"]
    finally:
        b.close()
    # the I picture's CU records as the B picture's search reads them, from the oracle (the batch keeps depth / mode maps, not kvz_hip_cu_info)
    _, _, cu, oqps = ic.oracle_encode(oracle, w, h, frames, qp, preset=preset, deblock=True, sao=True, mv_constraint=owf > 0)
    assert [int(q) for q in oqps] == qps
    ip = inter.InterPictures(lib, w, h, 1)
    try:
        ip.upload(0, frames[1], ref, cu[0])
        for k in range(1, n):
            if k > 1:
                ip.upload_source(0, frames[k])
            prm = inter.veryfast_params(qps[k], k, mv_constraint=owf > 0)
            ip.run(prm)
            ip.loop_filters(prm)
            sse, psnr = ip.sse(), ip.psnr()
            assert sse.dtype == np.uint64 and sse.shape == (1, 3)
            assert sse[0].tolist() == gold[str(k)]["sse"], k
            assert kvazaar_amd.psnr_text(psnr[0]) == gold[str(k)]["psnr_text"], k
            ip.advance()
    finally:
        ip.close()


def test_sse_async_is_ordered_against_upload_all_async():
    """two picture sets A, B in pinned memory: chain on A, sse_async, upload_all_async(B) with no sync in between, chain again, sse_async again; after one sync the
    first result is A's and the second B's (a sum queued before an upload sees the old pictures, one queued after it the new ones)"""
    import kvazaar_amd
    from kvazaar_amd.batch import HipBatch, cost_model, pinned_bytes, pinned_free
    lib = kvazaar_amd.load_library()
    clip_a, clip_b = pg.INTRA_CLIPS[4], pg.INTRA_CLIPS[6]  # 416x240, two pictures each: ultrafast QP 32 with deblocking, veryfast QP 22 with deblocking + SAO
    (w, h, n), fs = clip_a[1:4], clip_a[1] * clip_a[2] * 3 // 2
    assert clip_b[1:4] == (w, h, n)
    ptrs = []
    b = HipBatch(lib, w, h, n)
    try:
        views = []
        for clip in (clip_a, clip_b):
            p, v = pinned_bytes(lib, n * fs)
            ptrs.append(p)
            v[:] = np.concatenate(cc.yuv_frames(w, h, n, clip[4], clip[5]))
            views.append(v)
        out_ptr, out_view = pinned_bytes(lib, 2 * n * 24)
        ptrs.append(out_ptr)
        out_view[:] = 0xee
        models = [cost_model(lib, clip_a[6]), cost_model(lib, clip_b[6])]
        b.upload_all_async(ptrs[0])
        _intra_chain(b, models[0], clip_a, wait=False)
        b.sse_async(out_ptr)
        b.upload_all_async(ptrs[1])
        _intra_chain(b, models[1], clip_b, wait=False)
        b.sse_async(out_ptr + n * 24)
        b.sync()
        got = np.frombuffer(out_view, np.uint64).reshape(2, n, 3)
        assert got[0].tolist() == [GOLDEN[clip_a[0]][str(i)]["sse"] for i in range(n)]
        assert got[1].tolist() == [GOLDEN[clip_b[0]][str(i)]["sse"] for i in range(n)]
        assert np.array_equal(b.sse(), got[1])  # the synchronous call on the state the chain left
    finally:
        b.close()
        for p in ptrs:
            pinned_free(lib, p)


def test_batch_sse_bad_arguments():
    import kvazaar_amd
    from kvazaar_amd.batch import HipBatch
    lib = kvazaar_amd.load_library()
    for f in (lib.kvz_hip_batch_sse, lib.kvz_hip_batch_sse_async):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p]
    out = np.zeros(3, np.uint64)
    b = HipBatch(lib, 64, 64, 1)
    try:
        assert lib.kvz_hip_batch_sse(None, out.ctypes.data) == -1 and lib.kvz_hip_batch_sse_async(None, out.ctypes.data) == -1
        assert lib.kvz_hip_batch_sse(b.handle, None) == -1 and lib.kvz_hip_batch_sse_async(b.handle, None) == -1
        b.sync()
    finally:
        b.close()
