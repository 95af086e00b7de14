"""The deblocking kernels on the MI355X (-m gpu) against the oracle, byte for byte on all three planes, on the inputs of tests/deblock_atlas.py -- whose census
(every filter path, per-line event and boundary-strength exit at least 16 times per direction) and whose sensitivity to one-token errors
tests/test_deblock_paths.py asserts without a GPU -- over every QP, and over every (beta, tc) offset pair where the device derives the thresholds itself."""
import ctypes as C

import numpy as np
import pytest

import deblock_atlas as atlas
import deblock_common as dc
import test_deblock_inter as tdi

pytestmark = pytest.mark.gpu

W, H = 72, 72  # the inter launches: 9x9 units, ragged chroma part counts, partial CTUs
FRAME = W * H * 3 // 2
I, VP = C.c_int, C.c_void_p


@pytest.fixture(scope="module")
def dev():
    import kvazaar_amd
    from kvazaar_amd.dev import Dev
    d = Dev(kvazaar_amd.load_library())
    lib = d.lib
    lib.kvz_hip_dev_deblock_frames.restype = None
    lib.kvz_hip_dev_deblock_frames.argtypes = [VP, I, I, I, VP, I, I, I]
    lib.kvz_hip_dev_deblock_frames_inter.restype = None
    lib.kvz_hip_dev_deblock_frames_inter.argtypes = [VP, I, I, I, VP, I, I, I, I]
    lib.kvz_hip_dev_loop_filters_inter.restype = I
    lib.kvz_hip_dev_loop_filters_inter.argtypes = [VP, VP, I, I, I, VP] + [I] * 7 + [VP] * 3
    lib.kvz_hip_dev_loop_filters_inter_pictures.restype = I
    lib.kvz_hip_dev_loop_filters_inter_pictures.argtypes = [VP, VP, I, I, I, VP, VP] + [I] * 6 + [VP] * 3
    return d


def differences(got, want):
    return np.flatnonzero(got != want)[:8]


# ---- (a) all-intra pictures, thresholds from the host -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", atlas.GEOMETRIES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_deblock_frames_every_qp_and_corner(oracle, dev, size):
    """kvz_hip_dev_deblock_frames on the atlas batch of a geometry: 2 - 4 workgroups per kernel, the last one ragged, parts of two pictures in one workgroup"""
    w, h = size
    pics = atlas.pictures(w, h)
    frames, depths = np.stack([f for f, _ in pics]), np.stack([d for _, d in pics])
    d_fr, d_dp = dev.empty(frames.nbytes), dev.put(depths)
    for b_off, t_off in [(0, 0)] + atlas.CORNERS:
        for qp in range(52):
            dev.copy_in(d_fr, frames)
            dev.lib.kvz_hip_dev_deblock_frames(d_fr, w, h, len(pics), d_dp, qp, b_off, t_off)
            got = dev.get(d_fr, frames.shape, np.uint8)
            for i, (f, d) in enumerate(pics):
                want = dc.run_cpu(oracle.lib.kvz_oracle_deblock_frame, w, h, qp, b_off, t_off, f, d)
                assert np.array_equal(got[i], want), (i, qp, b_off, t_off, differences(got[i], want))
    dev.free(d_fr, d_dp)


# ---- (b) a QP per picture: the thresholds derived on the device ---------------------------------------------------------------------------------------------------
class Launch:
    """the 52 pictures of deblock_atlas.launch_of_52 on the device: picture i at QP i"""

    def __init__(self, dev, kind):
        self.dev, self.kind, self.slice_b = dev, kind, int(kind == "B")
        frames, self.records, self.depths = atlas.launch_of_52(W, H, kind)
        self.frames = np.stack(frames)
        blob = b"".join(bytes(r) for r in self.records)
        self.d_info = dev.empty(len(blob))
        dev.lib.kvz_hip_dev_upload(self.d_info, blob, len(blob))
        self.d_src, self.d_rec = dev.put(self.frames), dev.empty(self.frames.nbytes)  # src: unused without SAO, but not NULL
        self.qps = np.arange(52, dtype=np.int32)

    def per_picture(self, b_off, t_off, qps=None, width=W):
        self.dev.copy_in(self.d_rec, self.frames)
        qps = self.qps if qps is None else qps
        rc = self.dev.lib.kvz_hip_dev_loop_filters_inter_pictures(self.d_src, self.d_rec, width, H, 52, self.d_info, qps.ctypes.data, self.slice_b, 1, b_off, t_off, 0, 0,
                                                                  None, None, None)
        return rc, self.dev.get(self.d_rec, self.frames.shape, np.uint8)

    def oracle(self, oracle, i, qp, b_off, t_off):
        return tdi.run(oracle.lib.kvz_oracle_deblock_frame_inter, W, H, qp, b_off, t_off, self.frames[i], self.records[i], self.slice_b)

    def close(self):
        self.dev.free(self.d_info, self.d_src, self.d_rec)


@pytest.fixture(scope="module", params=["intra", "P", "B"])
def launch(request, dev):
    l = Launch(dev, request.param)
    yield l
    l.close()


def test_loop_filters_inter_pictures_every_offset_pair(oracle, launch):
    """kvz_hip_dev_loop_filters_inter_pictures(deblock = 1, sao = 0): 169 launches of 52 pictures; tc at strength 1 and 2, beta and the chroma tc meet every
    table index and both clips of either index"""
    for b_off in range(-6, 7):
        for t_off in range(-6, 7):
            rc, got = launch.per_picture(b_off, t_off)
            assert rc == 0
            for i in range(52):
                want = launch.oracle(oracle, i, i, b_off, t_off)
                assert np.array_equal(got[i], want), (launch.kind, i, b_off, t_off, differences(got[i], want))
                if launch.kind == "intra":  # records derived from a depth map filter like the map itself
                    want = dc.run_cpu(oracle.lib.kvz_oracle_deblock_frame, W, H, i, b_off, t_off, launch.frames[i], launch.depths[i])
                    assert np.array_equal(got[i], want), ("depth map", i, b_off, t_off, differences(got[i], want))


# ---- (c) the uniform-QP entry points ------------------------------------------------------------------------------------------------------------------------------
def test_uniform_qp_entry_points_every_qp(oracle, launch, dev):
    """kvz_hip_dev_deblock_frames_inter and kvz_hip_dev_loop_filters_inter(sao = 0) at every QP: the oracle's pictures, and picture qp of the per-picture launch"""
    rc, mixed = launch.per_picture(0, 0)
    assert rc == 0
    for qp in range(52):
        want = [launch.oracle(oracle, i, qp, 0, 0) for i in range(52)]
        dev.copy_in(launch.d_rec, launch.frames)
        dev.lib.kvz_hip_dev_deblock_frames_inter(launch.d_rec, W, H, 52, launch.d_info, qp, 0, 0, launch.slice_b)
        a = dev.get(launch.d_rec, launch.frames.shape, np.uint8)
        dev.copy_in(launch.d_rec, launch.frames)
        assert dev.lib.kvz_hip_dev_loop_filters_inter(launch.d_src, launch.d_rec, W, H, 52, launch.d_info, qp, launch.slice_b, 1, 0, 0, 0, 0, None, None, None) == 0
        b = dev.get(launch.d_rec, launch.frames.shape, np.uint8)
        for i in range(52):
            assert np.array_equal(a[i], want[i]), ("deblock_frames_inter", launch.kind, qp, i, differences(a[i], want[i]))
            assert np.array_equal(b[i], want[i]), ("loop_filters_inter", launch.kind, qp, i, differences(b[i], want[i]))
        assert np.array_equal(a[qp], mixed[qp]) and np.array_equal(b[qp], mixed[qp]), (launch.kind, qp)


# ---- (d) refusals -------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_pictures_alone(launch):
    """a QP outside 0 .. 51 in qp_of_picture and a width that is no multiple of 8: -1 before anything is queued"""
    for bad in (52, -1):
        for at in (0, 51):
            qps = launch.qps.copy()
            qps[at] = bad
            rc, after = launch.per_picture(0, 0, qps=qps)
            assert rc == -1 and np.array_equal(after, launch.frames), (bad, at)
    rc, after = launch.per_picture(0, 0, width=68)
    assert rc == -1 and np.array_equal(after, launch.frames)
    rc, after = launch.per_picture(0, 0)  # and the same arguments without the fault are taken
    assert rc == 0 and not np.array_equal(after, launch.frames)
