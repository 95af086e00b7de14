"""The SAO kernels on the MI355X (-m gpu) against the oracle: dev_sao_stats_kernel, dev_sao_chain_kernel and dev_sao_kernel<TAIL> through
kvz_hip_dev_loop_filters_inter and its _pictures and _slices twins, which decide and apply SAO on exactly the (source, reconstruction) pair they are given -- luma
and chroma parameters, merge flags and output pictures, on the inputs of tests/sao_atlas.py, whose census (every branch of the decision and of the filter at least
16 times), whose sensitivity to the R / V / D view and to one-token errors tests/test_sao_paths.py asserts without a GPU, where the oracle is also held against
a statement in plain Python.  The filter alone (kvz_hip_dev_sao_frames, parameter structures instead of packed records) runs at every width residue mod 32.

Out of scope: kvz_hip_batch_loop_filters and its _models twin cannot take an injected reconstruction; they run the same three kernels and stay covered by the
encoder clips of tests/test_sao_decision.py and tests/test_gpu_mixed_qp.py."""
import ctypes as C

import numpy as np
import pytest

import sao_atlas as atlas
import sao_common as sc
import sao_reference as sr
import test_sao_paths as tsp
from flatapi import SaoParams

pytestmark = pytest.mark.gpu

I, VP = C.c_int, C.c_void_p
N = atlas.LAUNCH  # pictures of a launch: picture i at QP i % 52; more than 64 put work into the chain kernel's second workgroup
SLICE_B, SLICE_P, SLICE_I = 0, 1, 2  # KVZ_HIP_SLICE_* (include/kvz_hip_types.h) = sao_reference's numbering
IDS = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


@pytest.fixture(scope="module")
def dev():
    import kvazaar_amd
    from kvazaar_amd.dev import Dev
    d = Dev(kvazaar_amd.load_library())
    lib = d.lib
    lib.kvz_hip_dev_loop_filters_inter.restype = I
    lib.kvz_hip_dev_loop_filters_inter.argtypes = [VP, VP, I, I, I, VP] + [I] * 7 + [VP] * 3
    lib.kvz_hip_dev_loop_filters_inter_pictures.restype = I
    lib.kvz_hip_dev_loop_filters_inter_pictures.argtypes = [VP, VP, I, I, I, VP, VP] + [I] * 6 + [VP] * 3
    lib.kvz_hip_dev_loop_filters_inter_slices.restype = I
    lib.kvz_hip_dev_loop_filters_inter_slices.argtypes = [VP, VP, I, I, I, VP, I, VP] + [I] * 6 + [VP] * 3
    lib.kvz_hip_dev_sao_frames.restype = None
    lib.kvz_hip_dev_sao_frames.argtypes = [VP, VP, I, I, I, VP, VP]
    return d


def differences(got, want):
    return np.flatnonzero(got != want)[:8]


_oracle = {}


def expected(oracle, w, h, j, qp, slice_type, no_wpp, deblock):
    """the oracle's (records, merge flags, final picture) of atlas picture j; computed once, shared by every test of the module"""
    key = (w, h, j, qp, slice_type, no_wpp, deblock)
    if key not in _oracle:
        src, rec, depth = atlas.pictures(w, h)[j]
        _oracle[key] = tsp.oracle_decide(oracle, tsp.model_of(oracle, qp, slice_type, no_wpp), w, h, src, rec, depth, deblock)
    return _oracle[key]


class Launch:
    """n pictures of one geometry on the device, cycling through the atlas pictures as sao_atlas.launch_content says for a slice type and WPP setting"""

    def __init__(self, dev, w, h, n=N, slice_b=0, no_wpp=0):
        pics = atlas.pictures(w, h)
        self.dev, self.w, self.h, self.n, self.lcus = dev, w, h, n, tsp.lcus_of(w, h)
        self.content = atlas.launch_content(n, slice_b, no_wpp)
        self.src, self.rec = np.stack([pics[j][0] for j in self.content]), np.stack([pics[j][1] for j in self.content])
        blob = b"".join(bytes(atlas.records_from_depth(w, h, pics[j][2])) for j in self.content)
        self.d_info = dev.empty(len(blob))
        dev.lib.kvz_hip_dev_upload(self.d_info, blob, len(blob))
        self.d_src, self.d_rec = dev.put(self.src), dev.empty(self.rec.nbytes)
        self.qps = np.arange(n, dtype=np.int32) % 52

    def run(self, entry, deblock, no_wpp, slice_type=SLICE_B, qp=None, want=(1, 1, 1)):
        """entry: "pictures" (a QP per picture), "uniform" (qp), "slices" (slice_type; qp or a QP per picture) -> (rc, records per picture, merge per picture, pictures);
        want: which of the luma / chroma / merge outputs are asked for (the others go in as NULL; their records come back all zero, their merge flags as None)"""
        lib, count = self.dev.lib, self.n * self.lcus
        luma, chroma, merge = (SaoParams * count)(), (SaoParams * count)(), np.zeros(count, np.uint8)
        outs = [luma if want[0] else None, chroma if want[1] else None, merge.ctypes.data if want[2] else None]
        self.dev.copy_in(self.d_rec, self.rec)
        head = (self.d_src, self.d_rec, self.w, self.h, self.n, self.d_info)
        if entry == "pictures":
            rc = lib.kvz_hip_dev_loop_filters_inter_pictures(*head, self.qps.ctypes.data, int(slice_type == SLICE_B), deblock, 0, 0, 1, no_wpp, *outs)
        elif entry == "uniform":
            rc = lib.kvz_hip_dev_loop_filters_inter(*head, qp, int(slice_type == SLICE_B), deblock, 0, 0, 1, no_wpp, *outs)
        else:
            rc = lib.kvz_hip_dev_loop_filters_inter_slices(*head, 0 if qp is None else qp, self.qps.ctypes.data if qp is None else None, slice_type, deblock, 0, 0, 1, no_wpp, *outs)
        pictures = self.dev.get(self.d_rec, self.rec.shape, np.uint8)
        recs = tsp.records_of(luma, chroma)  # (an output that went in as NULL stays all zero here)
        k = self.lcus
        return (rc, [recs[i * k:(i + 1) * k] for i in range(self.n)], [[int(v) for v in merge[i * k:(i + 1) * k]] for i in range(self.n)] if want[2] else None, pictures)

    def check(self, oracle, got, slice_type, no_wpp, deblock, qp=None, label=""):
        rc, recs, merge, pictures = got
        assert rc == 0
        for i in range(self.n):
            q = int(self.qps[i]) if qp is None else qp
            w_recs, w_merge, w_final = expected(oracle, self.w, self.h, self.content[i], q, slice_type, no_wpp, deblock)
            where = (label, i, q, self.content[i])
            assert merge[i] == w_merge, where
            assert [r[0] for r in recs[i]] == [r[0] for r in w_recs], ("luma",) + where
            assert [r[1:] for r in recs[i]] == [r[1:] for r in w_recs], ("chroma",) + where
            assert np.array_equal(pictures[i], w_final), where + (differences(pictures[i], w_final),)

    def close(self):
        self.dev.free(self.d_info, self.d_src, self.d_rec)


# ---- (a) every QP in one launch ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deblock", [0, 1], ids=["plain", "deblocked"])
@pytest.mark.parametrize("slice_b", [0, 1], ids=["I", "B"])
@pytest.mark.parametrize("size", atlas.GEOMETRIES, ids=IDS)
def test_every_qp_in_one_launch(oracle, dev, size, slice_b, deblock):
    """kvz_hip_dev_loop_filters_inter_pictures on 104 pictures, picture i at QP i % 52, WPP on and off: every row of the QP table (lambda, both initial states) of
    either slice type, two workgroups of the chain kernel; between the slice types and WPP settings every atlas picture meets every QP.  These launches are
    sao_atlas.launch_cases(), the list the census of tests/test_sao_paths.py is counted over"""
    slice_type = SLICE_B if slice_b else SLICE_I
    for no_wpp in (0, 1):
        launch = Launch(dev, *size, slice_b=slice_b, no_wpp=no_wpp)
        try:
            launch.check(oracle, launch.run("pictures", deblock, no_wpp, slice_type), slice_type, no_wpp, deblock, label=("no_wpp", no_wpp))
        finally:
            launch.close()


# ---- (b) the uniform-QP entry point --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(136, 72), (72, 72)], ids=IDS)
def test_uniform_qp_entry_point_every_qp(oracle, dev, size):
    """kvz_hip_dev_loop_filters_inter at every QP on the atlas pictures: the oracle's decisions and pictures, and what picture q of the per-picture launch gave"""
    pics = len(atlas.pictures(*size))
    mixed, uniform = Launch(dev, *size), Launch(dev, *size, n=pics)
    try:
        _, m_recs, m_merge, m_pictures = got = mixed.run("pictures", 1, 0)
        mixed.check(oracle, got, SLICE_B, 0, 1)
        for qp in range(52):
            _, recs, merge, pictures = got = uniform.run("uniform", 1, 0, qp=qp)
            uniform.check(oracle, got, SLICE_B, 0, 1, qp=qp)
            for i in (qp, qp + 52):
                j = mixed.content[i]
                assert recs[j] == m_recs[i] and merge[j] == m_merge[i] and np.array_equal(pictures[j], m_pictures[i]), (qp, i)
    finally:
        mixed.close()
        uniform.close()


# ---- (c) P slices ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", atlas.GEOMETRIES, ids=IDS)
def test_p_slices_every_qp(oracle, dev, size):
    """kvz_hip_dev_loop_filters_inter_slices with KVZ_HIP_SLICE_P: the type context starts from 185; a QP per picture, and the scalar QP at both ends"""
    launch = Launch(dev, *size)
    try:
        for deblock in (0, 1):
            launch.check(oracle, launch.run("slices", deblock, 0, SLICE_P), SLICE_P, 0, deblock, label=("deblock", deblock))
        for qp in (0, 51):
            launch.check(oracle, launch.run("slices", 1, 1, SLICE_P, qp=qp), SLICE_P, 1, 1, qp=qp, label="scalar")
    finally:
        launch.close()


# ---- (d) outputs that are not asked for ------------------------------------------------------------------------------------------------------------------------------
def test_null_outputs_leave_the_picture_alone(oracle, dev):
    """luma, chroma and merge each NULL in turn, and all three: the same pictures, and the same decisions in every output that is still returned"""
    launch = Launch(dev, 136, 72)
    try:
        _, recs, merge, pictures = launch.run("pictures", 1, 0)
        assert any(r[0][0] for p in recs for r in p) and any(r[1][0] for p in recs for r in p)  # (a zeroed array would not pass for either output)
        for want in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)):
            rc, r, m, p = launch.run("pictures", 1, 0, want=want)
            assert rc == 0 and np.array_equal(p, pictures), want
            if want[0]:
                assert [[lcu[0] for lcu in pic] for pic in r] == [[lcu[0] for lcu in pic] for pic in recs], ("luma", want)
            if want[1]:
                assert [[lcu[1:] for lcu in pic] for pic in r] == [[lcu[1:] for lcu in pic] for pic in recs], ("chroma", want)
            if want[2]:
                assert m == merge, want
    finally:
        launch.close()


# ---- (e) the filter alone: kvz_hip_dev_sao_frames ------------------------------------------------------------------------------------------------------------------
FILTER_SIZES = atlas.GEOMETRIES + [(96, 64), (120, 72)]  # widths 0, 8, 8, 0, 24, 16, 0, 24 mod 32 -- with 72 and 136 = 8 mod 32 of two lengths; see below


def run_sao_frames(dev, oracle, w, h, frames, lumas, chromas, python=()):
    din, dout = dev.put(frames), dev.empty(frames.nbytes)
    dl = dev.put(np.frombuffer(b"".join(bytes(x) for x in lumas), dtype=np.uint8))
    dc_ = dev.put(np.frombuffer(b"".join(bytes(x) for x in chromas), dtype=np.uint8))
    dev.lib.kvz_hip_dev_sao_frames(din, dout, w, h, len(frames), dl, dc_)
    got = dev.get(dout, frames.shape, np.uint8)
    dev.free(din, dout, dl, dc_)
    for f in range(len(frames)):
        want = sc.run_cpu(oracle.lib.kvz_oracle_sao_frame, w, h, frames[f], lumas[f], chromas[f])
        assert np.array_equal(got[f], want), (f, differences(got[f], want))
        if f in python:  # and the plain statement of 8.7.3 (positions up to 27: beyond, the standard's band table wraps and the encoder's does not)
            assert np.array_equal(got[f], sr.apply(w, h, frames[f], tsp.records_of(lumas[f], chromas[f]))), ("python", f)


def test_filter_sizes_cover_every_row_tail():
    """the kernel's TAIL build moves a row's last lane as 1, 2 or 3 dwords: 4 x dwords = plane width mod 16.  Luma widths are multiples of 8 (0 or 2 dwords),
    chroma widths multiples of 4"""
    tails = {(w % 16 // 4, (w // 2) % 16 // 4) for w, _ in FILTER_SIZES}
    assert {t[1] for t in tails} == {0, 1, 2, 3} and (0, 2) in tails and (2, 3) in tails and (2, 1) in tails and {w % 32 for w, _ in FILTER_SIZES} == {0, 8, 16, 24}


@pytest.mark.parametrize("size", FILTER_SIZES, ids=IDS)
def test_sao_frames_random_parameters_every_band_position(oracle, dev, size):
    """random bytes, random per-CTU parameters with band positions 0 .. 31 (a band record then covers fewer than four bands at the top of the range)"""
    w, h = size
    rng = np.random.default_rng(5 * w + h)
    nf, n = 32, tsp.lcus_of(w, h)
    frames = rng.integers(0, 256, (nf, w * h * 3 // 2), dtype=np.uint8)
    lumas, chromas = [sc.random_params(rng, n, False, band_positions=32) for _ in range(nf)], [sc.random_params(rng, n, True, band_positions=32) for _ in range(nf)]
    for f in range(nf):  # every position is met in every plane, whatever the draws: the first CTU of frame f
        lumas[f][0].type = chromas[f][0].type = 1
        lumas[f][0].band_position[0], chromas[f][0].band_position[0], chromas[f][0].band_position[1] = f, 31 - f, (7 * f + 5) % 32
    run_sao_frames(dev, oracle, w, h, frames, lumas, chromas)


@pytest.mark.parametrize("size", FILTER_SIZES, ids=IDS)
def test_sao_frames_saturated_planes_and_a_class_per_ctu(oracle, dev, size):
    """offsets of +-7 on samples within 7 of 0 (odd frames) and of 255 (even frames): both clips of the packed add.  Frames 0 .. 7: edge records, CTU (x, y) under
    class (x + y + f // 2) % 4 -- every CTU under every class at both ends of the range, so each class at each picture border and each row-tail length; frames
    8 and 9: band records in every CTU and plane, +7 on bands 28 .. 31 and -7 on bands 0 .. 3"""
    w, h = size
    rng = np.random.default_rng(9 * w + h)
    n, wl = tsp.lcus_of(w, h), (w + 63) // 64
    frames, lumas, chromas = [], [], []
    for f in range(10):
        low = rng.integers(0, 8, w * h * 3 // 2)
        frames.append((low if f & 1 else 255 - low).astype(np.uint8))
        arrays = (SaoParams * n)(), (SaoParams * n)()
        for arr in arrays:
            for i, p in enumerate(arr):
                p.bitdepth, p.eo_class, p.type = 8, (i % wl + i // wl + f // 2) % 4, (2 if f < 8 else 1)
                p.band_position[0], p.band_position[1] = (0, 0) if f & 1 else (28, 28)  # bands 28 .. 31 hold 224 .. 255
                for k in range(10):
                    p.offsets[k] = 0 if k % 5 == 0 else ((-7 if f & 1 else 7) if p.type == 1 else (7 if k % 5 <= 2 else -7))
        lumas.append(arrays[0])
        chromas.append(arrays[1])
    run_sao_frames(dev, oracle, w, h, np.stack(frames), lumas, chromas)


@pytest.mark.parametrize("size", FILTER_SIZES, ids=IDS)
def test_sao_frames_equal_python_statement(oracle, dev, size):
    """band positions an encoder can code (0 .. 27; offsets of any sign) on noise: the device, the oracle and the Python statement of 8.7.3"""
    w, h = size
    rng = np.random.default_rng(13 * w + h)
    n = tsp.lcus_of(w, h)
    frames = rng.integers(0, 256, (2, w * h * 3 // 2), dtype=np.uint8)
    lumas, chromas = [sc.random_params(rng, n, False, band_positions=28) for _ in range(2)], [sc.random_params(rng, n, True, band_positions=28) for _ in range(2)]
    for arr in chromas:  # the statement's chroma records share type and class, as the syntax does; nothing else is constrained
        for p in arr:
            p.band_position[1] = int(rng.integers(0, 28))
    run_sao_frames(dev, oracle, w, h, frames, lumas, chromas, python=(0, 1))
