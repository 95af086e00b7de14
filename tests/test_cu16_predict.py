"""Stage 1's luma prediction of a 16x16 CU's reconstruction in the intra CTU pass (kvz_ctu.hpp recon_cu16: 64 lanes, a row segment of four samples each, modes 11..25
from the extended references the CU's rough search built) against the oracle's intra prediction, exactly: every mode 0..34 -- the pass-level tests only see the modes
that win -- on six reference sets (seeded random, flat 128, a ramp, all 0, all 255, and one whose unavailable sides were substituted as intra.c:305-425 does), one
16x16 block each.  On the CPU through the serial host twin (tests/hostsim/hostsim_cu16_predict.cpp), on the device through kvz_hip_dev_cu16_predict in one launch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flatapi
import rough_rows_common as rr

W, N = 16, 33
SETS = ("random", "flat128", "ramp", "all0", "all255", "substituted")
_CASES, _WANT = [], []


def cases():
    """(top, left, modes): [35 x 6][N + PAD] unfiltered references, the corner shared, and the mode of each"""
    if not _CASES:
        rng = np.random.default_rng(1604)
        i = np.arange(N)
        sets = {"random": (rng.integers(0, 256, N, dtype=np.uint8), rng.integers(0, 256, N, dtype=np.uint8)),
                "flat128": (np.full(N, 128, np.uint8), np.full(N, 128, np.uint8)),
                "ramp": (np.clip(100 + 5 * i, 0, 255).astype(np.uint8), np.clip(100 - 4 * i, 0, 255).astype(np.uint8)),
                "all0": (np.zeros(N, np.uint8), np.zeros(N, np.uint8)),
                "all255": (np.full(N, 255, np.uint8), np.full(N, 255, np.uint8))}
        # a CU on the picture's left edge whose above-right neighbour is not coded yet: the left side and the corner are the sample above the CU's first column,
        # the above-right half repeats the last sample above the CU
        t = rng.integers(0, 256, N, dtype=np.uint8)
        t[W + 1:] = t[W]
        t[0] = t[1]
        sets["substituted"] = (t, np.full(N, t[1], np.uint8))
        tops, lefts, modes = [], [], []
        for name in SETS:
            top, left = (a.copy() for a in sets[name])
            left[0] = top[0]
            for mode in range(35):
                tops.append(np.concatenate([top, np.zeros(rr.PAD, np.uint8)]))
                lefts.append(np.concatenate([left, np.zeros(rr.PAD, np.uint8)]))
                modes.append(mode)
        _CASES.extend([np.ascontiguousarray(np.array(tops)), np.ascontiguousarray(np.array(lefts)), np.array(modes, np.uint8)])
        for a in _CASES:
            a.setflags(write=False)
    return _CASES


def oracle_blocks(oracle):
    """[35 x 6][16][16]: kvz_intra_predict for luma (intra.c:252-301) -- the filtered or unfiltered references (intra.c:262-281), the oracle's planar, filtered DC and
    angular predictions, intra_post_process_angular (intra.c:207-219).  Computed once and left unchanged."""
    if not _WANT:
        tops, lefts, modes = cases()
        want = np.empty((len(modes), W, W), np.uint8)
        dst = np.zeros(W * W, np.uint8)
        for i, mode in enumerate(int(m) for m in modes):
            reads_filtered = mode != 1 and rr.reads_filtered(4, mode)  # (planar does, DC never: intra.c:262-281)
            t, l = rr.filtered(tops[i], lefts[i], N) if reads_filtered else (tops[i].copy(), lefts[i].copy())
            if mode == 0:
                oracle.intra_pred_planar(4, flatapi.ptr(t), flatapi.ptr(l), flatapi.ptr(dst))
            elif mode == 1:
                oracle.intra_pred_filtered_dc(4, flatapi.ptr(t), flatapi.ptr(l), flatapi.ptr(dst))
            else:
                oracle.angular_pred(4, mode, flatapi.ptr(t), flatapi.ptr(l), flatapi.ptr(dst))
            pred = dst.reshape(W, W).astype(np.int32)
            if mode == 10:
                pred[0, :] = np.clip(pred[0, :] + ((t[1:W + 1].astype(np.int32) - int(t[0])) >> 1), 0, 255)
            if mode == 26:
                pred[:, 0] = np.clip(pred[:, 0] + ((l[1:W + 1].astype(np.int32) - int(l[0])) >> 1), 0, 255)
            want[i] = pred.astype(np.uint8)
        want.setflags(write=False)
        _WANT.append(want)
    return _WANT[0]


def compare(got, want):
    """every sample of every block; returns the (row, first sample) of every four-sample segment that was compared"""
    assert got.shape == want.shape == (35 * len(SETS), W, W)
    segments = set()
    bad = []
    for py in range(W):
        for px0 in range(0, W, 4):
            differs = (got[:, py, px0:px0 + 4] != want[:, py, px0:px0 + 4]).any(axis=1)
            bad += [(SETS[i // 35], i % 35, py, px0) for i in np.flatnonzero(differs)]
            segments.add((py, px0))
    assert not bad, bad[:8]  # (set, mode, row, first sample of the segment)
    return segments


ALL_SEGMENTS = {(py, px0) for py in range(W) for px0 in (0, 4, 8, 12)}


@pytest.fixture(scope="module")
def sim():
    """tests/hostsim/libkvz_hostsim_cu16_predict.so, built with the recipe of the other host simulations when it is missing or older than a source"""
    d, csrc = os.path.join(flatapi.ROOT, "tests", "hostsim"), os.path.join(flatapi.ROOT, "kvazaar_amd", "csrc")
    so = os.path.join(d, "libkvz_hostsim_cu16_predict.so")
    srcs = [os.path.join(d, "hostsim_cu16_predict.cpp"), os.path.join(flatapi.ROOT, "include", "kvz_hip_types.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = os.path.join(d, f".libkvz_hostsim_cu16_predict.{os.getpid()}.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp, os.path.join(d, "hostsim_cu16_predict.cpp")])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.kvz_hostsim_cu16_predict.restype = C.c_int
    lib.kvz_hostsim_cu16_predict.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def test_the_sets_are_what_they_are_meant_to_be():
    tops, lefts, modes = cases()
    assert len(modes) == 35 * len(SETS) and sorted(set(int(m) for m in modes)) == list(range(35))
    assert all(sorted(int(m) for m in modes[35 * k:35 * k + 35]) == list(range(35)) for k in range(len(SETS)))
    assert (tops[:, 0] == lefts[:, 0]).all() and (tops[:, N:] == 0).all()
    s = SETS.index("substituted") * 35
    assert (lefts[s, :N] == tops[s, 1]).all() and (tops[s, W + 1:N] == tops[s, W]).all() and len(set(tops[s, 1:W + 1].tolist())) > 8


def test_host_twin_equals_the_oracle_prediction(oracle, sim):
    tops, lefts, modes = cases()
    want = oracle_blocks(oracle)
    t, l = np.ascontiguousarray(tops[:, :N]), np.ascontiguousarray(lefts[:, :N])
    got = np.full(want.size + 64, 0xA5, np.uint8)
    covered = np.zeros(want.size, np.uint8)
    assert sim.kvz_hostsim_cu16_predict(t.ctypes.data, l.ctypes.data, modes.ctypes.data, len(modes), got.ctypes.data, covered.ctypes.data) == 0
    assert (got[want.size:] == 0xA5).all()
    assert (covered == 1).all()  # 64 lanes of four samples tile the block: every sample written once
    assert compare(got[:want.size].reshape(want.shape), want) == ALL_SEGMENTS
    assert sim.kvz_hostsim_cu16_predict(t.ctypes.data, l.ctypes.data, modes.ctypes.data, -1, got.ctypes.data, None) == -1


@pytest.mark.gpu
def test_device_equals_the_oracle_prediction(oracle):
    import kvazaar_amd
    from kvazaar_amd import dev as devapi
    dev = devapi.Dev(kvazaar_amd.load_library())
    tops, lefts, modes = cases()
    want = oracle_blocks(oracle)
    count = len(modes)
    bufs = [dev.put(tops[:, :N]), dev.put(lefts[:, :N]), dev.put(modes), dev.put(np.full(want.size + 256, 0xA5, np.uint8))]
    try:
        assert dev.lib.kvz_hip_dev_cu16_predict(bufs[0], bufs[1], bufs[2], count, bufs[3]) == 0  # one launch
        got = dev.get(bufs[3], (count + 1, W, W), np.uint8)
        assert (got[count] == 0xA5).all()  # nothing written past the last CU
        assert compare(got[:count], want) == ALL_SEGMENTS
        # an odd number of CUs: the last workgroup is half filled
        assert dev.lib.kvz_hip_dev_cu16_predict(bufs[0], bufs[1], bufs[2], count - 1, bufs[3]) == 0
        again = dev.get(bufs[3], (count + 1, W, W), np.uint8)
        assert np.array_equal(again, got)
        assert dev.lib.kvz_hip_dev_cu16_predict(bufs[0], bufs[1], bufs[2], -1, bufs[3]) == -1 and dev.lib.kvz_hip_dev_cu16_predict(bufs[0], bufs[1], bufs[2], 0, bufs[3]) == 0
    finally:
        dev.free(*bufs)
