"""Stages 2-5 of the 8x8 CU's reconstruction at the extremes of their arithmetic, which pictures cannot reach.  The stages are functions of kvz_recon.hpp (cu8_matrix_rows,
cu8_fwd_first / _second, cu8_inv_first / _second, cu8_transposed: a lane's inputs as one row of int16 pairs against its matrix row, the inverse path on transposed
intermediates) that kvz_ctu.hpp recon_cu8 calls; the same functions run here on blocks without a picture -- serially on the host (tests/hostsim/hostsim_cu8.cpp) and,
under -m gpu, on the device in recon_cu8's lane roles (kvz_hip_dev_cu8_units, v_dot2_i32_i16) -- against the per-call oracle's dct -> quant -> dequant -> idct (pinned
to the compiled reference by tests/test_oracle_vs_ref.py).  What these tests do not run is recon_cu8's own text around the calls -- which buffer a stage reads and
writes, prediction, cost sums, sign hiding: tests/test_ctu_cu8_transform.py holds that against the oracle on pictures.  A unit is an 8x8 luma and two 4x4 chroma
residual blocks with a QP.  Inputs: all +255 and all -255, +-255 in the sign pattern of every matrix row and column, single impulses at every position, 256 random
units -- each at QP 0, 22 and 51 -- and, fed to the inverse passes directly, coefficient blocks that drive the first inverse pass into its int16 clip."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flatapi
from flatapi import A, ptr

QPS = [0, 22, 51]
DCT = {2: (0, 5), 3: (1, 6)}  # log2 -> (kvz_hip_transform_kind forward, inverse)


@pytest.fixture(scope="module")
def sim():
    """tests/hostsim/libkvz_hostsim_cu8.so, built with the recipe of the other host simulations when it is missing or older than a source"""
    d, csrc = os.path.join(flatapi.ROOT, "tests", "hostsim"), os.path.join(flatapi.ROOT, "kvazaar_amd", "csrc")
    so = os.path.join(d, "libkvz_hostsim_cu8.so")
    srcs = [os.path.join(d, "hostsim_cu8.cpp"), os.path.join(flatapi.ROOT, "include", "kvz_hip_types.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = os.path.join(d, f".libkvz_hostsim_cu8.{os.getpid()}.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp, os.path.join(d, "hostsim_cu8.cpp")])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.kvz_hostsim_cu8_units.restype = C.c_int
    lib.kvz_hostsim_cu8_units.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 5
    return lib


def _matrix(l2):
    """the 8- and 4-point matrices of the standard (dct-generic.c:46-120), for the sign patterns of the inputs"""
    m8 = np.array([[64, 64, 64, 64, 64, 64, 64, 64], [89, 75, 50, 18, -18, -50, -75, -89], [83, 36, -36, -83, -83, -36, 36, 83], [75, -18, -89, -50, 50, 89, 18, -75],
                   [64, -64, -64, 64, 64, -64, -64, 64], [50, -89, 18, 75, -75, -18, 89, -50], [36, -83, 83, -36, -36, 83, -83, 36], [18, -50, 75, -89, 89, -75, 50, -18]])
    m4 = np.array([[64, 64, 64, 64], [83, 36, -36, -83], [64, -64, -64, 64], [36, -83, 83, -36]])
    return m8 if l2 == 3 else m4


def _sign_blocks(l2):
    """+-255 in the sign pattern of each matrix row (along x and along y) and of each column, and their outer products row x row: the inputs that add every product
    of a pass with one sign"""
    n = 1 << l2
    m = _matrix(l2)
    sg = lambda v: np.where(v >= 0, 255, -255)  # noqa: E731
    out = []
    for k in range(n):
        for v in (m[k], m[:, k]):
            out += [np.tile(sg(v), (n, 1)), np.tile(sg(v)[:, None], (1, n))]
        for k2 in range(n):
            out.append(np.outer(sg(m[k]), sg(m[k2])) // 255)
    return [b.astype(np.int16) for b in out]


def _residual_units():
    """(name, [units of 96 int16]) -- luma and chroma blocks of a family paired up index by index (the shorter list repeats)"""
    rng = np.random.default_rng(88)
    fam = {}
    for l2 in (3, 2):
        n = 1 << l2
        imp = []
        for e in range(n * n):
            for v in (255, -255):
                b = np.zeros(n * n, np.int16)
                b[e] = v
                imp.append(b.reshape(n, n))
        fam[l2] = {"flat": [np.full((n, n), 255, np.int16), np.full((n, n), -255, np.int16)], "signs": _sign_blocks(l2), "impulses": imp,
                   "random": [rng.integers(-255, 256, (n, n)).astype(np.int16) for _ in range(256)]}
    out = []
    for name in ("flat", "signs", "impulses", "random"):
        ys, cs = fam[3][name], fam[2][name]
        units = [np.concatenate([ys[i % len(ys)].reshape(-1), cs[(2 * i) % len(cs)].reshape(-1), cs[(2 * i + 1) % len(cs)].reshape(-1)]) for i in range(max(len(ys), (len(cs) + 1) // 2))]
        out.append((name, units))
    return out


def _sim_units(sim, units, qp, from_coeffs=0):
    src = A(np.concatenate(units).astype(np.int16))
    qps = np.full(len(units), qp, np.int32)
    lv, dq, rs = (np.zeros(src.size, np.int16) for _ in range(3))
    assert sim.kvz_hostsim_cu8_units(len(units), from_coeffs, src.ctypes.data, qps.ctypes.data, lv.ctypes.data, dq.ctypes.data, rs.ctypes.data) == 0
    return lv.reshape(-1, 96), dq.reshape(-1, 96), rs.reshape(-1, 96)


def _oracle_plane(oracle, l2, typ, qp, block, from_coeffs=0):
    n = 1 << l2
    p = flatapi.QuantParams(qp=qp, bitdepth=8, slice_is_intra=1, signhide=0, scaling_list=0, cu_is_intra=1, quant_coeff=None, dequant_coeff=None)
    src = A(np.ascontiguousarray(block, np.int16))
    coef, lv, dq, rs = (A(np.zeros(n * n, np.int16)) for _ in range(4))
    if from_coeffs:
        dq[:] = src
    else:
        oracle.transform(DCT[l2][0], 8, ptr(src), ptr(coef))
        oracle.quant(C.byref(p), ptr(coef), ptr(lv), n, n, typ, 0, 1)
        oracle.dequant(C.byref(p), ptr(lv), ptr(dq), n, n, typ, 1)
    oracle.transform(DCT[l2][1], 8, ptr(dq), ptr(rs))
    return lv, dq, rs


def _oracle_units(oracle, units, qp, from_coeffs=0):
    out = [[], [], []]
    for u in units:
        parts = [_oracle_plane(oracle, 3, 0, qp, u[:64], from_coeffs), _oracle_plane(oracle, 2, 2, qp, u[64:80], from_coeffs), _oracle_plane(oracle, 2, 2, qp, u[80:], from_coeffs)]
        for k in range(3):
            out[k].append(np.concatenate([pt[k] for pt in parts]))
    return [np.array(o) for o in out]


@pytest.mark.parametrize("qp", QPS)
@pytest.mark.parametrize("family", _residual_units(), ids=lambda f: f[0])
def test_host_row_passes_equal_the_oracle_on_residual_blocks(oracle, sim, family, qp):
    name, units = family
    got, want = _sim_units(sim, units, qp), _want(oracle, name, units, qp)
    for what, g, w in zip(("levels", "dequantised", "residual"), got, want):
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, (name, qp, what, bad[:8])
    if qp == 0:
        assert all(np.any(w) for w in want), name  # nothing of the comparison is empty: levels, coefficients and residuals are there


def _clip_units():
    """dequantised coefficients that take the first inverse pass to +-32768 and beyond: the int16 ends in the sign pattern of every column of M, alone and mixed"""
    rng = np.random.default_rng(89)
    units = []
    for i in range(64):
        parts = []
        for l2 in (3, 2, 2):
            n = 1 << l2
            m = _matrix(l2)
            col = np.where(m[:, (i + l2) % n] >= 0, 32767, -32768)
            b = np.tile(col[:, None], (1, n)) if i % 2 == 0 else np.outer(col, np.where(m[:, i % n] >= 0, 1, -1))
            if i >= 32:
                b = np.where(rng.random((n, n)) < 0.25, rng.integers(-32768, 32768, (n, n)), b)
            parts.append(np.clip(b, -32768, 32767).astype(np.int16).reshape(-1))
        units.append(np.concatenate(parts))
    units += [rng.integers(-32768, 32768, 96).astype(np.int16) for _ in range(64)]
    return units


def test_host_inverse_passes_equal_the_oracle_into_the_clip(oracle, sim):
    units = _clip_units()
    got, want = _sim_units(sim, units, 22, 1), _want(oracle, "clip", units, 22, 1)
    assert np.array_equal(got[2], want[2]), np.flatnonzero((got[2] != want[2]).any(axis=1))[:8]
    # the inputs do reach the clip of the first pass: a column of int16 ends in the signs of a matrix column sums to 8 * 32767 * 64 >> 7 and more
    m = _matrix(3).astype(np.int64)
    first = (np.einsum("ki,ukj->uji", m, np.array([u[:64].reshape(8, 8) for u in units], np.int64)) + 64) >> 7
    assert (first > 32767).any() and (first < -32768).any()


# ---- the device
_WANT = {}


def _want(oracle, name, units, qp, from_coeffs=0):
    """the oracle's results of a family, computed once and shared by the tests that need them"""
    if (name, qp) not in _WANT:
        _WANT[(name, qp)] = _oracle_units(oracle, units, qp, from_coeffs)
    return _WANT[(name, qp)]


def _dev_units(units, qp, from_coeffs=0):
    """kvz_hip_dev_cu8_units on the units, with a guard unit behind every output: nothing may be written past the last unit"""
    import kvazaar_amd
    from kvazaar_amd import dev as devapi
    dev = devapi.Dev(kvazaar_amd.load_library())
    n = len(units)
    bufs = [dev.put(np.concatenate(units).astype(np.int16)), dev.put(np.full(n, qp, np.int32))] + [dev.put(np.full(96 * (n + 1), -21846, np.int16)) for _ in range(3)]
    try:
        assert dev.lib.kvz_hip_dev_cu8_units(n, from_coeffs, *bufs) == 0
        outs = [dev.get(b, (n + 1, 96), np.int16) for b in bufs[2:]]
        assert all((o[n] == -21846).all() for o in outs)
        assert dev.lib.kvz_hip_dev_cu8_units(n, 2, *bufs) == -1 and dev.lib.kvz_hip_dev_cu8_units(0, 0, *bufs) == 0
        return [o[:n] for o in outs]
    finally:
        dev.free(*bufs)


@pytest.mark.gpu
@pytest.mark.parametrize("qp", QPS)
@pytest.mark.parametrize("family", _residual_units(), ids=lambda f: f[0])
def test_device_stages_equal_the_oracle_on_residual_blocks(oracle, family, qp):
    """a workgroup takes two units: the random family runs without its last unit, 255 units, so that a half-filled last workgroup occurs"""
    name, units = family
    n = len(units) - (name == "random")
    assert n % 2 == (name == "random")
    got, want = _dev_units(units[:n], qp), _want(oracle, name, units, qp)
    for what, g, w in zip(("levels", "dequantised", "residual"), got, want):
        bad = np.flatnonzero((g != w[:n]).any(axis=1))
        assert bad.size == 0, (name, qp, what, bad[:8])


@pytest.mark.gpu
def test_device_inverse_passes_equal_the_oracle_into_the_clip(oracle):
    units = _clip_units()
    got, want = _dev_units(units, 22, 1), _want(oracle, "clip", units, 22, 1)
    assert np.array_equal(got[2], want[2]), np.flatnonzero((got[2] != want[2]).any(axis=1))[:8]
    assert np.array_equal(got[1], np.array(units)) and not got[0].any()
