"""The mode selection of search_intra_rough (search_intra.c:433-530) on tables of SATDs, without a picture around it.  The expected winner comes from a
restatement of the reference's order in Python (the list modes[] / costs[] kept as a list, its first minimum taken at the end); the serial host form of the
CTU pass (CtuProgramT::replay_selection through tests/hostsim/hostsim_select.cpp) must return it on the CPU, and the device form (kvz_select.hpp select_on_wave,
wavefront reductions, through kvz_hip_dev_intra_select) under -m gpu.  The tables are made so that the corners are certain to occur -- ties everywhere, the
min == max exit, minima at both ends of the mode range, every shape of most probable modes, equal mode-bit prices -- and the test counts from the restatement
that they do."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import flatapi
from test_ctu_recon_wide import _oracle_model

SHAPES = [(3, 1), (4, 4)]  # (log2w, nblk): an 8x8 CU, a 16x16 CU
N_BASE = 4096


def mpm(l, a):
    """intra.c:84-126 on the two neighbours' modes"""
    if l == a:
        return (l, 2 + (l + 29) % 32, 2 + (l - 1) % 32) if l > 1 else (0, 1, 26)
    return (l, a, 0 if l and a else (26 if l + a < 2 else 1))


def reference_select(satd, preds, bits, log2w):
    """search_intra.c:433-530 on the 35 SATDs of one block -> (winner, visited modes at the minimum cost, whether min_cost == max_cost ended the search)"""
    offset = 4 if log2w == 3 else 8
    modes = list(range(2, 35, offset))
    min_cost, max_cost = min(satd[m] for m in modes), max(satd[m] for m in modes)
    best_mode = next(m for m in modes if satd[m] == min_cost)  # the first one: costs[] is only replaced by a smaller cost
    best_cost = min_cost
    if min_cost != max_cost:
        while offset > 1:
            offset >>= 1
            centre = best_mode
            for m in (centre - offset, centre + offset):
                if 2 <= m <= 34:
                    modes.append(m)
                    if satd[m] < best_cost:
                        best_cost, best_mode = satd[m], m
    for m in tuple(preds) + (0, 1):
        if m not in modes:
            modes.append(m)
    costs = [float(satd[m]) + bits[1 if m == preds[0] else (2 if m in preds[1:] else 0)] for m in modes]
    low = min(costs)
    return modes[costs.index(low)], costs.count(low), min_cost == max_cost


def _prices(oracle):
    """lambda_sqrt * kvz_luma_mode_bits of the three outcomes at the slice-start state of the intra-mode context (kvz_ctu.hpp price_modes), QP 22 and 37"""
    out = []
    for qp in (22, 37):
        m = _oracle_model(oracle, qp)
        f0, f1 = float(m.intra_mode[0]), float(m.intra_mode[1])
        out.append((m.lambda_sqrt * (f0 + 5), m.lambda_sqrt * (f1 + 1), m.lambda_sqrt * (f1 + 2)))
    return out


def _blocks(rng, kind, log2w, nblk):
    """35 x nblk block SATDs of one table"""
    cand = list(range(2, 35, 4 if log2w == 3 else 8))
    if kind == "uniform":
        return rng.integers(0, 1 << 20, (35, nblk))
    four = rng.integers(0, 1 << 20, 4)
    raw = np.repeat(rng.choice(four, 35)[:, None], nblk, axis=1)  # a mode's blocks alike: equal sums are as frequent as equal draws
    if kind == "four":
        return raw
    raw[cand] = four[0]  # "flat": every mode of the initial pass costs the same
    if kind == "flat-all":
        raw[:] = four[0]
    return raw


@functools.lru_cache(maxsize=None)
def _tables_cached(log2w, nblk, prices):
    rng = np.random.default_rng(1000 * log2w + nblk)
    raws, preds, bits = [], [], []

    def add(kind, force=None):
        i = len(raws)
        raw = _blocks(rng, kind, log2w, nblk)
        if force is not None:  # the minimum of the whole table on this mode
            raw = raw + 8
            raw[force] = 0
        shape = i % 3  # l == a > 1, l == a <= 1, l != a
        l = int(rng.integers(2, 35)) if shape == 0 else int(rng.integers(0, 2)) if shape == 1 else int(rng.integers(0, 35))
        a = l if shape < 2 else int(rng.choice([m for m in range(35) if m != l]))
        p = prices[(i >> 1) & 1]
        raws.append(raw.astype(np.uint32)); preds.append(mpm(l, a)); bits.append((p[0],) * 3 if (i >> 2) % 4 == 0 else p)

    third = N_BASE // 3
    for kind, n in (("uniform", third), ("four", third), ("flat", (N_BASE - 2 * third + 1) // 2), ("flat-all", (N_BASE - 2 * third) // 2)):
        for _ in range(n):
            add(kind)
    for force in (2, 34):
        for k in range(64):
            add("uniform" if k & 1 else "four", force)
    want = stats = None
    for _ in range(8):  # generate until the corners are frequent enough (they are at once; the assertion is test_tables_hold_the_corners')
        satd = [((r.astype(np.int64) + 2) >> 2).sum(axis=1) for r in raws]
        res = [reference_select([int(v) for v in satd[i]], preds[i], bits[i], log2w) for i in range(len(raws))]
        want = np.array([r[0] for r in res], np.int32)
        stats = dict(ties=sum(r[1] >= 2 for r in res), exits=sum(r[2] for r in res), winners={r[0] for r in res},
                     ends={m: sum(int(np.argmin(v)) == m and int(np.sum(v == v.min())) == 1 for v in satd[N_BASE:N_BASE + 128]) for m in (2, 34)}, shapes={(p[0] == 0 and p[1] == 1, p[2]) for p in preds})
        if stats["ties"] >= 1000 and stats["exits"] >= 1000:
            break
        for _ in range(256):
            add("four"); add("flat")
    return dict(raw=np.ascontiguousarray(np.stack(raws)), preds=np.array(preds, np.int8), bits=np.array(bits, np.float64), want=want, stats=stats)


@pytest.fixture(scope="module")
def tables(oracle):
    prices = tuple(_prices(oracle))
    return {shape: _tables_cached(shape[0], shape[1], prices) for shape in SHAPES}


@pytest.fixture(scope="module")
def sim():
    """tests/hostsim/libkvz_hostsim_select.so, built with the recipe of the other host simulations when it is missing or older than a source"""
    d, csrc = os.path.join(flatapi.ROOT, "tests", "hostsim"), os.path.join(flatapi.ROOT, "kvazaar_amd", "csrc")
    so = os.path.join(d, "libkvz_hostsim_select.so")
    srcs = [os.path.join(d, f) for f in ("hostsim_select.cpp", "hostsim.cpp")] + [os.path.join(flatapi.ROOT, "include", "kvz_hip_types.h")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = os.path.join(d, f".libkvz_hostsim_select.{os.getpid()}.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp, os.path.join(d, "hostsim_select.cpp")])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.kvz_hostsim_intra_select.restype = C.c_int
    lib.kvz_hostsim_intra_select.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
    return lib


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{1 << s[0]}x{1 << s[0]}")
def test_tables_hold_the_corners(tables, shape):
    t = tables[shape]
    st = t["stats"]
    assert len(t["want"]) >= N_BASE + 128
    assert st["ties"] >= 1000, st  # two or more visited modes at the minimum cost: append order decides
    assert st["exits"] >= 1000, st  # min_cost == max_cost: no refinement
    assert st["ends"] == {2: 64, 34: 64}, st  # the smallest SATD on mode 2 / 34: the refinement at the ends of the range, where one of its two modes does not exist
    assert {0, 1, 2, 34} <= st["winners"] and len(st["winners"]) >= 30, st
    assert {(True, 26), (False, 0), (False, 1), (False, 26)} <= st["shapes"], st  # (0, 1, 26); a third candidate of planar, DC, 26
    same = np.all(t["bits"] == t["bits"][:, :1], axis=1)
    assert 0.2 < same.mean() < 0.3  # a quarter of the tables price every outcome alike
    assert len({tuple(b) for b in t["bits"][~same]}) == 2  # QP 22 and 37


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{1 << s[0]}x{1 << s[0]}")
def test_host_form_returns_the_reference_order_winner(tables, sim, shape):
    t = tables[shape]
    got = np.full(len(t["want"]), -2, np.int32)
    assert sim.kvz_hostsim_intra_select(shape[0], shape[1], t["raw"].ctypes.data, t["preds"].ctypes.data, t["bits"].ctypes.data, len(got), got.ctypes.data) == 0
    bad = np.flatnonzero(got != t["want"])
    assert bad.size == 0, (bad[:8], got[bad[:8]], t["want"][bad[:8]])


def test_host_form_refuses_other_shapes(sim):
    assert sim.kvz_hostsim_intra_select(3, 4, None, None, None, 0, None) == -1


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{1 << s[0]}x{1 << s[0]}")
def test_device_form_returns_the_reference_order_winner(tables, shape):
    """one launch per shape, a wavefront per table; the count is no multiple of the four tables of a workgroup only by what the generator added, so the last
    table's index is also run alone"""
    import kvazaar_amd
    from kvazaar_amd import dev as devapi
    dev = devapi.Dev(kvazaar_amd.load_library())
    t = tables[shape]
    n = len(t["want"])
    draw, dpreds, dbits, dout = dev.put(t["raw"]), dev.put(t["preds"]), dev.put(t["bits"]), dev.put(np.full(n + 1, -2, np.int32))
    try:
        assert dev.lib.kvz_hip_dev_intra_select(shape[0], shape[1], draw, dpreds, dbits, n, dout) == 0
        got = dev.get(dout, (n + 1,), np.int32)
        assert got[n] == -2  # nothing written past the last table
        bad = np.flatnonzero(got[:n] != t["want"])
        assert bad.size == 0, (bad[:8], got[bad[:8]], t["want"][bad[:8]])
        assert dev.lib.kvz_hip_dev_intra_select(shape[0], shape[1], draw, dpreds, dbits, 1, dout) == 0  # a workgroup with one wavefront at work
        assert dev.get(dout, (2,), np.int32).tolist() == [int(t["want"][0]), int(t["want"][1])]
        assert dev.lib.kvz_hip_dev_intra_select(3, 4, draw, dpreds, dbits, n, dout) == -1
    finally:
        dev.free(draw, dpreds, dbits, dout)
