"""The rough search's row table (Tables::satd_rows, kvz_tables.hpp): what a lane of a group of 32 (angular mode, block) pairs reads for each of its four rows --
reference array and window start, fraction, source row, edge byte -- as constants of (CU size, group, lane, row).  Through the host twin
(tests/hostsim/hostsim_satd_rows.cpp):
 - every entry, both CU sizes, all groups, lanes and rows, against a restatement of the index arithmetic the generator did per search before the table
   (intra-generic.c:59-148 on the group's lane decomposition), and the wide window read against the end of the array's row;
 - the eight predicted bytes of every row, by the scalar walk of the table on the pass's own filtered / extended references and edge bytes, against the oracle's
   intra prediction on the reference sets of rough_rows_common.py (tests/test_rough_rows.py runs the device's packed generator on the same sets)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flatapi
import rough_rows_common as rr

DISP = [0, 0, 32, 26, 21, 17, 13, 9, 5, 2, 0, -2, -5, -9, -13, -17, -21, -26, -32, -26, -21, -17, -13, -9, -5, -2, 0, 2, 5, 9, 13, 17, 21, 26, 32]  # intra-generic.c:59-60


@pytest.fixture(scope="module")
def sim():
    """tests/hostsim/libkvz_hostsim_satd_rows.so, built with the recipe of the other host simulations when it is missing or older than a source"""
    d, csrc = os.path.join(flatapi.ROOT, "tests", "hostsim"), os.path.join(flatapi.ROOT, "kvazaar_amd", "csrc")
    so = os.path.join(d, "libkvz_hostsim_satd_rows.so")
    srcs = [os.path.join(d, "hostsim_satd_rows.cpp"), os.path.join(flatapi.ROOT, "include", "kvz_hip_types.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = os.path.join(d, f".libkvz_hostsim_satd_rows.{os.getpid()}.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp, os.path.join(d, "hostsim_satd_rows.cpp")])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.kvz_hostsim_satd_rows_table.restype = None
    lib.kvz_hostsim_satd_rows_table.argtypes = [C.c_void_p, C.c_void_p]
    lib.kvz_hostsim_rough_rows.restype = C.c_int
    lib.kvz_hostsim_rough_rows.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return lib


def _table(sim):
    table, layout = np.zeros((5, 64, 8), np.uint32), np.zeros(9, np.uint32)
    sim.kvz_hostsim_satd_rows_table(table.ctypes.data, layout.ctypes.data)
    names = ("ref_row", "filtered", "extended", "mref_stride", "mref_org", "src_t", "edge", "window", "src_vertical")
    return table, dict(zip(names, (int(v) for v in layout)))


@pytest.mark.parametrize("log2w", [3, 4])
def test_every_entry_names_what_the_generator_worked_out_per_search(sim, log2w):
    table, L = _table(sim)
    w, lb = 1 << log2w, 2 * (log2w - 3)
    nblk, seen = 1 << lb, set()
    for g in range(1 if log2w == 3 else 4):
        for lane in range(64):
            # the pair of the lane and the generator's parameters: the statement of angular_block_satd, on the lane's half of the block
            p = 32 * g + (lane & 31)
            mode, b, half = 2 + (p >> lb), p & (nblk - 1), lane >> 5
            bx, by = (b & ((w >> 3) - 1)) * 8, (b >> (log2w - 3)) * 8
            vertical, disp = mode >= 18, DISP[mode]
            p0, q0 = (bx, by) if vertical else (by, bx)
            if disp < 0:
                row, row_len, at0 = L["extended"] + L["mref_stride"] * (mode - 11), L["mref_stride"], L["mref_org"]
            else:
                row, row_len, at0 = (L["filtered"] if rr.reads_filtered(log2w, mode) else 0) + L["ref_row"] * (0 if vertical else 1), L["ref_row"], 0
            for i in range(4):
                r = 4 * half + i
                qa = q0 + r + 1
                delta = qa * disp
                di, df = delta >> 5, delta & 31
                w0, w1 = (int(v) for v in table[0 if log2w == 3 else 1 + g, lane, 2 * i:2 * i + 2])
                where = (log2w, g, lane, i, mode, b)
                assert w0 & 0xffff == row + at0 + p0 + 1 + di, where            # the array and the window's start in it
                assert 0 <= at0 + p0 + 1 + di and at0 + p0 + 1 + di + L["window"] <= row_len, where  # the wide read stays inside the array's row
                assert (w1 & 0xffff) == 8 * df, where                            # the fraction (as the right neighbour's weight, times 8)
                edge = disp == 0 and p0 == 0                                     # intra.c:207-219: first row of mode 26 / first column of mode 10
                assert w0 >> 16 == (L["edge"] + 1 + (0 if vertical else w) + qa - 1 if edge else L["edge"]), where
                src = w1 >> 16
                assert bool(src & L["src_vertical"]) == vertical, where
                want_src = (by + r) * 32 + bx if vertical else L["src_t"] + bx * w + by + r * w  # quadrant-buffer row / row of the transposed block
                assert src & (L["src_vertical"] - 1) == want_src and want_src % 8 == 0, where
                seen.add((mode, b, r))
    assert len(seen) == 32 * nblk * 8  # every row of every (mode, block) pair, once
    assert sum(1 for g in range(1 if log2w == 3 else 4) for lane in range(64) for i in range(4) if int(table[0 if log2w == 3 else 1 + g, lane, 2 * i]) >> 16 != L["edge"]) == 2 * w


@pytest.mark.parametrize("log2w", [3, 4])
def test_scalar_walk_of_the_table_equals_the_oracle_prediction(oracle, sim, log2w):
    tops, lefts = rr.ref_sets(log2w)
    n = 2 * (1 << log2w) + 1
    want = rr.oracle_blocks(oracle, log2w)
    t, l = np.ascontiguousarray(tops[:, :n]), np.ascontiguousarray(lefts[:, :n])
    got = np.full(want.size + 64, 0xA5, np.uint8)
    assert sim.kvz_hostsim_rough_rows(log2w, t.ctypes.data, l.ctypes.data, len(t), got.ctypes.data) == 0
    assert (got[want.size:] == 0xA5).all()
    bad = np.argwhere((got[:want.size].reshape(want.shape) != want).any(axis=3))
    assert bad.size == 0, bad[:8]  # (set, mode - 2, block)
    # the sets do drive the edge samples into both ends of their clip, and leave most of them inside it
    for mode, side, main in ((26, lefts, tops), (10, tops, lefts)):
        raw = main[:, 1:2].astype(np.int32) + ((side[:, 1:(1 << log2w) + 1].astype(np.int32) - side[:, :1].astype(np.int32)) >> 1)
        assert (raw < 0).any() and (raw > 255).any() and ((raw >= 0) & (raw <= 255)).any(), mode
    assert sim.kvz_hostsim_rough_rows(5, t.ctypes.data, l.ctypes.data, 1, got.ctypes.data) == -1
