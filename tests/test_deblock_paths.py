"""Deblocking, every decision and threshold, without a GPU: the Python reference (tests/deblock_reference.py, written from H.265 8.7.2 and filter.c) against
the standard's tables, the C oracle against the Python reference over every QP, the oracle against the compiled reference over the whole (QP, beta, tc) grid, and
two conditions on the inputs that tests/test_gpu_deblock_paths.py runs on the device (tests/deblock_atlas.py): they reach every path of the filter and every exit
of the boundary-strength rule at least MIN_COUNT times per direction, and a one-token error in any of the listed places changes the result on them."""
import os
from collections import Counter

import numpy as np
import pytest

import deblock_atlas as atlas
import deblock_common as dc
import deblock_reference as dr
import flatapi
import test_deblock_inter as tdi

MIN_COUNT = 16
OFFSETS = [(0, 0)] + atlas.CORNERS
W, H = 72, 72  # the picture size of everything that runs the Python reference per QP and offset


def oracle_intra(oracle, w, h, qp, b_off, t_off, frame, depth):
    return dc.run_cpu(oracle.lib.kvz_oracle_deblock_frame, w, h, qp, b_off, t_off, frame, depth)


def oracle_inter(oracle, w, h, qp, b_off, t_off, frame, info, slice_b):
    return tdi.run(oracle.lib.kvz_oracle_deblock_frame_inter, w, h, qp, b_off, t_off, frame, info, slice_b)


# ---- tables and thresholds ------------------------------------------------------------------------------------------------------------------------------------
def test_tables_have_the_shape_of_the_standard():
    """Table 8-12 / 8-10 as typed out: the entries the text of the standard singles out, and what holds for every entry"""
    assert dr.BETA_TABLE[15] == 0 and dr.BETA_TABLE[16] == 6 and dr.BETA_TABLE[28] == 18 and dr.BETA_TABLE[29] == 20 and dr.BETA_TABLE[51] == 64
    assert dr.TC_TABLE[17] == 0 and dr.TC_TABLE[18] == 1 and dr.TC_TABLE[26] == 1 and dr.TC_TABLE[27] == 2 and dr.TC_TABLE[46] == 11 and dr.TC_TABLE[47] == 13
    assert dr.TC_TABLE[51] == 20 and dr.TC_TABLE[53] == 24
    assert all(a <= b for a, b in zip(dr.BETA_TABLE, dr.BETA_TABLE[1:])) and all(a <= b for a, b in zip(dr.TC_TABLE, dr.TC_TABLE[1:]))
    # beta' = Q - 10 on 16 .. 28 and 2 Q - 38 from 29 on; tc' in runs of 9, 4, 4, 3, 2, 2 from Q = 18, then 7 .. 11 and 13, 14, 16 .. 24
    assert sum(dr.BETA_TABLE) == sum(range(6, 19)) + sum(range(20, 65, 2)) == 1122
    assert sum(dr.TC_TABLE) == 9 * 1 + 4 * 2 + 4 * 3 + 3 * 4 + 2 * 5 + 2 * 6 + sum(range(7, 12)) + 13 + 14 + sum(range(16, 25, 2)) == 235
    assert dr.CHROMA_QP_TABLE[:30] == list(range(30)) and dr.CHROMA_QP_TABLE[30:44] == [29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37]
    assert dr.CHROMA_QP_TABLE[44:] == [q - 6 for q in range(44, 58)]


def test_thresholds_against_the_literal_tables():
    seen_beta, seen_tc = set(), set()
    for qp in range(52):
        for b_off in range(-6, 7):
            for t_off in range(-6, 7):
                beta, tc, tc1, tc_c = dr.thresholds(qp, b_off, t_off)
                ib, i2, i1, ic = (min(max(qp + 2 * b_off, 0), 51), min(max(qp + 2 + 2 * t_off, 0), 53), min(max(qp + 2 * t_off, 0), 53),
                                  min(max(dr.CHROMA_QP_TABLE[qp] + 2 + 2 * t_off, 0), 53))
                assert (beta, tc, tc1, tc_c) == (dr.BETA_TABLE[ib], dr.TC_TABLE[i2], dr.TC_TABLE[i1], dr.TC_TABLE[ic]), (qp, b_off, t_off)
                seen_beta.add(ib)
                seen_tc.update((i2, i1, ic))
    assert seen_beta == set(range(52)) and seen_tc == set(range(54))  # every table entry is reached, both clips of either index included


# ---- the oracle against the Python reference --------------------------------------------------------------------------------------------------------------------
def test_oracle_equals_python_reference_intra(oracle):
    for qp in range(52):
        for b_off, t_off in OFFSETS:
            for frame, depth in atlas.pictures(W, H):
                want, _ = dr.deblock_intra(W, H, qp, b_off, t_off, frame, depth)
                got = oracle_intra(oracle, W, H, qp, b_off, t_off, frame, depth)
                assert np.array_equal(got, want), (qp, b_off, t_off, np.flatnonzero(got != want)[:8])


@pytest.mark.parametrize("slice_b", [0, 1], ids=["P", "B"])
def test_oracle_equals_python_reference_inter(oracle, slice_b):
    """every record set meets every picture and both parities of the QP within the sweep"""
    pics, sets = atlas.pictures(W, H), atlas.inter_records(W, H, slice_b)
    for qp in range(52):
        for b_off, t_off in OFFSETS:
            for j, (frame, _) in enumerate(pics):
                info = sets[(j + qp // 2 + len(pics) * (qp & 1)) % len(sets)]
                want, _ = dr.deblock_inter(W, H, qp, b_off, t_off, frame, info, slice_b)
                got = oracle_inter(oracle, W, H, qp, b_off, t_off, frame, info, slice_b)
                assert np.array_equal(got, want), (qp, b_off, t_off, j, np.flatnonzero(got != want)[:8])


# ---- the oracle against the compiled reference: the whole grid, both sides C -----------------------------------------------------------------------------------
def test_oracle_equals_compiled_reference_on_the_whole_grid(oracle):
    if not os.path.exists(flatapi.refshim_path()):
        pytest.skip("oracle/_ref not built")
    ref = flatapi.load_ref(0)
    frame, depth = atlas.pictures(W, H)[0]
    sets = {slice_b: atlas.inter_records(W, H, slice_b) for slice_b in (0, 1)}
    for qp in range(52):
        for b_off in range(-6, 7):
            for t_off in range(-6, 7):
                a = oracle_intra(oracle, W, H, qp, b_off, t_off, frame, depth)
                b = dc.run_cpu(ref.lib.kvz_ref_deblock_frame, W, H, qp, b_off, t_off, frame, depth)
                assert np.array_equal(a, b), ("intra", qp, b_off, t_off, np.flatnonzero(a != b)[:8])
                for slice_b in (0, 1):
                    info = sets[slice_b][(qp + b_off + t_off) % len(sets[slice_b])]
                    a = oracle_inter(oracle, W, H, qp, b_off, t_off, frame, info, slice_b)
                    b = tdi.run(ref.lib.kvz_ref_deblock_frame_inter, W, H, qp, b_off, t_off, frame, info, slice_b)
                    assert np.array_equal(a, b), ("inter", slice_b, qp, b_off, t_off, np.flatnonzero(a != b)[:8])


# ---- the census of what the GPU tests run -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def intra_census():
    """GPU test (a) at offsets (0, 0): every geometry's batch at every QP"""
    total = Counter()
    for w, h in atlas.GEOMETRIES:
        for frame, depth in atlas.pictures(w, h):
            for qp in range(52):
                total.update(dr.deblock_intra(w, h, qp, 0, 0, frame, depth)[1])
    return total


@pytest.mark.parametrize("direction", ["ver", "hor"])
def test_census_luma(intra_census, direction):
    counts = {k: intra_census["luma", direction, k] for k in dr.LUMA_PATHS + dr.LUMA_EVENTS}
    print(direction, counts)
    assert all(v >= MIN_COUNT for v in counts.values()), counts


@pytest.mark.parametrize("direction", ["ver", "hor"])
def test_census_chroma(intra_census, direction):
    counts = {k: intra_census["chroma", direction, k] for k in dr.CHROMA_EVENTS}
    print(direction, counts)
    assert all(v >= MIN_COUNT for v in counts.values()), counts


@pytest.mark.parametrize("kind", ["P", "B"])
def test_census_strength_exits(kind):
    """GPU test (b): the 52 pictures of a launch; the exits do not depend on the offsets"""
    frames, records, _ = atlas.launch_of_52(W, H, kind)
    total = Counter()
    for i in range(52):
        total.update(dr.deblock_inter(W, H, i, 0, 0, frames[i], records[i], kind == "B")[1])
    for direction in ("ver", "hor"):
        counts = {e: total["bs", direction, e[0], e[1]] for e in (dr.STRENGTH_EXITS_B if kind == "B" else dr.STRENGTH_EXITS_P)}
        print(kind, direction, counts)
        assert all(v >= MIN_COUNT for v in counts.values()), (direction, counts)
        # strength 1 and 2 parts are filtered, not only classified: tc1 and tc both meet the weak and the strong filter
        assert all(total["luma", direction, k] >= MIN_COUNT for k in ("strong", "weak_pq", "bs0")), direction


def test_partitioned_records_have_prediction_edges_off_the_transform_grid():
    """every part_size appears, and coded coefficients on a prediction edge that is no transform edge leave equal motion at strength 0"""
    seen = set()
    for slice_b in (0, 1):
        for info in atlas.inter_records(W, H, slice_b) + atlas.inter_records(136, 72, slice_b):
            seen.update(r.part_size for r in info if r.type == 2)
    assert seen == set(range(8))
    info = atlas.partitioned_records(W, H, 0, 1)
    _, census = dr.deblock_inter(W, H, 40, 0, 0, atlas.pictures(W, H)[0][0], info, 0)
    assert census["bs", "ver", "p_slice", 0] and census["bs", "hor", "p_slice", 0]
    assert all(r.cbf_y for r in info if r.type == 2)


# ---- the inputs discriminate ------------------------------------------------------------------------------------------------------------------------------------
def sweep():
    """(qp, beta_off, tc_off) as the GPU tests (a) and (b) run them, high QPs first: that is where most mutations show"""
    return [(qp, b, t) for qp in range(51, -1, -1) for b, t in OFFSETS]


@pytest.mark.parametrize("mut", dr.LUMA_MUTATIONS + dr.CHROMA_MUTATIONS)
def test_mutation_is_seen_intra(oracle, mut):
    for w, h in atlas.GEOMETRIES:
        for frame, depth in atlas.pictures(w, h):
            for qp, b_off, t_off in sweep():
                if not np.array_equal(dr.deblock_intra(w, h, qp, b_off, t_off, frame, depth, mut)[0], oracle_intra(oracle, w, h, qp, b_off, t_off, frame, depth)):
                    return
    pytest.fail(f"the atlas cannot see: {dr.MUTATIONS[mut]}")


@pytest.mark.parametrize("mut", dr.INTER_MUTATIONS)
def test_mutation_is_seen_inter(oracle, mut):
    kind = "B" if mut == "b_same_or" else "P"
    frames, records, _ = atlas.launch_of_52(W, H, kind)
    for b_off, t_off in OFFSETS:
        for qp in range(51, -1, -1):
            want = oracle_inter(oracle, W, H, qp, b_off, t_off, frames[qp], records[qp], kind == "B")
            if not np.array_equal(dr.deblock_inter(W, H, qp, b_off, t_off, frames[qp], records[qp], kind == "B", mut)[0], want):
                return
    pytest.fail(f"the atlas cannot see: {dr.MUTATIONS[mut]}")


def test_every_listed_mutation_is_tested():
    assert sorted(dr.LUMA_MUTATIONS + dr.CHROMA_MUTATIONS + dr.INTER_MUTATIONS) == sorted(dr.MUTATIONS)
