"""The SAO decision and filter, every branch, without a GPU: the Python statement (tests/sao_reference.py, written from H.265 8.7.3 / 9.3 and the repository's own
description of the encoder's search) against the C oracle and against the device sources compiled for the host, on the pictures of tests/sao_atlas.py over every
QP, the B / P / I initial context values, WPP on and off, deblocking off and on -- and three conditions on those pictures, which are what
tests/test_gpu_sao_paths.py runs on the device: they reach every event of sao_reference.EVENTS at least MIN_COUNT times, with deblocking the R / V / D view changes
at least MIN_COUNT decisions, and a one-token error in any of the places of sao_reference.MUTATIONS changes a parameter, a merge flag or a sample."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import ctu_common as cc
import sao_atlas as atlas
import sao_reference as sr
from flatapi import SaoParams, ptr
from test_encoder_parity import oracle_model
from test_hostsim import hostsim  # noqa: F401  (fixture)

MIN_COUNT = 16
CX_SAO_MERGE, CX_SAO_TYPE = 148, 149  # KVZ_HIP_CX_SAO_MERGE / _TYPE (include/kvz_hip_types.h)
SLICES = [("B", sr.B), ("P", sr.P), ("I", sr.I)]
IDS = [f"{w}x{h}" for w, h in atlas.GEOMETRIES]


@pytest.fixture(scope="module")
def fbits():
    return np.array(cc.model_constants()["entropy_fbits"], np.float32)


def model_of(oracle, qp, slice_type, no_wpp):
    """the cost model both C sides read: lambda of the QP, the two SAO contexts at the slice type's initial values"""
    m = oracle_model(oracle, qp)
    assert m.lambda_ == sr.lambda_of(qp)
    m.ctx_init[CX_SAO_MERGE], m.ctx_init[CX_SAO_TYPE] = sr.ctx_state(sr.INIT_MERGE, qp), sr.ctx_state(sr.INIT_TYPE[slice_type], qp)
    m.no_wpp = no_wpp
    return m


def records_of(luma, chroma):
    """kvz_hip_sao_params arrays -> [lcu][3] records of sao_reference"""
    out = []
    for l, c in zip(luma, chroma):
        out.append([(l.type, l.eo_class, l.band_position[0], tuple(l.offsets[1:5])), (c.type, c.eo_class, c.band_position[0], tuple(c.offsets[1:5])),
                    (c.type, c.eo_class, c.band_position[1], tuple(c.offsets[6:10]))])
    return out


def lcus_of(w, h):
    return ((w + 63) // 64) * ((h + 63) // 64)


def oracle_decide(oracle, model, w, h, src, rec, depth, deblock):
    """the oracle's search LCU by LCU (literally deblocking one LCU at a time) and its filter -> (records, merge flags, final picture)"""
    n = lcus_of(w, h)
    luma, chroma, merge = (SaoParams * n)(), (SaoParams * n)(), np.zeros(n, np.uint8)
    work, info = rec.copy(), atlas.records_from_depth(w, h, depth)
    f = oracle.lib.kvz_oracle_sao_search_frame_inter
    f.restype = None
    f(C.byref(model), w, h, ptr(src), ptr(work), info, 0, int(deblock), 0, 0, luma, chroma, ptr(merge))
    out = work.copy()
    g = oracle.lib.kvz_oracle_sao_frame
    g.restype = None
    g(w, h, ptr(work), ptr(out), luma, chroma)
    return records_of(luma, chroma), [int(v) for v in merge], out


def deblock_passes(oracle, w, h, qp, frame, depth, passes):
    out = frame.copy()
    ys, cs = w * h, w * h // 4
    f = oracle.lib.kvz_oracle_deblock_frame_passes
    f.restype = None
    f(w, h, qp, 0, 0, ptr(out), ptr(out, offset=ys), ptr(out, offset=ys + cs), ptr(np.ascontiguousarray(depth)), passes)
    return out


def views(oracle, w, h, qp, rec, depth, deblock):
    """(R, V, D): before deblocking, after the vertical edges, after the horizontal edges too"""
    if not deblock:
        return rec, rec, rec
    V = deblock_passes(oracle, w, h, qp, rec, depth, 1)
    return rec, V, deblock_passes(oracle, w, h, qp, V, depth, 2)


def hostsim_decide(hostsim, model, w, h, src, R, V, D):
    n = lcus_of(w, h)
    luma, chroma, merge = (SaoParams * n)(), (SaoParams * n)(), np.zeros(n, np.uint8)
    f = hostsim.lib.kvz_hostsim_sao_decide
    f.restype = None
    f(C.byref(model), w, h, ptr(src), ptr(R), ptr(V), ptr(D), luma, chroma, ptr(merge))
    return records_of(luma, chroma), [int(v) for v in merge]


def test_transition_tables_are_the_oracles(oracle):
    """Table 9-45 as typed out in sao_reference against cabac.c's tables as the oracle regenerates them, over pStateIdx 0 .. 62 (63 belongs to the terminating bin
    alone: no context reaches it, and what an LPS does there is the encoder's choice)"""
    oracle.lib.kvz_oracle_next_state_table.restype = C.POINTER(C.c_uint8)
    for lps, mine in ((0, sr.NEXT_MPS), (1, sr.NEXT_LPS)):
        assert [oracle.lib.kvz_oracle_next_state_table(lps)[i] for i in range(126)] == mine[:126]


def test_initial_states_are_the_models(oracle):
    """H.265 9.3.2.2 in sao_reference against the oracle's I-slice model: sao_merge_flag 153, sao_type_idx 200"""
    for qp in range(52):
        m = oracle_model(oracle, qp)
        assert (m.ctx_init[CX_SAO_MERGE], m.ctx_init[CX_SAO_TYPE]) == (sr.ctx_state(153, qp), sr.ctx_state(200, qp)), qp


@pytest.mark.parametrize("deblock", [0, 1], ids=["plain", "deblocked"])
@pytest.mark.parametrize("size", atlas.GEOMETRIES, ids=IDS)
def test_oracle_and_hostsim_equal_python_statement(oracle, hostsim, fbits, size, deblock):
    """parameters, merge flags and the final picture, per picture at every QP, slice type and WPP setting; the statistics of a picture (and QP, with deblocking) are
    taken once"""
    w, h = size
    for j, (src, rec, depth) in enumerate(atlas.pictures(w, h)):
        blocks = None
        for qp in range(52):
            R, V, D = views(oracle, w, h, qp, rec, depth, deblock)
            if deblock or blocks is None:
                blocks = sr.prepare(w, h, src, R, V, D)
            for name, slice_type in SLICES:
                for no_wpp in (0, 1):
                    model = model_of(oracle, qp, slice_type, no_wpp)
                    want = sr.decide(w, h, blocks, qp, slice_type, no_wpp, fbits)
                    final = sr.apply(w, h, D, want[0])
                    o_recs, o_merge, o_final = oracle_decide(oracle, model, w, h, src, rec, depth, deblock)
                    where = (j, qp, name, no_wpp)
                    assert o_merge == want[1], where
                    assert o_recs == want[0], (where, [i for i in range(len(o_recs)) if o_recs[i] != want[0][i]][:4])
                    assert np.array_equal(o_final, final), (where, np.flatnonzero(o_final != final)[:8])
                    assert hostsim_decide(hostsim, model, w, h, src, R, V, D) == (o_recs, o_merge), ("hostsim", where)


@pytest.fixture(scope="module")
def census(oracle, fbits):
    """exactly what test_gpu_sao_paths.py::test_every_qp_in_one_launch runs on the device (sao_atlas.launch_cases): per geometry eight launches of 104 pictures --
    I and B, deblocking off and on, WPP on and off --, each (picture, QP) pair in the (slice type, WPP) launches that hold it.  The context-free candidates of a
    picture are counted once per view: once without deblocking, once per QP with it."""
    total = Counter()
    for w, h in atlas.GEOMETRIES:
        pics, blocks = atlas.pictures(w, h), {}
        for slice_b, deblock, no_wpp, cases in atlas.launch_cases():
            for j, qp in cases:
                src, rec, depth = pics[j]
                R, V, D = views(oracle, w, h, qp, rec, depth, deblock)
                key = (j, qp if deblock else None)
                if key not in blocks:
                    blocks[key] = sr.prepare(w, h, src, R, V, D, census=total)
                recs, _ = sr.decide(w, h, blocks[key], qp, sr.B if slice_b else sr.I, no_wpp, fbits, census=total)
                sr.apply(w, h, D, recs, census=total)
    return total


def test_census(census):
    """Every event at least MIN_COUNT times.  Lowest counts seen: tie left==up 70, merge from a luma band record 85, tie edge==band 89, tie up==own 92, tie
    left==own 131, merge up 134 (the filter's events count samples).
    edge_dd == band_dd is counted only where the winner of that comparison goes on to beat "nothing" -- elsewhere < and <= end at the same "none" -- and it is
    constructed: the "tie" blocks of the atlas (sao_atlas._block) make class 0 and one band catch the same samples at the same offset and give band a lead of k
    in distortion for its 4 more mode bits, so the costs meet where round(4 lambda) = k.  The band_valid == false branch is not an event: see sao_reference's
    docstring for why the band search total cannot reach INT_MAX."""
    counts = {e: census[e] for e in sr.EVENTS}
    print(sorted(counts.items(), key=lambda kv: kv[1])[:12])
    assert all(v >= MIN_COUNT for v in counts.values()), {e: v for e, v in counts.items() if v < MIN_COUNT}


def test_band_offsets_are_one_step_from_zero(fbits):
    """the quirk of calc_sao_band_offsets as a property of the results: errors of up to 200 levels, and no band record carries more than +-1"""
    seen = 0
    for w, h in atlas.GEOMETRIES:
        for src, rec, _ in atlas.pictures(w, h):
            blocks = sr.prepare(w, h, src, rec)
            for qp in (0, 22, 37, 51):
                for r in (r for lcu in sr.decide(w, h, blocks, qp, sr.B, 0, fbits)[0] for r in lcu if r[0] == 1):
                    assert all(abs(o) <= 1 for o in r[3]), r
                    seen += 1
    assert seen >= MIN_COUNT


def test_view_sensitivity(oracle):
    """with deblocking, the LCU decisions that differ from what the fully deblocked picture alone would give (the oracle without deblocking on the picture
    deblocked beforehand): without them nothing here would notice a wrong R / V / D rule"""
    differing = 0
    for w, h in atlas.GEOMETRIES[1:]:
        for src, rec, depth in atlas.pictures(w, h):
            for qp in range(20, 52, 3):  # (below QP 16 the deblocking thresholds are zero: nothing is filtered)
                model = model_of(oracle, qp, sr.B, 0)
                D = deblock_passes(oracle, w, h, qp, rec, depth, 3)
                a, am, _ = oracle_decide(oracle, model, w, h, src, rec, depth, 1)
                b, bm, _ = oracle_decide(oracle, model, w, h, src, D, depth, 0)
                differing += sum(a[i] != b[i] or am[i] != bm[i] for i in range(len(a)))
    print("decisions the view changes:", differing)
    assert differing >= MIN_COUNT


def test_view_rows_beyond_the_filters_reach_do_not_matter(oracle):
    """sao_reference.EQUIVALENT_VIEW_MUTATIONS: V and D agree on luma row n - 4 and chroma rows n - 3, n - 2 of every LCU row but the last, so reading one more luma
    row or two more chroma rows from V is no error an input could show -- held here on the pictures deblocking changes most, at every QP"""
    changed = 0
    for w, h in atlas.GEOMETRIES[1:]:
        for src, rec, depth in atlas.pictures(w, h):
            for qp in range(52):
                _, V, D = views(oracle, w, h, qp, rec, depth, 1)
                changed += int(np.count_nonzero(V != D))
                for c, (v, d) in enumerate(zip(sr.planes_of(w, h, V), sr.planes_of(w, h, D))):
                    n = 32 if c else 64
                    rows = [y for y in range(v.shape[0]) if y % n in ((n - 3, n - 2) if c else (n - 4,))]
                    assert np.array_equal(v[rows], d[rows]), (w, h, qp, c)
                for mut in sr.EQUIVALENT_VIEW_MUTATIONS if qp % 13 == 12 else ():  # and prepare() under either builds the same views (QP 12, 25, 38, 51)
                    a, b = sr.prepare(w, h, src, rec, V, D, mutation=mut), sr.prepare(w, h, src, rec, V, D)
                    assert all(np.array_equal(x.rec, y.rec) for ra, rb in zip(a, b) for x, y in zip(ra, rb)), (w, h, qp, mut)
    assert changed >= MIN_COUNT  # the horizontal edges did write something


# ---- the inputs discriminate ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mut", sorted(sr.MUTATIONS))
def test_mutation_is_seen(oracle, fbits, mut):
    deblock = int(mut in sr.VIEW_MUTATIONS)
    for w, h in atlas.GEOMETRIES[::-1]:
        for src, rec, depth in atlas.pictures(w, h):
            blocks = None
            for qp in (range(51, 19, -3) if deblock else (0, 4, 9, 14, 19, 24, 29, 34, 39, 45, 51)):
                R, V, D = views(oracle, w, h, qp, rec, depth, deblock)
                if deblock or blocks is None:
                    blocks = sr.prepare(w, h, src, R, V, D, mutation=mut)
                recs, merge = sr.decide(w, h, blocks, qp, sr.B, 0, fbits, mutation=mut)
                o_recs, o_merge, o_final = oracle_decide(oracle, model_of(oracle, qp, sr.B, 0), w, h, src, rec, depth, deblock)
                if recs != o_recs or merge != o_merge or not np.array_equal(sr.apply(w, h, D, o_recs, mutation=mut), o_final):
                    return
    pytest.fail(f"the atlas cannot see: {sr.MUTATIONS[mut]}")
