"""Helpers of the tests of P pictures (kvz_hip_dev_inter_ctu_pass_slices / _loop_filters_inter_slices / _entropy_code_inter_slices with KVZ_HIP_SLICE_P: kvazaar's
--no-bipred, the IPPP stream): the clips of tests/golden/inter_p.json, the host simulation with both forms of the inter program
(tests/hostsim/hostsim_inter_p.cpp), the chain I picture -> loop filters -> P pictures -> loop filters -> P-slice coder on the host, and the census of the P
pictures' decisions.  Used by tests/test_inter_p_sim.py, tests/test_gpu_inter_p.py, tests/golden/make_inter_p_golden.py and tools/bench_inter_p.py.
TEST INFRASTRUCTURE -- never imported by the product."""
import ctypes as C
import json
import os

import numpy as np

import entropy_common as ec
import inter_common as ic
import inter_lists_common as ilc
import inter_mixed_common as imc
import scaling_lists_common as slc

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "inter_p.json")
B, P, I = 0, 1, 2  # KVZ_HIP_SLICE_*

# ((name, width, height, frames, qp, preset, deblock, sao, owf, clip) as tests/inter_common.py CASES, the reference encoder's --gop): encodes with --no-bipred
CLIPS = [
    (("pan11", 136, 72, 4, 27, "veryfast", 1, 1, 0, ("motion", 5, 1.5, (11, -6))), "lp-g4d3t1"),                    # deblocking and SAO, P pictures on both sides of fast-residual-cost 28
    (("one-ctu-qp20", 64, 64, 4, 20, "veryfast", 1, 1, 0, ("motion", 48, 1.5, (5, -3))), "lp-g4d3t1"),              # kvz_fast_coeff_cost: the _p_fast build
    (("pan9-qp32-owf2", 136, 72, 4, 32, "veryfast", 1, 1, 2, ("motion", 7, 1.0, (-9, 7))), "lp-g4d3t1"),            # the _p_cabac build under the MV constraint
    (("pan37-owf2", 200, 136, 3, 27, "ultrafast", 1, 0, 2, ("motion", 5, 1.5, (37, -18))), "lp-g4d3t1"),            # vectors leaving the frame; no fractional search
    (("faster-qp24", 136, 72, 4, 24, "faster", 1, 1, 0, ("motion", 9, 1.5, (2.25, -1.5))), "lp-g4d3t1"),            # subme 4, CABAC pricing at every QP
    (("blocks-72x40", 72, 40, 4, 30, "veryfast", 0, 0, 0, ("hard", 46, "blocks", (3.0, -2.0))), "lp-g4d3t1"),       # content that forces intra CUs; no loop filter at all
    (("tiny-qp51", 24, 16, 4, 51, "veryfast", 1, 1, 0, ("hard", 44, "smooth", (2.75, -1.25))), "lp-g4d3t1"),       # smaller than a CTU, at both ends of the QP range
    (("tiny-qp0", 24, 16, 4, 0, "veryfast", 1, 1, 0, ("hard", 44, "smooth", (2.75, -1.25))), "lp-g4d3t1"),         # (a slower pan encodes alike with and without --no-bipred at QP 0)
    (("static-qp30", 136, 72, 3, 30, "veryfast", 1, 1, 0, ("motion", 12, 0.0, (0.0, 0.0))), "lp-g4d3t1"),             # nothing moves: 32x32 CUs, skips by the zero candidate
    (("pan11-gop0", 136, 72, 4, 27, "veryfast", 1, 1, 0, ("motion", 5, 1.5, (11, -6))), "0"),                       # --gop 0: every picture at the sequence QP
]
# what the census of the P pictures' decisions counts (kvz_hostsim_p_census), and what must occur at least CENSUS_MIN times over the set
CENSUS = ("intra_cus", "skipped_cus", "merged_idx0", "merged_idx_above0", "temporal_merge_chosen", "zero_merge_chosen", "amvp_mvp_idx0", "amvp_mvp_idx1", "fractional_vectors",
          "depth1_cus", "depth2_cus", "depth3_cus", "inter_cus_with_residual", "root_cbf0_not_merged", "mv_dir_not_1", "merge_list_unknown")
CENSUS_REQUIRED, CENSUS_MIN = CENSUS[:14], 16
# the three 136x72 clips of one preset and the same switches whose P pictures share one device launch at their own QP and POC (QPs on both sides of 28)
SHARED_LAUNCH = ("pan11", "static-qp30", "pan11-gop0")


def fixture():
    return json.load(open(FIXTURE))


def clip_named(name):
    return [c for c, _ in CLIPS if c[0] == name][0]


def gop_of(name):
    return [g for c, g in CLIPS if c[0] == name][0]


def names():
    return [c[0] for c, _ in CLIPS]


def picture_qps(clip, gop):
    """the QP of every picture of the encode: kvazaar's low-delay GOP layers, or -- --gop 0 -- the sequence QP (no GOP: no layer offsets, intra_qp_offset 0)"""
    return [int(clip[4])] * clip[3] if gop == "0" else ilc.picture_qps(clip)


def params_of(clip, qp, poc):
    return ilc.params_of(clip, qp, poc)


def load_sim():
    """the simulation with both forms of the inter program, B and P, and the twins of the entry points that take a slice type"""
    return ilc._load_hostsim("hostsim_inter_p", ("hostsim_inter_models", "hostsim"))


def slice_contexts(sim, slice_type, qp):
    """the 168 initial context states of a B or P slice at `qp` in the coder's numbering, as the library fills them (kvz_slice_contexts.hpp)"""
    f = sim.kvz_hostsim_slice_contexts
    f.restype = None
    f.argtypes = [C.c_int, C.c_int, C.c_void_p]
    out = np.zeros(176, np.uint8)
    f(int(slice_type), int(qp), out.ctypes.data)
    return out[:168].copy()


def slices_check(sim, params, slice_type, stage, has_tile_xy=False):
    """the twin of what the entry point of `stage` ("pass", "loop_filters", "coder") refuses of the slice type: 0 accepted, -1 refused"""
    f = sim.kvz_hostsim_inter_slices_check
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    return f(C.addressof(params), int(has_tile_xy), int(slice_type), ("pass", "loop_filters", "coder").index(stage))


def sim_pass(sim, pics, params, pictures, w, h, slice_type=P, tile_xy=None, out=None):
    """kvz_hostsim_inter_pass_slices on the pictures `pics` (dicts with src, ref, ref_cu) -> (rc, rec [n, fs], cu [n, h/4, w/4], coeff [n, ctus * 6144]).
    out: (rec, cu, coeff) flat arrays to write into instead of fresh zeroed ones"""
    n = len(pics)
    fs, cells, ctus = w * h * 3 // 2, (w // 4) * (h // 4), ((w + 63) // 64) * ((h + 63) // 64)
    fb, wts = imc.model_constants()
    src, ref = imc.stacked(pics, "src"), imc.stacked(pics, "ref")
    ref_cu = np.concatenate([np.ascontiguousarray(p["ref_cu"]).reshape(-1) for p in pics])
    rec, cu, coeff = out if out is not None else (np.zeros(n * fs, np.uint8), np.zeros(n * cells, ic.CU_DTYPE), np.zeros(n * ctus * 6144, np.int16))
    xy = None if tile_xy is None else np.ascontiguousarray(tile_xy, np.int32)
    f = sim.kvz_hostsim_inter_pass_slices
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 3 + [C.c_void_p] * 11 + [C.c_int, C.c_int]
    rc = f(w, h, n, C.addressof(params), pictures.ptr if pictures is not None else None, wts.ctypes.data, fb.ctypes.data, src.ctypes.data, ref.ctypes.data, ref_cu.ctypes.data,
           rec.ctypes.data, cu.ctypes.data, coeff.ctypes.data, xy.ctypes.data if xy is not None else None, 0, int(slice_type))
    return rc, rec.reshape(n, fs), cu.reshape(n, h // 4, w // 4), coeff.reshape(n, ctus * 6144)


def census(sim, cu, w, h, picture=0, into=None):
    """kvz_hostsim_p_census of picture `picture` of the simulation's LAST P launch, from that picture's records -> {name: count}, added to `into`"""
    f = sim.kvz_hostsim_p_census
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    out = (C.c_ulonglong * 16)()
    cu = np.ascontiguousarray(cu).reshape(-1)
    f(cu.ctypes.data, w, h, int(picture), out)
    into = {} if into is None else into
    for i, k in enumerate(CENSUS):
        into[k] = into.get(k, 0) + int(out[i])
    return into


def sim_slice_data(sim, slice_type, w, h, qps, pocs, cu, ref_cu, coeff, recs, merge, no_wpp=0):
    """kvz_hostsim_entropy_code_inter_slices: the slice data of len(qps) pictures (records, levels, SAO decisions back to back) -> (bytes, substream sizes), or None
    when the coder refuses the slice type"""
    f = sim.kvz_hostsim_entropy_code_inter_slices
    f.restype = C.c_long
    f.argtypes = [C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_void_p]
    n = len(qps)
    qp_a, poc_a = np.ascontiguousarray(qps, np.int32), np.ascontiguousarray(pocs, np.int32)
    out, sizes = np.zeros(n * (w * h * 4 + 4096), np.uint8), np.zeros(n * (1 if no_wpp else (h + 63) // 64), np.uint32)
    cu, ref_cu, coeff = np.ascontiguousarray(cu).reshape(-1), np.ascontiguousarray(ref_cu).reshape(-1), np.ascontiguousarray(coeff).reshape(-1)
    total = f(int(slice_type), qp_a.ctypes.data, poc_a.ctypes.data, w, h, n, int(no_wpp), cu.ctypes.data, ref_cu.ctypes.data, coeff.ctypes.data,
              recs.ctypes.data if recs is not None else None, merge.ctypes.data if merge is not None else None, 49152, out.ctypes.data, sizes.ctypes.data)
    if total < 0:
        return None
    return out[:total].tobytes(), [int(v) for v in sizes]


def oracle_loop_filters(sim, oracle, clip, qp, slice_type, src, rec, cu):
    """deblocking, the SAO decision and SAO of one picture by the oracle (tests/inter_lists_common.py oracle_loop_filters) for a slice type: a P picture is deblocked
    under the rule of every slice that is not B, and its SAO decision starts from the context states of the P row
    -> (final picture, SAO records [ctus, 3] or None, merge flags or None)"""
    if slice_type != P:
        return ilc.oracle_loop_filters(oracle, clip, qp, slice_type == B, src, rec, cu)
    from flatapi import SaoParams, ptr
    from test_encoder_parity import oracle_model
    name, w, h, n, base_qp, preset, dbk, sao, owf, _ = clip
    ctus = ((w + 63) // 64) * ((h + 63) // 64)
    rec = np.ascontiguousarray(rec).copy()
    info = ic.cu_dbk_records(cu)
    if sao:
        model = oracle_model(oracle, qp)
        model.coeff_cabac = int(ilc.prices_with_cabac(clip, qp))
        init = slice_contexts(sim, P, qp)
        for i in range(150):
            model.ctx_init[i] = int(init[i])
        luma, chroma, merge = (SaoParams * ctus)(), (SaoParams * ctus)(), np.zeros(ctus, np.uint8)
        f = oracle.lib.kvz_oracle_sao_search_frame_inter
        f.restype = None
        f(C.byref(model), w, h, ptr(src), ptr(rec), info.ctypes.data_as(C.c_void_p), 0, int(dbk), 0, 0, luma, chroma, ptr(merge))
        final = rec.copy()
        g = oracle.lib.kvz_oracle_sao_frame
        g.restype = None
        g(w, h, ptr(rec), ptr(final), luma, chroma)
        return final, ec.pack_sao_records(luma, chroma, ctus), merge
    if dbk:
        ys = w * h
        y, u, v = rec[:ys], rec[ys:ys + ys // 4], rec[ys + ys // 4:]
        f = oracle.lib.kvz_oracle_deblock_frame_inter
        f.restype = None
        f(w, h, int(qp), 0, 0, ptr(y), ptr(u), ptr(v), info.ctypes.data_as(C.c_void_p), 0)
    return rec, None, None


_intra = {}


def intra_picture(intra_sim, oracle, lib, clip, gop):
    """picture 0 of the clip through the simulation of the all-intra pass and the oracle's loop filters -> (frames, qps, final picture, CU records), as
    tests/inter_me_common.py intra_picture makes it, at the I picture's QP under `gop`"""
    name, w, h, n, base_qp, preset, dbk, sao, owf, _ = clip
    if name not in _intra:
        frames, qps = ic.case_frames(clip), picture_qps(clip, gop)
        pm = slc.table(lib, [qps[0]], coeff_cabac=int(ilc.prices_with_cabac(clip, qps[0])))
        o = slc.sim_pass(intra_sim, pm, [], None, w, h, [frames[0]])[0]
        cu = ilc.intra_cu_records(o["depth"], o["mode"], w, h)
        final, _, _ = ilc.oracle_loop_filters(oracle, clip, qps[0], False, frames[0], o["rec"], cu)
        final.setflags(write=False)
        _intra[name] = (frames, qps, final, cu)
    return _intra[name]


def sim_chain(sim, intra_sim, oracle, lib, clip, gop, slice_type=P, counts=None):
    """The clip through the host simulations: picture 0 as intra_picture, every later picture as a picture of `slice_type` through kvz_hostsim_inter_pass_slices from
    the chain's own previous picture, the oracle's loop filters for the slice type, the coder simulation for the slice type.  counts: a dict the census of the P
    pictures is added to.
    -> dict: final [n] pictures, rec [n], cu [n], coeff [n] (None for the I picture), qps, slices [n] of (bytes, sizes) or None"""
    name, w, h, n, base_qp, preset, dbk, sao, owf, _ = clip
    frames, qps, final0, cu0 = intra_picture(intra_sim, oracle, lib, clip, gop)
    out = dict(final=[final0], cu=[cu0], coeff=[None], qps=qps, slices=[None], rec=[None])
    for k in range(1, n):
        pic = dict(src=frames[k], ref=out["final"][k - 1], ref_cu=out["cu"][k - 1])
        rc, rec, cus, coeff = sim_pass(sim, [pic], params_of(clip, qps[k], k), None, w, h, slice_type)
        assert rc == 0, (name, k, rc)
        if counts is not None and slice_type == P:
            census(sim, cus[0], w, h, 0, counts)
        final, recs, merge = oracle_loop_filters(sim, oracle, clip, qps[k], slice_type, frames[k], rec[0], cus[0])
        out["rec"].append(rec[0]); out["final"].append(final); out["cu"].append(cus[0]); out["coeff"].append(coeff[0])
        out["slices"].append(sim_slice_data(sim, slice_type, w, h, [qps[k]], [k], cus[0], out["cu"][k - 1], coeff[0], recs, merge))
    return out


def assert_chain_equals_fixture(chain, entry, what):
    """every final picture and every P picture's slice data against the fixture's entry of the case"""
    assert chain["qps"] == entry["qps"], what
    for k, final in enumerate(chain["final"]):
        assert ilc.sha(final) == entry["rec"][k], (what, k, "picture")
        if k > 0:
            data, sizes = chain["slices"][k]
            assert sizes == entry["slices"][k]["sizes"] and ilc.sha(np.frombuffer(data, np.uint8)) == entry["slices"][k]["sha"], (what, k, "slice data")
