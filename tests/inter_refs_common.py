"""Helpers of the tests of P pictures with reference lists of 1 to 4 pictures (kvz_hip_dev_inter_ctu_pass_refs / _loop_filters_inter_refs / _entropy_code_inter_refs:
kvazaar's --no-bipred --ref N): the clips of tests/golden/inter_refs.json -- among them one that alternates two scenes, so that the second entry of a list is the
better reference --, the host simulation with every form of the inter program (tests/hostsim/hostsim_inter_refs.cpp), the chain I picture -> loop filters -> P
pictures with their pools -> loop filters -> P-slice coder on the host, and the census of what the program met of the lists.  Used by tests/test_inter_refs_sim.py,
tests/test_gpu_inter_refs.py, tests/golden/make_inter_refs_golden.py and tools/bench_inter_refs.py.
TEST INFRASTRUCTURE -- never imported by the product."""
import ctypes as C
import json
import os

import numpy as np

import inter_common as ic
import inter_lists_common as ilc
import inter_mixed_common as imc
import inter_p_common as pc
import scaling_lists_common as slc

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "inter_refs.json")
P = pc.P

# the clip that alternates two scenes: even pictures from one pan, odd ones from another (seed, noise, pan of each) -- a picture resembles the one before the previous
ALTERNATING = ("alternating", (5, 1.5, (3.0, -1.5)), (23, 1.5, (-2.25, 1.0)))
ALT8 = ("alt", 136, 72, 8, 27, "veryfast", 1, 1, 0, ALTERNATING)
# ((name, width, height, frames, qp, preset, deblock, sao, owf, clip) as tests/inter_common.py CASES, --gop, --ref): encodes with --no-bipred.  The first seven clips
# are those of tests/inter_p_common.py; never --gop lp-g4d3t1 --ref 4, which selects kvazaar's fixed lowdelay4 table (encoder.c:172)
CASES = [
    ("pan11", pc.clip_named("pan11"), "lp-g4d3t1", 2),
    ("one-ctu-qp20", pc.clip_named("one-ctu-qp20"), "lp-g4d3t1", 2),
    ("faster-qp24", pc.clip_named("faster-qp24"), "lp-g4d3t1", 2),
    ("blocks-72x40", pc.clip_named("blocks-72x40"), "lp-g4d3t1", 2),
    ("tiny-qp51", pc.clip_named("tiny-qp51"), "lp-g4d3t1", 2),
    ("tiny-qp0", pc.clip_named("tiny-qp0"), "lp-g4d3t1", 2),
    ("pan9-qp32-owf2", pc.clip_named("pan9-qp32-owf2"), "lp-g4d3t1", 2),     # the MV constraint
    ("alt-g4-ref2", ALT8, "lp-g4d3t1", 2),
    ("alt-gop0-ref2", ALT8, "0", 2),
    ("alt-gop0-ref3", ALT8, "0", 3),
    ("alt-g8-ref4", ("alt10", 136, 72, 10, 27, "veryfast", 1, 1, 0, ALTERNATING), "lp-g8d4t1", 4),  # (ten pictures of this GOP hold lists of two: the buffer drops what a picture does not ask for, the third key picture comes at POC 16)
    ("alt-g4-ref3", ALT8, "lp-g4d3t1", 3),
    ("alt-gop0-ref4", ("alt6", 96, 56, 6, 30, "veryfast", 1, 1, 0, ALTERNATING), "0", 4),             # a list of four: pictures 4 and 5
]
CENSUS = ("ref_idx1_searched", "merged_ref_idx_above0", "skipped_ref_idx_above0", "zero_merge_ref_idx_above0_chosen", "ref_idx_second_context_bin", "ref_idx_2_or_3",
          "ref_idx_outside_list", "spatial_amvp_scaled", "temporal_scaled", "zero_merge_ref_idx_above0_evaluated")
# what must occur at least this often over the set
CENSUS_MIN = {"ref_idx1_searched": 16, "merged_ref_idx_above0": 16, "skipped_ref_idx_above0": 16, "spatial_amvp_scaled": 16, "temporal_scaled": 16,
              "zero_merge_ref_idx_above0_evaluated": 16, "ref_idx_second_context_bin": 16, "ref_idx_2_or_3": 4}
SMALLEST = ("tiny-qp51", "tiny-qp0", "alt-gop0-ref4")  # device == simulation on records and levels


def fixture():
    return json.load(open(FIXTURE))


def names():
    return [c[0] for c in CASES]


def case_named(name):
    return [c for c in CASES if c[0] == name][0]


def case_frames(clip):
    src = clip[9]
    if src[0] != "alternating":
        return ic.case_frames(clip)
    name, w, h, n = clip[:4]
    a, b = ic.clip(w, h, n, *src[1]), ic.clip(w, h, n, *src[2])
    return [a[k] if k % 2 == 0 else b[k] for k in range(n)]


def gop_shape(gop):
    """(length, depth) of --gop lp-g<len>d<depth>t1"""
    return int(gop[4:gop.index("d")]), int(gop[gop.index("d") + 1:gop.index("t")])


def picture_qps(clip, gop):
    from kvazaar_amd import inter
    if gop == "0":
        return [int(clip[4])] * clip[3]
    g, d = gop_shape(gop)
    return [inter.lowdelay_picture_qp(clip[4], k, gop_len=g, gop_depth=d) for k in range(clip[3])]


def load_sim():
    """the simulation with every form of the inter program -- B, P, P with reference lists -- and the twins of the entry points that take the lists"""
    return ilc._load_hostsim("hostsim_inter_refs", ("hostsim_inter_p", "hostsim_inter_models", "hostsim"))


def references_of(pool, lists, n_frames=None):
    """InterReferences for pictures whose lists name frames of `pool`: pool = [(poc, [the POCs that frame's own list named])], lists = [[pool index, ...]]"""
    from kvazaar_amd.inter import InterReferences
    return InterReferences([p for p, _ in pool], [r for _, r in pool], [len(l) for l in lists], lists)


def refs_check(sim, params, slice_type, stage, n_pictures, pictures, references, has_tile_xy=False):
    """the twin of what the entry point of `stage` ("pass", "loop_filters", "coder") refuses: 0 accepted, -1 refused"""
    f = sim.kvz_hostsim_inter_refs_check
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return f(C.addressof(params), int(has_tile_xy), int(slice_type), ("pass", "loop_filters", "coder").index(stage), int(n_pictures), pictures.ptr if pictures is not None else None,
             references.ptr if references is not None else None)


def sim_pass(sim, srcs, pool_frames, pool_cus, params, pictures, references, w, h, slice_type=P):
    """kvz_hostsim_inter_pass_refs: the pictures `srcs` over the pool (frames, their CU records) -> (rc, rec [n, fs], cu [n, h/4, w/4], coeff [n, ctus * 6144])"""
    n = len(srcs)
    fs, cells, ctus = w * h * 3 // 2, (w // 4) * (h // 4), ((w + 63) // 64) * ((h + 63) // 64)
    fb, wts = imc.model_constants()
    src = np.concatenate([np.ascontiguousarray(s).reshape(-1) for s in srcs])
    ref = np.concatenate([np.ascontiguousarray(f).reshape(-1) for f in pool_frames])
    ref_cu = np.concatenate([np.ascontiguousarray(c).reshape(-1) for c in pool_cus])
    rec, cu, coeff = np.zeros(n * fs, np.uint8), np.zeros(n * cells, ic.CU_DTYPE), np.zeros(n * ctus * 6144, np.int16)
    f = sim.kvz_hostsim_inter_pass_refs
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 3 + [C.c_void_p] * 11 + [C.c_int, C.c_int, C.c_void_p]
    rc = f(w, h, n, C.addressof(params), pictures.ptr if pictures is not None else None, wts.ctypes.data, fb.ctypes.data, src.ctypes.data, ref.ctypes.data, ref_cu.ctypes.data,
           rec.ctypes.data, cu.ctypes.data, coeff.ctypes.data, None, 0, int(slice_type), references.ptr if references is not None else None)
    return rc, rec.reshape(n, fs), cu.reshape(n, h // 4, w // 4), coeff.reshape(n, ctus * 6144)


def events(sim, reset=False):
    """what the program met of the lists since the last reset: (spatial AMVP candidates scaled, temporal candidates scaled, zero merge candidates of a reference index
    above 0 evaluated)"""
    out = (C.c_ulonglong * 8)()
    sim.kvz_hostsim_refs_events.restype = None
    sim.kvz_hostsim_refs_events.argtypes = [C.c_void_p, C.c_int]
    sim.kvz_hostsim_refs_events(out, int(reset))
    return int(out[0]), int(out[1]), int(out[2])


def census(sim, cu, w, h, n_refs, picture=0, into=None):
    """kvz_hostsim_refs_census of picture `picture` of the simulation's LAST launch with lists, from that picture's records -> {name: count}, added to `into`"""
    f = sim.kvz_hostsim_refs_census
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    out = (C.c_ulonglong * 8)()
    cu = np.ascontiguousarray(cu).reshape(-1)
    f(cu.ctypes.data, w, h, int(picture), int(n_refs), out)
    into = {} if into is None else into
    for i, k in enumerate(CENSUS[:7]):
        into[k] = into.get(k, 0) + int(out[i])
    return into


def sim_slice_data(sim, w, h, qps, pocs, cu, pool_cus, coeff, recs, merge, references, no_wpp=0):
    """kvz_hostsim_entropy_code_inter_refs: the slice data of len(qps) P pictures over the pool's records -> (bytes, substream sizes), or None when refused"""
    f = sim.kvz_hostsim_entropy_code_inter_refs
    f.restype = C.c_long
    f.argtypes = [C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    n = len(qps)
    qp_a, poc_a = np.ascontiguousarray(qps, np.int32), np.ascontiguousarray(pocs, np.int32)
    out, sizes = np.zeros(n * (w * h * 4 + 4096), np.uint8), np.zeros(n * (1 if no_wpp else (h + 63) // 64), np.uint32)
    cu, coeff = np.ascontiguousarray(cu).reshape(-1), np.ascontiguousarray(coeff).reshape(-1)
    ref_cu = np.concatenate([np.ascontiguousarray(c).reshape(-1) for c in pool_cus])
    total = f(P, qp_a.ctypes.data, poc_a.ctypes.data, w, h, n, int(no_wpp), cu.ctypes.data, ref_cu.ctypes.data, coeff.ctypes.data,
              recs.ctypes.data if recs is not None else None, merge.ctypes.data if merge is not None else None, 49152, out.ctypes.data, sizes.ctypes.data,
              references.ptr if references is not None else None)
    if total < 0:
        return None
    return out[:total].tobytes(), [int(v) for v in sizes]


_intra = {}


def intra_picture(intra_sim, oracle, lib, case):
    """picture 0 of the case through the simulation of the all-intra pass and the oracle's loop filters -> (frames, qps, final picture, CU records), as
    tests/inter_p_common.py intra_picture makes it, at the I picture's QP under the case's GOP"""
    key, clip, gop, ref = case
    name, w, h, n, base_qp, preset, dbk, sao, owf, _ = clip
    if key not in _intra:
        frames, qps = case_frames(clip), picture_qps(clip, gop)
        pm = slc.table(lib, [qps[0]], coeff_cabac=int(ilc.prices_with_cabac(clip, qps[0])))
        o = slc.sim_pass(intra_sim, pm, [], None, w, h, [frames[0]])[0]
        cu = ilc.intra_cu_records(o["depth"], o["mode"], w, h)
        final, _, _ = ilc.oracle_loop_filters(oracle, clip, qps[0], False, frames[0], o["rec"], cu)
        final.setflags(write=False)
        _intra[key] = (frames, qps, final, cu)
    return _intra[key]


def picture_references(k, ref_pocs_of, ref, gop):
    """picture k's list as (pool [(poc, that frame's own list)], InterReferences): the pool holds exactly the list's frames, in list order"""
    from kvazaar_amd import inter
    pocs = inter.reference_pocs(k, ref, gop)
    pool = [(p, ref_pocs_of[p]) for p in pocs]
    return pocs, references_of(pool, [list(range(len(pocs)))])


def sim_chain(sim, intra_sim, oracle, lib, case, counts=None):
    """The case through the host simulations: picture 0 as intra_picture, every later picture as a P picture through kvz_hostsim_inter_pass_refs from the chain's own
    earlier pictures -- those kvazaar's --gop / --ref put into its list --, the oracle's loop filters for a P slice, the coder simulation with the lists.
    counts: a dict the census is added to.
    -> dict: final [n] pictures, rec [n], cu [n], coeff [n] (None for the I picture), qps, slices [n] of (bytes, sizes) or None, lists [n] of POCs"""
    from kvazaar_amd.inter import InterPictureParams
    key, clip, gop, ref = case
    name, w, h, n, base_qp, preset, dbk, sao, owf, _ = clip
    frames, qps, final0, cu0 = intra_picture(intra_sim, oracle, lib, case)
    out = dict(final=[final0], cu=[cu0], coeff=[None], qps=qps, slices=[None], rec=[None], lists=[[]])
    ref_pocs_of = {0: []}
    for k in range(1, n):
        pocs, references = picture_references(k, ref_pocs_of, ref, gop)
        pool_frames, pool_cus = [out["final"][p] for p in pocs], [out["cu"][p] for p in pocs]
        pictures = InterPictureParams([qps[k]], [k])
        if counts is not None:
            events(sim, reset=True)
        rc, rec, cus, coeff = sim_pass(sim, [frames[k]], pool_frames, pool_cus, pc.params_of(clip, qps[k], k), pictures, references, w, h)
        assert rc == 0, (key, k, rc)
        if counts is not None:
            census(sim, cus[0], w, h, len(pocs), 0, counts)
            for name_, v in zip(CENSUS[7:], events(sim)):
                counts[name_] = counts.get(name_, 0) + v
        final, recs, merge = pc.oracle_loop_filters(sim, oracle, clip, qps[k], P, frames[k], rec[0], cus[0])
        out["rec"].append(rec[0]); out["final"].append(final); out["cu"].append(cus[0]); out["coeff"].append(coeff[0]); out["lists"].append(pocs)
        out["slices"].append(sim_slice_data(sim, w, h, [qps[k]], [k], cus[0], pool_cus, coeff[0], recs, merge, references))
        ref_pocs_of[k] = pocs
    return out


def assert_chain_equals_fixture(chain, entry, what):
    """every final picture and every P picture's slice data against the fixture's entry of the case"""
    assert chain["qps"] == entry["qps"], what
    for k, final in enumerate(chain["final"]):
        assert ilc.sha(final) == entry["rec"][k], (what, k, "picture")
        if k > 0:
            data, sizes = chain["slices"][k]
            assert sizes == entry["slices"][k]["sizes"] and ilc.sha(np.frombuffer(data, np.uint8)) == entry["slices"][k]["sha"], (what, k, "slice data")
