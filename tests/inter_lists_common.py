"""Helpers of the scaling-list tests of the inter CTU pass (kvz_hip_dev_inter_ctu_pass_lists, kvazaar's --scaling-list on B pictures): the clips of
tests/golden/inter_scaling_lists.json, the host simulation with both forms of the inter program (tests/hostsim/hostsim_inter_lists.cpp), the chain
I picture -> loop filters -> B pictures -> loop filters -> B-slice coder on the host, and the coverage table of the fixture.  Used by
tests/test_inter_scaling_lists_sim.py, tests/test_gpu_inter_scaling_lists.py, tests/golden/make_inter_scaling_lists_golden.py and tools/bench_inter_scaling_lists.py.
TEST INFRASTRUCTURE -- never imported by the product."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np

import entropy_common as ec
import flatapi
import inter_common as ic
import inter_mixed_common as imc
import scaling_lists as sl
import scaling_lists_common as slc

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "inter_scaling_lists.json")
FLAT = 0xffff  # set_of_picture: the picture stays without lists

# (name, width, height, frames, qp, preset, deblock, sao, owf, clip) as tests/inter_common.py CASES: low-delay encodes (--gop lp-g4d3t1) with --scaling-list default.
# The first six are that file's cases of the same name.  What each is there for:
CLIPS = [
    ("pan", 200, 136, 4, 22, "veryfast", 1, 1, 0, ("motion", 5, 1.5, (1.25, -0.5))),                  # every inter and intra size; filtered pictures and slice data pinned here
    ("noisy-qp27", 200, 136, 4, 27, "veryfast", 1, 1, 0, ("motion", 6, 3.0, (-2.0, 1.75))),           # B pictures on both sides of fast-residual-cost 28
    ("cabac-coeff-cost-qp32", 264, 200, 4, 32, "veryfast", 1, 1, 0, ("motion", 7, 1.0, (0.5, 0.25))),  # the _cabac LISTS build
    ("ultrafast-8mod16", 200, 136, 4, 25, "ultrafast", 1, 0, 2, ("motion", 14, 1.5, (2.5, -1.25))),    # partial CTUs, inter 8x8 at the edges, many intra CUs in B pictures
    ("faster-pan", 200, 136, 4, 22, "faster", 1, 1, 0, ("motion", 5, 1.5, (1.25, -0.5))),             # CABAC cost at every QP
    ("qp0", 200, 136, 3, 0, "veryfast", 1, 1, 0, ("motion", 41, 1.5, (1.25, -0.5))),                  # large levels
    ("binary-qp50-ultrafast", 136, 72, 3, 50, "ultrafast", 1, 0, 0, ("hard", 45, "binary", (3.0, -2.0))),  # B pictures at QP 51: every size on the clip-and-shift-left side
    ("blocks-qp50-veryfast", 136, 72, 3, 50, "veryfast", 1, 1, 0, ("hard", 46, "blocks", (3.0, -2.0))),
    ("binary-qp41", 200, 136, 3, 41, "veryfast", 1, 1, 0, ("hard", 47, "binary", (3.0, -2.0))),      # B pictures at QP 44 and 46: 16x16 on the left side, 32x32 on the right
    ("motion-64x64", 64, 64, 3, 22, "veryfast", 1, 1, 0, ("motion", 48, 1.5, (1.25, -0.5))),          # one CTU
    ("smooth-40x24", 40, 24, 4, 27, "veryfast", 1, 1, 0, ("hard", 44, "smooth", (1.5, -0.75))),       # smaller than a CTU
]
PINNED = "pan"
# digests only: the B picture tools/bench_inter_scaling_lists.py times (picture 1 of BASELINE config 4's sequence, tests/inter_common.py "baseline-c4-2160p")
BENCH_CLIP = "baseline-c4-2160p"
# every block kind and transform size that occurs, on both sides of the dequantiser's branch (coverage()); an intra CU of a B slice is at most 16x16 (pu-depth-intra 2-3)
CELLS = [f"{kind}-{p}-{s}-{side}" for kind, planes in (("inter", (("luma", (8, 16, 32)), ("chroma", (4, 8, 16)))), ("intra", (("luma", (8, 16)), ("chroma", (4, 8)))))
         for p, sizes in planes for s in sizes for side in ("right", "left")]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def fixture():
    return json.load(open(FIXTURE))


def clip_named(name):
    return [c for c in CLIPS if c[0] == name][0]


def picture_qps(clip):
    from kvazaar_amd import inter
    return [inter.lowdelay_picture_qp(clip[4], k) for k in range(clip[3])]


def prices_with_cabac(clip, qp):
    """rdo.c:311-340"""
    return not (qp < ic.PRESETS[clip[5]]["fast_residual_cost"] and qp < 50)


def params_of(clip, qp, poc):
    from kvazaar_amd.inter import InterParams
    name, w, h, n, base_qp, preset, dbk, sao, owf, src = clip
    p = ic.PRESETS[preset]
    return InterParams(qp=int(qp), poc=int(poc), mv_constraint=int(owf > 0), sao=int(sao), deblock=int(dbk), fme_level=p["fme_level"], pu_depth_inter_max=p["pu_depth_inter_max"], no_wpp=0,
                       fast_residual_cost=p["fast_residual_cost"])


def _load_hostsim(unit, units):
    """tests/hostsim/libkvz_<unit>.so from tests/hostsim/<unit>.cpp (which includes `units`), built with the recipe of the other host simulations when it is missing or
    older than a source.  -Bsymbolic, as tests/test_inter_mixed_qp_sim.py builds libkvz_hostsim_inter_models.so: such a library holds a second copy of everything
    in libkvz_hostsim.so, which other tests load with RTLD_GLOBAL, and must bind its calls to its own copy (the program's state is file-static)"""
    d, csrc = os.path.join(flatapi.ROOT, "tests", "hostsim"), os.path.join(flatapi.ROOT, "kvazaar_amd", "csrc")
    so = os.path.join(d, f"libkvz_{unit}.so")
    srcs = [os.path.join(d, f + ".cpp") for f in (unit,) + units] + [os.path.join(flatapi.ROOT, "include", f) for f in ("kvz_hip_types.h", "kvz_hip_dev.h")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = os.path.join(d, f".libkvz_{unit}.{os.getpid()}.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wl,-Bsymbolic", "-o", tmp, os.path.join(d, unit + ".cpp")])
        os.replace(tmp, so)
    return C.CDLL(so)


def load_sim():
    """the simulation with both forms of the inter program and the twin of kvz_hip_dev_inter_ctu_pass_lists"""
    return _load_hostsim("hostsim_inter_lists", ("hostsim_inter_models", "hostsim"))


def load_flat_sim():
    """the simulation of the inter pass built WITHOUT the switch: the library tests/test_inter_mixed_qp_sim.py uses (same file, same recipe, same staleness rule)"""
    return _load_hostsim("hostsim_inter_models", ("hostsim",))


def mul24_violations(sim, reset=False):
    sim.kvz_hostsim_mul24_violations.restype = C.c_ulonglong
    v = int(sim.kvz_hostsim_mul24_violations())
    if reset:
        sim.kvz_hostsim_mul24_reset()
    return v


def sim_pass(sim, pics, params, pictures, sets, set_of_picture, w, h):
    """kvz_hostsim_inter_pass_lists on the pictures `pics` (dicts with src, ref, ref_cu) under the ScalingLists `sets` (set_of_picture: an index per picture, FLAT, or
    None for set 0 everywhere; sets empty: no lists) -> (rc, rec [n, fs], cu [n, h/4, w/4], coeff [n, ctus * 6144]); pictures: InterPictureParams or None"""
    n = len(pics)
    fs, cells, ctus = w * h * 3 // 2, (w // 4) * (h // 4), ((w + 63) // 64) * ((h + 63) // 64)
    fb, wts = imc.model_constants()
    src, ref = imc.stacked(pics, "src"), imc.stacked(pics, "ref")
    ref_cu = np.concatenate([np.ascontiguousarray(p["ref_cu"]).reshape(-1) for p in pics])
    rec, cu, coeff = np.zeros(n * fs, np.uint8), np.zeros(n * cells, ic.CU_DTYPE), np.zeros(n * ctus * 6144, np.int16)
    arr = slc.set_array(sets)
    index = None if set_of_picture is None else (C.c_uint16 * n)(*[int(v) for v in set_of_picture])
    f = sim.kvz_hostsim_inter_pass_lists
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 3 + [C.c_void_p] * 11 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    rc = f(w, h, n, C.addressof(params), pictures.ptr if pictures is not None else None, wts.ctypes.data, fb.ctypes.data, src.ctypes.data, ref.ctypes.data, ref_cu.ctypes.data,
           rec.ctypes.data, cu.ctypes.data, coeff.ctypes.data, None, 0, C.addressof(arr) if sets else None, len(sets), C.addressof(index) if index is not None else None)
    return rc, rec.reshape(n, fs), cu.reshape(n, h // 4, w // 4), coeff.reshape(n, ctus * 6144)


def list_factors(sim, lists_, qp, intra_cu, c, log2w):
    """kvz_hostsim_inter_list_factors: the (forward, inverse) factors quantize_tu takes for every element of a 2^log2w block of plane c"""
    f = sim.kvz_hostsim_inter_list_factors
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    fwd, inv = np.zeros(1 << (2 * log2w), np.int32), np.zeros(1 << (2 * log2w), np.int32)
    f(C.addressof(lists_.struct) if lists_ is not None else None, qp, int(intra_cu), c, log2w, fwd.ctypes.data, inv.ctypes.data)
    return fwd, inv


# ---- the chain on the host
def intra_cu_records(depth, mode, w, h):
    """the CU records of an I picture from the all-intra pass's maps (one entry per 8x8), as the next picture's search reads them"""
    from kvazaar_amd import inter
    cu = inter.intra_picture_cu_info(w, h).reshape(h // 4, w // 4).copy()
    cu["depth"] = np.repeat(np.repeat(depth.reshape(h // 8, w // 8), 2, 0), 2, 1)
    cu["mode"] = np.repeat(np.repeat(mode.reshape(h // 8, w // 8), 2, 0), 2, 1)
    cu["tr_depth"] = np.maximum(cu["depth"], 1)
    return cu


def oracle_loop_filters(oracle, clip, qp, slice_b, src, rec, cu):
    """deblocking, the SAO decision and SAO of one picture by the oracle, as its low-delay flow runs them (oracle/kvz_oracle_inter.inc lowdelay_encode)
    -> (final picture, SAO records [ctus, 3] or None, merge flags or None)"""
    from flatapi import SaoParams, ptr
    from test_encoder_parity import oracle_model
    name, w, h, n, base_qp, preset, dbk, sao, owf, _ = clip
    ctus = ((w + 63) // 64) * ((h + 63) // 64)
    rec = np.ascontiguousarray(rec).copy()
    info = ic.cu_dbk_records(cu)
    if sao:
        model = oracle_model(oracle, qp)
        model.coeff_cabac = int(prices_with_cabac(clip, qp))
        if slice_b:
            init = ic.b_slice_context_states(oracle, qp)
            for i in range(150):
                model.ctx_init[i] = int(init[i])
        luma, chroma, merge = (SaoParams * ctus)(), (SaoParams * ctus)(), np.zeros(ctus, np.uint8)
        f = oracle.lib.kvz_oracle_sao_search_frame_inter
        f.restype = None
        f(C.byref(model), w, h, ptr(src), ptr(rec), info.ctypes.data_as(C.c_void_p), int(slice_b), int(dbk), 0, 0, luma, chroma, ptr(merge))
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
        f(w, h, int(qp), 0, 0, ptr(y), ptr(u), ptr(v), info.ctypes.data_as(C.c_void_p), int(slice_b))
    return rec, None, None


def sim_slice_data(sim, oracle, w, h, qp, poc, cu, ref_cu, coeff, recs, merge):
    """kvz_hostsim_entropy_code_inter: the slice data of one B picture -> (bytes, substream sizes)"""
    f = sim.kvz_hostsim_entropy_code_inter
    f.restype = C.c_long
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_void_p]
    init = ic.b_slice_context_states(oracle, qp)
    out, sizes = np.zeros(w * h * 4 + 4096, np.uint8), np.zeros((h + 63) // 64, np.uint32)
    cu, ref_cu, coeff = np.ascontiguousarray(cu).reshape(-1), np.ascontiguousarray(ref_cu).reshape(-1), np.ascontiguousarray(coeff)
    total = f(init.ctypes.data, w, h, poc, 0, cu.ctypes.data, ref_cu.ctypes.data, coeff.ctypes.data, recs.ctypes.data if recs is not None else None,
              merge.ctypes.data if merge is not None else None, 49152, out.ctypes.data, sizes.ctypes.data)
    assert total >= 0
    return out[:total].tobytes(), [int(v) for v in sizes]


def sim_chain(sim, intra_sim, oracle, lib, clip, set_name="default", slice_data=False):
    """The clip through the host simulations: picture 0 through the LISTS simulation of the all-intra pass at the I picture's QP, the loop filters by the oracle,
    every B picture through kvz_hostsim_inter_pass_lists from the chain's own previous picture, its loop filters, and -- slice_data -- the B-slice coder.
    set_name: a list set of tests/scaling_lists.py, or None for a chain without lists.
    -> dict: final [n] pictures, cu [n] records, coeff [n] levels (None for the I picture), qps, slices [n] of (bytes, sizes) or None"""
    name, w, h, n, base_qp, preset, dbk, sao, owf, _ = clip
    frames, qps = ic.case_frames(clip), picture_qps(clip)
    sets = [slc.lists(set_name)] if set_name else []
    pm = slc.table(lib, [qps[0]], coeff_cabac=int(prices_with_cabac(clip, qps[0])))
    o = slc.sim_pass(intra_sim, pm, sets, None, w, h, [frames[0]])[0]
    cu = intra_cu_records(o["depth"], o["mode"], w, h)
    final, _, _ = oracle_loop_filters(oracle, clip, qps[0], False, frames[0], o["rec"], cu)
    out = dict(final=[final], cu=[cu], coeff=[None], qps=qps, slices=[None], rec=[o["rec"]])
    for k in range(1, n):
        pic = dict(src=frames[k], ref=out["final"][k - 1], ref_cu=out["cu"][k - 1])
        rc, rec, cus, coeff = sim_pass(sim, [pic], params_of(clip, qps[k], k), None, sets, None, w, h)
        assert rc == 0
        final, recs, merge = oracle_loop_filters(oracle, clip, qps[k], True, frames[k], rec[0], cus[0])
        out["rec"].append(rec[0]); out["final"].append(final); out["cu"].append(cus[0]); out["coeff"].append(coeff[0])
        out["slices"].append(sim_slice_data(sim, oracle, w, h, qps[k], k, cus[0], out["cu"][k - 1], coeff[0], recs, merge) if slice_data else None)
    return out


# ---- the coverage table of the fixture
def coverage(cus, coeffs, w, h, qps, set_name="default"):
    """From the records and levels of B pictures at the picture QPs `qps`: the number of non-zero levels at positions whose list entry is not 16 (at 4x4, where the
    default list is flat: all of them), per CU kind, plane kind, transform size and side of the dequantiser's branch ("right": rounded and shifted right, "left":
    clipped and shifted left) -- {"inter-luma-8-right": count, ...}.  A CU of depth d has luma transform units of min(64 >> d, 32) and chroma units of half that (4x4
    for the 8x8 CU); a block's list is (intra CU ? 0 : 3) + plane."""
    s = sl.get(set_name)
    wc = (w + 63) // 64
    out = {}
    for cu, coeff, qp in zip(cus, coeffs, qps):
        cqp = int(slc.flatapi_chroma_qp(qp))
        coeff = coeff.reshape(-1, 6144)
        for y0 in range(0, h, 8):
            for x0 in range(0, w, 8):
                r = cu[y0 // 4, x0 // 4]
                size = 64 >> int(r["depth"])
                if x0 % size or y0 % size or r["type"] not in (1, 2):
                    continue
                tu, intra = min(size, 32), r["type"] == 1
                for ty in range(y0, y0 + size, tu):
                    for tx in range(x0, x0 + size, tu):
                        ctu = coeff[(ty // 64) * wc + tx // 64]
                        for c in range(3):
                            bs = tu if c == 0 else max(tu // 2, 4)
                            l2 = bs.bit_length() - 1
                            lx, ly = (tx % 64) >> (1 if c else 0), (ty % 64) >> (1 if c else 0)
                            base = (0, 4096, 5120)[c] + slc._zorder(lx // 4, ly // 4) * 16
                            levels = ctu[base:base + bs * bs]
                            entries = s.tables(l2, sl.list_type(intra, (0, 2, 3)[c]), 0)[1].astype(np.int64) // sl.INV_QUANT_SCALES[0]
                            count = int(np.count_nonzero(levels[(entries != 16) | (l2 == 2)]))
                            side = "right" if (20 - 14 - (15 - 8 - l2) + 4) > (qp if c == 0 else cqp) // 6 else "left"
                            key = f"{'intra' if intra else 'inter'}-{'luma' if c == 0 else 'chroma'}-{bs}-{side}"
                            out[key] = out.get(key, 0) + count
    return out
