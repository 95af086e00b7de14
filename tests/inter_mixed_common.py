"""Launches of the inter path whose pictures have a QP and a POC of their own (kvz_hip_inter_pictures), as tests/test_inter_mixed_qp_sim.py (host simulation) and
tests/test_gpu_inter_mixed_qp.py (device) build them: B pictures drawn from low-delay sequences that were encoded ALONE by the oracle (inter_common.oracle_encode*, the
oracle pinned to the reference encoder), at different --qp and from different positions of the GOP.  Every picture of a mixed launch stays an ordinary constant-QP picture,
so its expected outputs are those of its own sequence's encode; nothing here is computed by the code under test."""
import ctypes as C
import functools

import numpy as np

import ctu_common as cc
import flatapi
import inter_common as ic

W, H, FRAMES = 264, 200, 4  # 5x4 CTUs, partial CTUs on both edges, width 8 mod 16; an I picture and the B pictures POC 1, 2, 3
SEQUENCE_QPS = (17, 22, 27, 32, 37)  # --qp of the sequences: 27 runs its B pictures on both sides of fast-residual-cost 28


@functools.lru_cache(maxsize=None)
def sequence(qp, preset="veryfast", seed=0, w=W, h=H, n=FRAMES, no_wpp=False, mv_constraint=True, parts=True):
    """one low-delay sequence at --qp `qp`, encoded alone by the oracle -> dict: frames, rs (before the loop filters), rf (final), cu, qps (picture QPs) and -- parts --
    levels, SAO decisions and slice data of every picture.  Shared and never modified."""
    oracle = flatapi.load_oracle()
    frames = ic.clip(w, h, n, 100 + seed)
    kw = dict(preset=preset, deblock=True, sao=True, mv_constraint=mv_constraint, no_wpp=no_wpp)
    rs, rf, cu, qps = ic.oracle_encode(oracle, w, h, frames, qp, **kw)
    s = dict(frames=frames, rs=rs, rf=rf, cu=cu, qps=[int(q) for q in qps], w=w, h=h, preset=preset)
    if parts:
        s["parts"] = ic.oracle_encode_parts(oracle, w, h, frames, qp, **kw)
        s["bits"] = ic.oracle_encode_bits(oracle, w, h, frames, qp, **kw)
        assert [int(q) for q in s["parts"]["qps"]] == s["qps"]
    for v in (rs, rf, cu):
        v.setflags(write=False)
    return s


def picture(seq, k):
    """B picture k of a sequence as one picture of a launch: inputs from the oracle's previous picture, expected outputs from the oracle's picture k"""
    p = dict(src=seq["frames"][k], ref=seq["rf"][k - 1], ref_cu=seq["cu"][k - 1], rec=seq["rs"][k], final=seq["rf"][k], cu=seq["cu"][k], qp=seq["qps"][k], poc=k, seq=seq, k=k)
    if "parts" in seq:
        p["coeff"] = seq["parts"]["coeff"][k]
    return p


def veryfast_pictures():
    """CPU case 1 / GPU case 1: two pictures of each of the five sequences, from GOP positions that differ between neighbouring sequences"""
    pics = []
    for i, qp in enumerate(SEQUENCE_QPS):
        s = sequence(qp, seed=i)
        pics += [picture(s, 1 + i % 3), picture(s, 1 + (i + 1) % 3)]
    return pics


def launch_params(preset, no_wpp=0, mv_constraint=1, sao=1, deblock=1, **tile):
    """the launch's kvz_hip_inter_params; qp / poc hold values no picture has, so a launch that took them instead of the table's cannot pass"""
    from kvazaar_amd.inter import InterParams
    p = ic.PRESETS[preset]
    return InterParams(qp=45, poc=9, mv_constraint=mv_constraint, sao=sao, deblock=deblock, fme_level=p["fme_level"], pu_depth_inter_max=p["pu_depth_inter_max"], no_wpp=no_wpp,
                       fast_residual_cost=p["fast_residual_cost"], **tile)


def stacked(pics, key, dtype=None):
    a = np.concatenate([np.ascontiguousarray(p[key]).reshape(-1) for p in pics])
    return a if dtype is None else a.astype(dtype)


def model_constants():
    mc = cc.model_constants()
    return np.array(mc["entropy_fbits"], np.float32), np.array([int(mc["coeff_weights"][str(q)]) for q in range(52)], np.uint64)


def hostsim_pass(sim, pics, params, pictures, w=W, h=H, tile_xy=None, n_references=0, ref=None, ref_cu=None):
    """kvz_hostsim_inter_pass_pictures -> (rc, rec [n, fs], cu [n, h/4, w/4], coeff [n, ctus * 6144]); pictures: InterPictureParams or None"""
    n = len(pics)
    fs, cells, ctus = w * h * 3 // 2, (w // 4) * (h // 4), ((w + 63) // 64) * ((h + 63) // 64)
    fb, wts = model_constants()
    src = stacked(pics, "src")
    ref = stacked(pics, "ref") if ref is None else ref
    ref_cu = np.concatenate([np.ascontiguousarray(p["ref_cu"]).reshape(-1) for p in pics]) if ref_cu is None else ref_cu
    rec, cu, coeff = np.zeros(n * fs, np.uint8), np.zeros(n * cells, ic.CU_DTYPE), np.zeros(n * ctus * 6144, np.int16)
    f = sim.kvz_hostsim_inter_pass_pictures
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 3 + [C.c_void_p] * 11 + [C.c_int]
    xy = None if tile_xy is None else np.ascontiguousarray(tile_xy, np.int32)
    rc = f(w, h, n, C.addressof(params), pictures.ptr if pictures is not None else None, wts.ctypes.data, fb.ctypes.data, src.ctypes.data, ref.ctypes.data, ref_cu.ctypes.data,
           rec.ctypes.data, cu.ctypes.data, coeff.ctypes.data, xy.ctypes.data if xy is not None else None, n_references)
    return rc, rec.reshape(n, fs), cu.reshape(n, h // 4, w // 4), coeff.reshape(n, ctus * 6144)


def assert_pictures_equal_the_oracle(pics, rec, cu):
    """reconstruction and CU records of every picture against its own sequence's encode.  (Levels are compared through the slice data -- assert_slice_data -- not buffer
    against buffer: the oracle's buffer keeps the levels of transform units whose coded block flag the zero-coefficient decision cleared afterwards, the pass writes zeros
    there, and nothing reads them; 3 of 122 880 values of the first --qp 17 picture, the same through the single-QP entry point.)"""
    for i, p in enumerate(pics):
        where = (i, p["qp"], p["poc"])
        assert ic.first_difference(cu[i][None], np.asarray(p["cu"])[None]) is None, where
        assert np.array_equal(rec[i], p["rec"]), where


def entropy_tables(pics):
    """what kvz_hip_dev_entropy_code_inter_pictures derives from the table, from the oracle: a row of B-slice context states per distinct QP, the row and POC of every picture"""
    oracle = flatapi.load_oracle()
    qps = sorted({p["qp"] for p in pics})
    rows = np.zeros((len(qps), 176), np.uint8)
    for r, q in enumerate(qps):
        rows[r, :168] = ic.b_slice_context_states(oracle, q)
    return rows, np.array([qps.index(p["qp"]) for p in pics], np.uint16), np.array([p["poc"] for p in pics], np.int32)


def hostsim_slice_data(sim, pics, cu, coeff, w=W, h=H):
    """kvz_hostsim_entropy_code_inter_pictures over the launch: cu [n, ...] / coeff [n, ...] of the pictures (the pass's, or the oracle's), reference records and SAO
    decisions from the oracle -> (bytes, sizes [n, rows])"""
    import entropy_common as ec
    rows, row_of, pocs = entropy_tables(pics)
    n, ctus, hc = len(pics), ((w + 63) // 64) * ((h + 63) // 64), (h + 63) // 64
    cu = np.ascontiguousarray(cu).reshape(-1)
    coeff = np.ascontiguousarray(coeff).reshape(-1)
    ref_cu = np.concatenate([np.ascontiguousarray(p["seq"]["parts"]["cu"][p["k"] - 1]) for p in pics])
    recs = np.concatenate([ec.pack_sao_records(np.ascontiguousarray(p["seq"]["parts"]["sao_luma"][p["k"]]), np.ascontiguousarray(p["seq"]["parts"]["sao_chroma"][p["k"]]), ctus) for p in pics])
    merge = np.concatenate([np.ascontiguousarray(p["seq"]["parts"]["merge"][p["k"]]) for p in pics])
    out, sizes = np.zeros(n * (w * h * 4 + 4096), np.uint8), np.zeros((n, hc), np.uint32)
    f = sim.kvz_hostsim_entropy_code_inter_pictures
    f.restype = C.c_long
    f.argtypes = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_void_p]
    total = f(rows.ctypes.data, row_of.ctypes.data, pocs.ctypes.data, w, h, n, 0, cu.ctypes.data, ref_cu.ctypes.data, coeff.ctypes.data, recs.ctypes.data, merge.ctypes.data, 49152,
              out.ctypes.data, sizes.ctypes.data)
    assert total >= 0
    return out[:total], sizes


def assert_slice_data(pics, data, sizes):
    """the slice data of every picture of the launch is that of its own sequence's bitstream (oracle_encode_bits)"""
    at = 0
    for i, p in enumerate(pics):
        want, want_sizes = p["seq"]["bits"][p["k"]]
        assert [int(v) for v in sizes[i]] == want_sizes, (i, p["qp"], p["poc"])
        assert bytes(data[at:at + len(want)]) == want, (i, p["qp"], p["poc"])
        at += len(want)
    assert at == len(data)
