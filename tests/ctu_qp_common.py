"""Helpers of the tests of a cost model per CTU (kvz_hip_ctu_models, HEVC's cu_qp_delta with one quantisation group per CTU; kvazaar's --roi): the clips of
tests/golden/ctu_qp.json, the host simulation (tests/hostsim/hostsim_ctu_qp.cpp) and its ctypes calls, the rule of the CU QPs as ten lines of plain Python and the
deblocking filter with a QP per edge stated over tests/deblock_reference.py.  Used by tests/test_ctu_qp_sim.py, tests/test_gpu_ctu_qp.py and
tests/golden/make_ctu_qp_golden.py."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np

import ctu_common as cc
import deblock_reference as dr
import flatapi

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "ctu_qp.json")

# A clip: name -> (width, height, seed, slice QP, preset, no_wpp, layouts, deltas).  Two pictures each.  layouts: per picture one letter per CTU, rows separated by
# "/": T textured, F flat (no coefficient at all where its left, above and above-right neighbours are flat too: the flat CTUs start at the picture's corner), H the
# top-left 32x32 flat and the rest textured (where that predicts well, the first CU with a coded block flag is not the CTU's first).
# deltas: per picture the --roi map, CTU QP - slice QP, on the CTU grid.  What each clip is there for:
CLIPS = {
    # one CTU: a chain of length 1
    "one-ctu": (64, 64, 1, 27, "ultrafast", 0, ["T", "H"], [[3], [-2]]),
    # 3x3 CTUs with a partial last row; CTU QPs 20 .. 35 around the limit 28 of the two coefficient pricings; flat CTUs whose successors differ
    "3x3": (192, 136, 2, 27, "ultrafast", 0, ["FFT/FTT/TTH", "FFH/TTT/THT"], [[-6, 0, 5, 3, -3, 0, 8, -7, 1], [2, -2, 4, -4, 6, 0, 0, -1, -7]]),
    # ... the same as one substream per picture: the predictor runs through the rows
    "3x3-nowpp": (192, 136, 2, 27, "ultrafast", 1, ["FFT/FTT/TTH", "FFH/TTT/THT"], [[-6, 0, 5, 3, -3, 0, 8, -7, 1], [2, -2, 4, -4, 6, 0, 0, -1, -7]]),
    # partial last column and last row, 32x32 CUs searched
    "fast-5x2": (264, 72, 3, 30, "fast", 0, ["THFTT/FTTHT", "HTTFT/TFHTT"], [[1, -1, 4, -4, 2, 0, -2, 3, -3, 5], [-5, 0, 0, 2, -1, 4, 1, -2, 0, 3]]),
    # the low end: CTU QPs down to 0
    "low": (128, 64, 4, 3, "ultrafast", 0, ["TT", "HT"], [[-3, 0], [-1, -2]]),
    # the high end: CTU QPs up to 51
    "high": (128, 64, 5, 48, "ultrafast", 0, ["TT", "HT"], [[3, 0], [1, 2]]),
    # the widest deltas the syntax has: +25 and -25 between neighbours
    "span25": (192, 64, 6, 20, "ultrafast", 0, ["TTT", "HTT"], [[0, 25, 0], [25, 0, 25]]),
}
ZERO_MAP = "3x3"  # the clip whose slice data with an all-zero map is pinned too


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def fixture():
    return json.load(open(FIXTURE))


def grid(clip):
    w, h = CLIPS[clip][:2]
    return (w + 63) // 64, (h + 63) // 64


def clip_frames(clip):
    """the clip's pictures, Y | U | V each: textured CTUs beside flat ones as its layouts say"""
    w, h, seed, _, _, _, layouts, _ = CLIPS[clip]
    rng = np.random.default_rng(seed)
    out = []
    for i, layout in enumerate(layouts):
        yy, xx = np.mgrid[0:h, 0:w]
        y = (128 + 60 * np.sin(xx / 7.0 + i) + 40 * np.cos(yy / 5.0) + rng.integers(-25, 25, (h, w))).clip(0, 255).astype(np.uint8)
        u, v = rng.integers(100, 156, (h // 2, w // 2)).astype(np.uint8), rng.integers(100, 156, (h // 2, w // 2)).astype(np.uint8)
        for cy, row in enumerate(layout.split("/")):
            for cx, kind in enumerate(row):
                size = {"T": 0, "F": 64, "H": 32}[kind]
                y[cy * 64:cy * 64 + size, cx * 64:cx * 64 + size] = 128
                u[cy * 32:cy * 32 + size // 2, cx * 32:cx * 32 + size // 2] = 128
                v[cy * 32:cy * 32 + size // 2, cx * 32:cx * 32 + size // 2] = 128
        out.append(np.concatenate([y.ravel(), u.ravel(), v.ravel()]))
    return out


def switches(clip):
    """the cost-model switches of the clip's preset (tests/test_encoder_parity.py: `fast` = 32x32 CUs searched + the CABAC coefficient cost at every QP)"""
    s = {}
    if CLIPS[clip][4] == "fast":
        s.update(search_32x32=1, coeff_cabac=1)
    if CLIPS[clip][5]:
        s["no_wpp"] = 1
    return s


def weights(qp):
    return cc.coeff_weights(qp) if qp < 50 else 0


def ctu_qps(clip, zero=False):
    qp, deltas = CLIPS[clip][3], CLIPS[clip][7]
    return [[qp + (0 if zero else d) for d in pic] for pic in deltas]


def models(lib, clip, zero=False):
    """the clip's CtuModels (zero: the all-zero map -- every CTU at the slice QP)"""
    from kvazaar_amd.batch import CtuModels
    return CtuModels(lib, [CLIPS[clip][3]] * 2, ctu_qps(clip, zero), weights=weights, **switches(clip))


def roi_file(path, clip, zero=False):
    """the clip's map as kvazaar's --roi reads it: per picture "width height" and the deltas, on the CTU grid"""
    wc, hc = grid(clip)
    with open(path, "w") as f:
        for pic in CLIPS[clip][7]:
            f.write(f"{wc} {hc}\n" + " ".join(str(0 if zero else d) for d in pic) + "\n")
    return path


def load_sim():
    """tests/hostsim/libkvz_hostsim_ctu_qp.so, built with the recipe of the other host simulations when it is missing or older than a source"""
    d, csrc = os.path.join(flatapi.ROOT, "tests", "hostsim"), os.path.join(flatapi.ROOT, "kvazaar_amd", "csrc")
    so = os.path.join(d, "libkvz_hostsim_ctu_qp.so")
    srcs = [os.path.join(d, f) for f in ("hostsim_ctu_qp.cpp", "hostsim_models.cpp", "hostsim.cpp")] + [os.path.join(flatapi.ROOT, "include", "kvz_hip_types.h")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = os.path.join(d, f".libkvz_hostsim_ctu_qp.{os.getpid()}.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp, os.path.join(d, "hostsim_ctu_qp.cpp")])
        os.replace(tmp, so)
    return C.CDLL(so)


def qp_outputs(w, h, n=1):
    return dict(cu_qp=np.zeros(n * (w // 8) * (h // 8), np.uint8), ctu_qp=np.zeros(n * ((w + 63) // 64) * ((h + 63) // 64), np.uint32))


def sim_pass(sim, cm, w, h, frames):
    """kvz_hostsim_intra_frames_ctu_models on the batch `frames` -> one output dict per picture, cu_qp / ctu_qp included (None: the map was refused)"""
    n = len(frames)
    one = dict(cc.outputs(w, h), **qp_outputs(w, h))
    big = {k: np.zeros(v.size * n, v.dtype) for k, v in one.items()}
    src = np.concatenate(frames)
    f = sim.kvz_hostsim_intra_frames_ctu_models
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8
    rc = f(C.addressof(cm.struct), w, h, n, src.ctypes.data, *(big[k].ctypes.data for k in ("rec", "coeff", "depth", "mode", "cost", "cu_qp", "ctu_qp")))
    if rc != 0:
        return None
    return [{k: v.reshape(n, -1)[i].copy() for k, v in big.items()} for i in range(n)]


def sim_pass_models(sim, pm, w, h, frames):
    """kvz_hostsim_intra_frames_models (tests/hostsim/hostsim_models.cpp, part of the same library) on the batch `frames`: the launch with a model per picture"""
    n = len(frames)
    big = {k: np.zeros(v.size * n, v.dtype) for k, v in cc.outputs(w, h).items()}
    src = np.concatenate(frames)
    f = sim.kvz_hostsim_intra_frames_models
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8
    assert f(C.addressof(pm.struct), w, h, n, src.ctypes.data, *(big[k].ctypes.data for k in ("rec", "coeff", "depth", "mode", "cost")), None, None) == 0
    return [{k: v.reshape(n, -1)[i].copy() for k, v in big.items()} for i in range(n)]


def sim_cu_qps(sim, w, h, no_wpp, coeff, depth, qp_of_ctu, slice_qps):
    """kvz_hostsim_cu_qps: the three steps of kvz_cu_qp.hpp on levels and depths of n pictures -> (cu_qp [n][...], ctu_qp [n][...])"""
    n = len(slice_qps)
    out = qp_outputs(w, h, n)
    coeff, depth = np.ascontiguousarray(coeff, np.int16), np.ascontiguousarray(depth, np.uint8)
    q, s = np.ascontiguousarray(qp_of_ctu, np.uint8), np.ascontiguousarray(slice_qps, np.int32)
    f = sim.kvz_hostsim_cu_qps
    f.restype = None
    f.argtypes = [C.c_int] * 4 + [C.c_void_p] * 6
    f(w, h, n, int(no_wpp), coeff.ctypes.data, depth.ctypes.data, q.ctypes.data, s.ctypes.data, out["cu_qp"].ctypes.data, out["ctu_qp"].ctypes.data)
    return out["cu_qp"].reshape(n, -1), out["ctu_qp"].reshape(n, -1)


def word(pred, q, coded, first):
    """a CTU's word as kvz_hip_batch_download_cu_qps hands it out"""
    return pred | q << 8 | coded << 16 | first << 24


def census(clip, words):
    """what the clip's CTU words (per picture, kvz_hip_batch_download_cu_qps) exercise: the CTUs without any coefficient whose chain successor has another QP, the CTUs
    whose first CU with a coded block flag is not their first CU, the coded deltas"""
    wc, hc = grid(clip)
    no_wpp = CLIPS[clip][5]
    out = {"uncoded_before_another_qp": 0, "first_coded_cu_not_first": 0, "deltas": []}
    for pic in words:
        w = [(int(v) & 255, int(v) >> 8 & 255, int(v) >> 16 & 1, int(v) >> 24) for v in pic]
        for i, (pred, q, coded, first) in enumerate(w):
            last_of_chain = i == len(w) - 1 if no_wpp else i % wc == wc - 1
            if not coded and not last_of_chain and w[i + 1][1] != q:
                out["uncoded_before_another_qp"] += 1
            if coded and first > 0:
                out["first_coded_cu_not_first"] += 1
            if coded:
                out["deltas"].append(q - pred)
    out["deltas"] = sorted(set(out["deltas"]))
    return out


def census_complete(census_of_clip):
    """the counts the clips must reach together (asserted by the generator and, on the record, by tests/test_ctu_qp_sim.py).  census_of_clip: {clip: census}.  CTUs
    are counted by content: two clips with the same pictures and the same map (a clip and its twin without WPP) count once; their coded deltas differ and all count"""
    deltas = {d for e in census_of_clip.values() for d in e["deltas"]}
    distinct = {(CLIPS[c][:5], str(CLIPS[c][6:])): e for c, e in census_of_clip.items()}.values()
    return (sum(e["uncoded_before_another_qp"] for e in distinct) >= 4 and sum(e["first_coded_cu_not_first"] for e in distinct) >= 4
            and {0, 1, 2, 3, 4, -1, -2, -3, -4, 25, -25} <= deltas and any(d >= 5 for d in deltas) and any(d <= -5 for d in deltas))


# ---- the rule, in plain Python (include/kvz_hip_batch.h; encoderstate.c:574-633 with one quantisation group per CTU)
def coding_order(depth, x8, y8, d, w8, h8):
    """the CUs of the CTU whose first 8x8 unit is (x8, y8), as (x8, y8, size in units) in coding order; depth: the picture's map [h8][w8]"""
    size = 8 >> d
    if x8 >= w8 or y8 >= h8:
        return []
    if depth[y8][x8] > d:
        return [cu for dy in (0, size // 2) for dx in (0, size // 2) for cu in coding_order(depth, x8 + dx, y8 + dy, d + 1, w8, h8)]
    return [(x8, y8, size)]


def cu_qps_rule(w, h, no_wpp, depth, cu_coded, ctu_q, slice_qp):
    """depth [h8][w8]; cu_coded(x8, y8, size) -> does the CU have any coded block flag; ctu_q [hc][wc] -> (cu_qp [h8][w8], {(cx, cy): (pred, coded delta or None)})"""
    w8, h8, wc, hc = w // 8, h // 8, (w + 63) // 64, (h + 63) // 64
    cu_qp, ctus, last = [[0] * w8 for _ in range(h8)], {}, slice_qp
    for cy in range(hc):
        if not no_wpp:
            last = slice_qp  # a substream per CTU row
        for cx in range(wc):
            pred, found = last, False
            for x8, y8, size in coding_order(depth, cx * 8, cy * 8, 0, w8, h8):
                found = found or cu_coded(x8, y8, size)
                for yy in range(y8, min(y8 + size, h8)):
                    cu_qp[yy][x8:x8 + size] = [ctu_q[cy][cx] if found else pred] * len(cu_qp[yy][x8:x8 + size])
            ctus[cx, cy] = (pred, ctu_q[cy][cx] - pred if found else None)
            last = ctu_q[cy][cx] if found else pred
    return cu_qp, ctus


def unit_coded(coeff, wc):
    """coeff: the levels of one picture -> f(x8, y8, size): does the CU carry a level in any plane (the levels of a CU lie in z-order)"""
    ctus = np.asarray(coeff, np.int16).reshape(-1, 6144)

    def z(x, y):
        return sum(((x >> b) & 1) << (2 * b) | ((y >> b) & 1) << (2 * b + 1) for b in range(3))

    def f(x8, y8, size):
        c, i, n = ctus[(y8 // 8) * wc + x8 // 8], z(x8 % 8, y8 % 8), size * size
        return bool(c[i * 64:(i + n) * 64].any() or c[4096 + i * 16:4096 + (i + n) * 16].any() or c[5120 + i * 16:5120 + (i + n) * 16].any())
    return f


def rule_of_outputs(w, h, no_wpp, o, ctu_q, slice_qp):
    """cu_qps_rule on the outputs of a pass"""
    wc = (w + 63) // 64
    depth = o["depth"].reshape(h // 8, w // 8).tolist()
    return cu_qps_rule(w, h, no_wpp, depth, unit_coded(o["coeff"], wc), np.asarray(ctu_q).reshape(-1, wc).tolist(), slice_qp)


# ---- deblocking with a QP per edge (filter.c:275-295), over the plain-Python filter of tests/deblock_reference.py
def deblock_cu_qps(w, h, b_off, t_off, frame, cu_depth, cu_qp, passes=3):
    """deblock_reference.deblock_intra with every 8x8 unit's edge filtered at (QpP + QpQ + 1) >> 1 of the CU QPs on its two sides: that value gives beta and tc and,
    through the chroma QP table, the chroma tc.  passes: 1 the vertical edges, 2 the horizontal edges, 3 both in that order.  -> picture"""
    depth, qp = np.asarray(cu_depth).reshape(h // 8, w // 8).tolist(), np.asarray(cu_qp).reshape(h // 8, w // 8).tolist()
    n, cw = w * h, w // 2
    flat = np.asarray(frame, np.uint8)
    Y, U, V = flat[:n].tolist(), flat[n:n + n // 4].tolist(), flat[n + n // 4:n + n // 2].tolist()
    for vertical in [v for v, bit in ((True, 1), (False, 2)) if passes & bit]:
        across, along = (1, w) if vertical else (w, 1)
        across_c, along_c = (1, cw) if vertical else (cw, 1)
        for ey in range(0, h, 8):
            for ex in range(0, w, 8):
                pos = ex if vertical else ey
                if pos == 0 or pos % (64 >> max(depth[ey >> 3][ex >> 3], 1)):
                    continue
                qp_p = qp[ey >> 3][(ex >> 3) - 1] if vertical else qp[(ey >> 3) - 1][ex >> 3]
                beta, tc, _, tc_c = dr.thresholds((qp_p + qp[ey >> 3][ex >> 3] + 1) >> 1, b_off, t_off)
                for part in range(2):
                    at = (ey + 4 * part) * w + ex if vertical else ey * w + ex + 4 * part
                    new, _, _ = dr.luma_part([[Y[at + i * along + k * across] for k in range(-4, 4)] for i in range(4)], beta, tc)
                    for i in range(4):
                        for k in range(1, 7):
                            Y[at + i * along + (k - 4) * across] = new[i][k]
                xc, yc = ex >> 1, ey >> 1
                if (xc if vertical else yc) & 7:
                    continue
                at = yc * cw + xc
                for plane in (U, V):
                    new, _, _ = dr.chroma_part([[plane[at + i * along_c + (k - 2) * across_c] for k in range(4)] for i in range(4)], tc_c)
                    for i in range(4):
                        plane[at + i * along_c - across_c], plane[at + i * along_c] = new[i][1], new[i][2]
    return np.array(Y + U + V, np.uint8)


# ---- the loop filters of a picture under a map, on the host: (deblocked picture, picture after deblocking + SAO)
def sim_loop_filters(sim, oracle, cm, picture, w, h, src, o):
    """What kvz_hip_batch_loop_filters_ctu_models computes for picture `picture` of the map `cm` from the pass outputs `o`: deblocking at the CU QPs (deblock_cu_qps:
    the picture after the vertical edges and after all edges), the SAO decision of every CTU under its own lambda (kvz_hostsim_sao_decide_ctu) and the SAO
    reconstruction of the decided parameters (the oracle's kvz_oracle_sao_frame, pinned against the reference by tests/test_oracle_vs_ref.py)"""
    from kvazaar_amd.capi import SaoParams
    ctus = ((w + 63) // 64) * ((h + 63) // 64)
    R = np.ascontiguousarray(o["rec"])
    V = deblock_cu_qps(w, h, 0, 0, R, o["depth"], o["cu_qp"], passes=1)
    D = deblock_cu_qps(w, h, 0, 0, V, o["depth"], o["cu_qp"], passes=2)
    rows = [cm.index[picture * ctus + i] for i in range(ctus)]
    lambdas = np.array([cm.pictures.models[r].lambda_ for r in rows], np.float64)
    luma, chroma, merge = (SaoParams * ctus)(), (SaoParams * ctus)(), np.zeros(ctus, np.uint8)
    f = sim.kvz_hostsim_sao_decide_ctu
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7
    src = np.ascontiguousarray(src)
    f(C.addressof(cm.pictures.model_of(picture)), lambdas.ctypes.data, w, h, src.ctypes.data, R.ctypes.data, V.ctypes.data, D.ctypes.data, C.addressof(luma), C.addressof(chroma), merge.ctypes.data)
    out = D.copy()
    g = oracle.lib.kvz_oracle_sao_frame
    g.restype = None
    g(w, h, flatapi.ptr(D), flatapi.ptr(out), luma, chroma)
    return D, out


# ---- the slice data
def reference_slice_payloads(clip, workdir, zero=False):
    """the slice NAL payloads the reference encoder writes for the clip under its --roi map (zero: the all-zero map), SAO off"""
    import entropy_common as ec
    w, h, _, qp, preset, no_wpp = CLIPS[clip][:6]
    yuv, out = os.path.join(workdir, "in.yuv"), os.path.join(workdir, "out.hevc")
    open(yuv, "wb").write(b"".join(f.tobytes() for f in clip_frames(clip)))
    cmd = [os.path.join(flatapi.ROOT, "oracle", "_ref", "kvazaar_ref"), "-i", yuv, "--input-res", f"{w}x{h}", "--preset", preset, "-p", "1", "-q", str(qp), "--threads", "4", "-o", out,
           "--roi", roi_file(os.path.join(workdir, "roi.txt"), clip, zero)] + (["--no-wpp"] if no_wpp else []) + (["--sao", "off"] if preset != "ultrafast" else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-1500:]
    return ec.slice_payloads(open(out, "rb").read())


def sim_entropy(sim, cm, w, h, outs):
    """kvz_hostsim_entropy_code_ctu_models on the pass outputs `outs` (cu_qp words included), SAO off -> [(slice data, substream sizes)] per picture"""
    n, hc = len(outs), (h + 63) // 64
    rows = 1 if cm.no_wpp else hc
    depth, mode, coeff, words = (np.concatenate([o[k] for o in outs]) for k in ("depth", "mode", "coeff", "ctu_qp"))
    f = sim.kvz_hostsim_entropy_code_ctu_models
    f.restype = C.c_long
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    buf, sizes, most = np.zeros(n * (w * h * 4 + 4096), np.uint8), np.zeros((n, rows), np.uint32), C.c_uint32(0)

    def run(cap):
        return f(C.addressof(cm.struct), w, h, n, depth.ctypes.data, mode.ctypes.data, coeff.ctypes.data, words.ctypes.data, None, None, cap, buf.ctypes.data, sizes.ctypes.data, C.byref(most))
    total = run(12288)
    if total == -1:  # a CTU's bin list did not fit: again with the room it needs, as the library does
        total = run(most.value)
    assert total >= 0 and total == int(sizes.sum()), total  # (-2: the counting run and the writing run disagree about a substream's size)
    out, at = [], 0
    for i in range(n):
        size = int(sizes[i].sum())
        out.append((bytes(buf[at:at + size]), [int(v) for v in sizes[i]]))
        at += size
    return out
