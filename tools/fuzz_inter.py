#!/usr/bin/env python3
"""Fuzz of the inter CTU pass's device sources (host simulation, tests/hostsim) against the sequence oracle.  The rounds are drawn by tests/inter_common.py
draw_fuzz_case, the distribution tools/fuzz_inter_oracle.py checks the oracle on against the reference encoder and the device meets in tests/test_gpu_inter_fuzz.py:
picture sizes from 8x8 to 264x264 in steps of 8, --qp 0..51 (picture QPs on both sides of fast-residual-cost and of MAX_FAST_COEFF_COST_QP 50), the four presets of
the low-delay configuration (ultrafast / superfast / veryfast / faster: subme 0 / 2 / 2 / 4, PUs down to 16x16 / 16x16 / 8x8 / 8x8, fast-residual-cost 28 / 28 / 28 / 0)
and overrides of --subme and --fast-residual-cost, low-delay GOPs of 2, 3, 4 and 8 pictures, loop filters and the overlapped-picture motion restriction on or off,
--no-wpp, and six kinds of content (textured clip with moving objects, per-sample 0 / 255, 0 / 255 in 4x4 blocks, uniform noise, flat, full-range smooth texture)
under whole- and sub-sample pans.  Every B picture is searched by the simulated device program from the oracle's reference picture and CU records; reconstruction
and every CU decision must be the oracle's, the device's entropy coder for B pictures must write the oracle coder's slice data from the oracle's records, and no
24-bit multiply of the pass may have met an operand that does not fit (kvz_hostsim_mul24_violations).
usage: tools/fuzz_inter.py [rounds] [seed]"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import flatapi, ctu_common as cc, inter_common as ic, entropy_common as ec

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 12
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
oracle = flatapi.load_oracle()
sim = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libkvz_hostsim.so"))
f = sim.kvz_hostsim_inter_frame
f.restype = None
f.argtypes = [C.c_int] * 4 + [C.c_uint64, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 5
mc = cc.model_constants()
fb = np.array(mc["entropy_fbits"], np.float32)
fe = sim.kvz_hostsim_entropy_code_inter  # the device's entropy coder for B pictures (kvz_entropy.hpp) on the oracle's records, levels and SAO decisions
fe.restype = C.c_long
fe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_void_p]

viol = sim.kvz_hostsim_mul24_violations
viol.restype = C.c_ulonglong
sim.kvz_hostsim_mul24_reset()

bad = 0
for r in range(rounds):
    c = ic.draw_fuzz_case(rng, max_frames=3)
    w, h, n, qp, dbk, sao, no_wpp, owf = c["w"], c["h"], c["n"], c["qp"], c["deblock"], c["sao"], c["no_wpp"], c["owf"]
    frames = ic.fuzz_frames(c)
    kw = ic.fuzz_oracle_kwargs(c)
    rs, rf, cu, qps = ic.oracle_encode(oracle, w, h, frames, qp, **kw)
    p = ic.fuzz_options(c)
    ok = True
    for k in range(1, n):
        rec = np.zeros(w * h * 3 // 2, np.uint8)
        out = np.zeros((h // 4, w // 4), ic.CU_DTYPE)
        f(w, h, int(qps[k]), k, int(mc["coeff_weights"][str(int(qps[k]))]), fb.ctypes.data, owf, sao, dbk, p["fme_level"], p["pu_depth_inter_max"], no_wpp, p["fast_residual_cost"],
          np.ascontiguousarray(frames[k]).ctypes.data, np.ascontiguousarray(rf[k - 1]).ctypes.data, np.ascontiguousarray(cu[k - 1]).ctypes.data, rec.ctypes.data, out.ctypes.data)
        ok = ok and ic.first_difference(out[None], cu[k][None]) is None and np.array_equal(rec, rs[k])
    # the slice data of every B picture: simulated device coder == the oracle's coder
    parts = ic.oracle_encode_parts(oracle, w, h, frames, qp, **kw)
    bits = ic.oracle_encode_bits(oracle, w, h, frames, qp, **kw)
    rows = 1 if no_wpp else (h + 63) // 64
    for k in range(1, n):
        init = ic.b_slice_context_states(oracle, parts["qps"][k])
        recs = merge = None
        if sao:
            recs = ec.pack_sao_records(np.ascontiguousarray(parts["sao_luma"][k]), np.ascontiguousarray(parts["sao_chroma"][k]), parts["ctus"])
            merge = np.ascontiguousarray(parts["merge"][k])
        out, sizes = np.zeros(w * h * 4 + 4096, np.uint8), np.zeros(rows, np.uint32)
        c_k, c_ref, lv = np.ascontiguousarray(parts["cu"][k]), np.ascontiguousarray(parts["cu"][k - 1]), np.ascontiguousarray(parts["coeff"][k])
        total = fe(init.ctypes.data, w, h, k, no_wpp, c_k.ctypes.data, c_ref.ctypes.data, lv.ctypes.data, recs.ctypes.data if recs is not None else None,
                   merge.ctypes.data if merge is not None else None, 49152, out.ctypes.data, sizes.ctypes.data)
        ok = ok and total >= 0 and out[:total].tobytes() == bits[k][0] and [int(v) for v in sizes] == list(bits[k][1])
    b = cu[1:]
    print("round %d: %s (pictures %s): intra %d skipped %d merged %d amvp %d -> %s" % (
        r, ic.describe_fuzz_case(c), list(map(int, qps)), int((b["type"] == 1).sum()), int(((b["type"] == 2) & (b["skipped"] == 1)).sum()),
        int(((b["type"] == 2) & (b["merged"] == 1)).sum()), int(((b["type"] == 2) & (b["merged"] == 0) & (b["skipped"] == 0)).sum()), "equal" if ok else "DIFFERENT"), flush=True)
    bad += not ok
violations = int(viol())
print("%d operands of 24-bit multiplies did not fit" % violations)
print("%d of %d rounds differ" % (bad, rounds))
sys.exit(1 if bad or violations else 0)
