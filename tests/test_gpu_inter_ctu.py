"""kvz_hip_dev_inter_ctu_pass -- the CTU pass of B pictures on the MI355X (kvazaar_amd/csrc/kvz_inter_ctu.hpp) -- against the sequence oracle
(oracle/kvz_oracle_inter.inc, equal to the reference encoder CU for CU: tests/test_inter_oracle.py): every B picture of a clip is searched on the device from the
oracle's reference picture and reference CU info, and the device's reconstruction and every CU decision must equal the oracle's picture for picture; then the
device chains its own pictures (its reconstruction deblocked on the device becomes the next picture's reference).  The host simulation of the same sources
(tests/hostsim, CPU) is checked the same way without a GPU."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import ctu_common as cc
import flatapi
import inter_common as ic


from kvazaar_amd.inter import InterParams  # noqa: E402  (kvz_hip_inter_params; sets struct_size)


FAST_COST_CASES = ["pan", "ultrafast", "vertical-pan-owf", "static-qp17", "no-loop-filters", "survey-416x240"]  # every picture QP below 28: kvz_fast_coeff_cost
CABAC_COST_CASES = ["noisy-qp27", "cabac-coeff-cost-qp32", "fast-pan-owf-qp37", "ultrafast-fast-pan-owf-qp30"]     # picture QPs from 28 on: the residual coder in counting mode
EDGE_CASES = ["ultrafast-8mod16", "superfast-8mod16-qp33"]  # 8x8 inter CUs where the picture edge forces the split below pu-depth-inter's 16x16 (search.c:702-713)
FASTER_CASES = ["faster-pan", "faster-qp32", "faster-owf-qp27"]  # `--preset faster`: quarter-sample steps in the fractional search, CABAC coefficient cost at every QP
END_CASES = ic.QP_END_CASES + ic.SMALL_AND_HARD_CASES  # --qp 0 / 51 / `faster` at 49, a 40x24 picture, per-sample 0 / 255 content
MC_EDGE_CASES = ["mc-overflow", "ultrafast-mc-overflow"]  # motion compensation where the 14-bit sample leaves int16 (inter_common.mc_overflow_clip)


@pytest.fixture(scope="module")
def oracle():
    return flatapi.load_oracle()


def params_of(case, qp, poc):
    name, w, h, n, base_qp, preset, dbk, sao, owf, src = case
    p = ic.PRESETS[preset]
    return InterParams(qp=int(qp), poc=poc, mv_constraint=int(owf > 0), sao=int(sao), deblock=int(dbk), fme_level=p["fme_level"], pu_depth_inter_max=p["pu_depth_inter_max"], no_wpp=0, fast_residual_cost=p["fast_residual_cost"])


@pytest.fixture(scope="module")
def hostsim_lib():
    d = os.path.join(flatapi.ROOT, "tests", "hostsim")
    so = os.path.join(d, "libkvz_hostsim.so")
    srcs = [os.path.join(d, "hostsim.cpp")] + [os.path.join(flatapi.ROOT, "kvazaar_amd", "csrc", f) for f in os.listdir(os.path.join(flatapi.ROOT, "kvazaar_amd", "csrc"))]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, os.path.join(d, "hostsim.cpp")])
    return C.CDLL(so)


@pytest.mark.parametrize("name", ["pan", "ultrafast", "vertical-pan-owf", "no-loop-filters", "noisy-qp27", "cabac-coeff-cost-qp32", "fast-pan-owf-qp37", "ultrafast-fast-pan-owf-qp30",
                                  "faster-pan", "faster-qp32", "faster-owf-qp27", "ultrafast-8mod16", "superfast-8mod16-qp33"] + MC_EDGE_CASES + END_CASES)
def test_host_simulation_of_the_device_program_equals_the_oracle(oracle, hostsim_lib, name):
    case = [c for c in ic.CASES if c[0] == name][0]
    _, w, h, n, qp, preset, dbk, sao, owf, src = case
    frames = ic.case_frames(case)
    rs, rf, cu, qps = ic.oracle_encode(oracle, w, h, frames, qp, preset=preset, deblock=bool(dbk), sao=bool(sao), mv_constraint=owf > 0)
    assert_covers_the_overflow(name, rf, cu, w, h)
    mc = cc.model_constants()
    fb = np.array(mc["entropy_fbits"], np.float32)
    f = hostsim_lib.kvz_hostsim_inter_frame
    f.restype = None
    f.argtypes = [C.c_int] * 4 + [C.c_uint64, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 5
    p = ic.PRESETS[preset]
    hostsim_lib.kvz_hostsim_mul24_reset()
    for k in range(1, n):
        rec = np.zeros(w * h * 3 // 2, np.uint8)
        out = np.zeros((h // 4, w // 4), ic.CU_DTYPE)
        f(w, h, int(qps[k]), k, int(mc["coeff_weights"][str(int(qps[k]))]), fb.ctypes.data, int(owf > 0), int(sao), int(dbk), p["fme_level"], p["pu_depth_inter_max"], 0, p["fast_residual_cost"],
          np.ascontiguousarray(frames[k]).ctypes.data, np.ascontiguousarray(rf[k - 1]).ctypes.data, np.ascontiguousarray(cu[k - 1]).ctypes.data, rec.ctypes.data, out.ctypes.data)
        assert ic.first_difference(out[None], cu[k][None]) is None, k
        assert np.array_equal(rec, rs[k]), k
    assert mul24_violations(hostsim_lib) == 0  # every operand of the pass's 24-bit multiplies fitted: the device's v_mul_i32_i24 / v_mul_u32_u24 compute the same


def mul24_violations(sim):
    sim.kvz_hostsim_mul24_violations.restype = C.c_ulonglong
    return int(sim.kvz_hostsim_mul24_violations())


@pytest.mark.parametrize("name", ["survey-1080p", "baseline-c4-2160p"])
def test_host_simulation_at_the_benchmarked_sizes_keeps_the_24_bit_multiplies_in_range(oracle, hostsim_lib, name):
    """the first B picture of the two large sequences through the simulated device program: the operands that grow with the picture (rows x stride, cell index x record
    size, the div_by products) at the sizes the project benchmarks -- equal to the oracle, and no operand beyond 24 bits"""
    case = [c for c in ic.CASES if c[0] == name][0]
    _, w, h, n, qp, preset, dbk, sao, owf, src = case
    frames = ic.case_frames(case)[:2]
    rs, rf, cu, qps = ic.oracle_encode(oracle, w, h, frames, qp, preset=preset, deblock=bool(dbk), sao=bool(sao), mv_constraint=owf > 0)
    mc = cc.model_constants()
    fb = np.array(mc["entropy_fbits"], np.float32)
    f = hostsim_lib.kvz_hostsim_inter_frame
    f.restype = None
    f.argtypes = [C.c_int] * 4 + [C.c_uint64, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 5
    p = ic.PRESETS[preset]
    hostsim_lib.kvz_hostsim_mul24_reset()
    rec = np.zeros(w * h * 3 // 2, np.uint8)
    out = np.zeros((h // 4, w // 4), ic.CU_DTYPE)
    f(w, h, int(qps[1]), 1, int(mc["coeff_weights"][str(int(qps[1]))]), fb.ctypes.data, int(owf > 0), int(sao), int(dbk), p["fme_level"], p["pu_depth_inter_max"], 0, p["fast_residual_cost"],
      np.ascontiguousarray(frames[1]).ctypes.data, np.ascontiguousarray(rf[0]).ctypes.data, np.ascontiguousarray(cu[0]).ctypes.data, rec.ctypes.data, out.ctypes.data)
    assert ic.first_difference(out[None], cu[1][None]) is None
    assert np.array_equal(rec, rs[1])
    assert mul24_violations(hostsim_lib) == 0


def test_host_simulation_models_the_24_bit_multiplies(hostsim_lib):
    """mul24 / mul24v / umul24 of the host simulation against Python integers: operands cut to 24 bits (sign-extended / masked), the low 32 bits of the product --
    what v_mul_i32_i24 / v_mul_u32_u24 compute -- and every operand that did not fit counted"""
    sim = hostsim_lib
    for g in (sim.kvz_hostsim_mul24, sim.kvz_hostsim_mul24v):
        g.restype, g.argtypes = C.c_int32, [C.c_int32, C.c_int32]
    sim.kvz_hostsim_umul24.restype, sim.kvz_hostsim_umul24.argtypes = C.c_uint32, [C.c_uint32, C.c_uint32]

    def sext(v, bits):
        v &= (1 << bits) - 1
        return v - (1 << bits) if v >> (bits - 1) else v
    edges = [0, 1, -1, 22, 4080, 16320, 65535, -(1 << 23), (1 << 23) - 1, 1 << 23, (1 << 24) - 1, 1 << 24, (1 << 24) + 5, -(1 << 23) - 1, -(1 << 24), (1 << 31) - 1, -(1 << 31)]
    beyond_32_bits = 0
    for a in edges:
        for b in edges:
            sim.kvz_hostsim_mul24_reset()
            exact = sext(a, 24) * sext(b, 24)
            beyond_32_bits += int(not -(1 << 31) <= exact < (1 << 31))
            assert sim.kvz_hostsim_mul24(a, b) == sext(exact, 32), (a, b)
            assert sim.kvz_hostsim_mul24v(a, b) == sext(exact, 32), (a, b)
            assert mul24_violations(sim) == 2 * (int(sext(a, 24) != a) + int(sext(b, 24) != b)), (a, b)
            if a >= 0 and b >= 0:
                sim.kvz_hostsim_mul24_reset()
                assert sim.kvz_hostsim_umul24(a, b) == ((a & 0xffffff) * (b & 0xffffff)) & 0xffffffff, (a, b)
                assert mul24_violations(sim) == int(a >> 24 != 0) + int(b >> 24 != 0), (a, b)
    assert beyond_32_bits > 10
    # where the operands fit and the product does, the model is the plain multiply
    sim.kvz_hostsim_mul24_reset()
    assert sim.kvz_hostsim_mul24(2159, 3840) == 2159 * 3840 and sim.kvz_hostsim_mul24(-3, 16320) == -3 * 16320 and sim.kvz_hostsim_umul24(1000, (1 << 20) // 3 + 1) == 1000 * ((1 << 20) // 3 + 1)
    assert sim.kvz_hostsim_umul24((1 << 24) - 1, (1 << 20) + 1) == (((1 << 24) - 1) * ((1 << 20) + 1)) & 0xffffffff  # a product beyond 2^32: its low half
    assert mul24_violations(sim) == 0


def test_inter_pass_geometry_check_at_its_borders(hostsim_lib):
    """inter_pass_geometry_refused (kvz_inter_host.hpp), the check kvz_hip_dev_inter_ctu_pass[_tiles] makes before it launches anything: InterCtu::cell_at and cand_fetch
    multiply a cell index by the record size with the signed 24-bit multiply, so a picture or a reference frame of 2^23 or more 4x4 cells is refused, and a reference frame
    may be no larger than a picture may be (255 CTUs a side)"""
    g = hostsim_lib.kvz_hostsim_inter_geometry_refused
    g.restype, g.argtypes = C.c_int, [C.c_int] * 7
    assert (16320 // 4) * (8256 // 4) >= 1 << 23 > (16320 // 4) * (8192 // 4)
    for (w, h) in ((16320, 8192), (8192, 16320), (8192, 4320), (3840, 2160), (8, 8), (11584, 11576)):
        assert g(w, h, 1, 0, 0, 0, 0) == 0, (w, h)
        assert g(8, 8, 1, w, h, w - 8, h - 8) == 0, (w, h)  # ... and as the reference frame of a tile in its far corner
    for (w, h) in ((16320, 8256), (8256, 16320), (16320, 16320), (11592, 11592), (16328, 64), (64, 16328), (0, 64), (64, -8), (68, 64), (64, 60)):
        assert g(w, h, 1, 0, 0, 0, 0) != 0, (w, h)
    for (rw, rh) in ((16320, 8256), (16328, 64), (16384, 4096), (64, 16328), (100, 64), (1 << 30, 64), (-64, 64), (128, 0)):
        assert g(64, 64, 1, rw, rh, 0, 0) != 0, (rw, rh)
    for (tx, ty) in ((128, 0), (4, 0), (0, 8), (-8, 0)):  # a tile that leaves its 128x64 frame, or off the 8-sample grid
        assert g(64, 64, 1, 128, 64, tx, ty) != 0, (tx, ty)
    assert g(64, 64, 65535, 0, 0, 0, 0) == 0 and g(64, 64, 65536, 0, 0, 0, 0) != 0


def assert_covers_the_overflow(name, rf, cu, w, h):
    """an MC_OVERFLOW case must keep putting one-list (2, 2) PUs on windows whose 14-bit sample leaves int16, or it no longer tests that edge; an
    MC_WHOLE_SAMPLE case must keep to whole-sample luma vectors (and still have inter CUs)"""
    if name in ic.MC_OVERFLOW_CASES:
        n22, over = ic.overflowing_uni_pus(rf, cu, w, h)
        assert over >= 8, (n22, over)
    if name in ic.MC_WHOLE_SAMPLE_CASES:
        b = cu[1:]
        inter = b["type"] == 2
        frac = [inter & ((b["mv_dir"] >> l) & 1 > 0) & ((b["mv"][..., l, :] & 3) != 0).any(axis=-1) for l in range(2)]
        assert inter.sum() > 0 and not (frac[0] | frac[1]).any()


def test_host_simulation_of_the_pass_prediction_at_the_int16_edge(hostsim_lib):
    """the pass's motion-compensated prediction of a CU (InterCtu::inter_predict -> predict_into -> predict_tile) on the luma (2, 2) maximising windows,
    against the model (tests/mc_reference.py): one list (14-bit samples of 33150 finish as 255), two lists (operands wrapped), and two lists with one vector,
    which the pass predicts as one list -- its operands must still wrap, as the reference's bipred average of two equal int16 operands does"""
    import mc_reference as mc
    W, H = 128, 128
    ext = np.ascontiguousarray(mc.extreme_frame(W, H))
    f = hostsim_lib.kvz_hostsim_inter_predict
    f.restype = None
    f.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    twice_wraps = 0
    for w in (8, 16, 32):
        for (x, y, a, b) in [(64, 32, (14, -18), (-22, 6)), (0, 0, (-18, -26), (6, 10)), (W - w, H - w, (2, 2), (10, -6))]:
            for (mv_dir, mv0, mv1) in [(1, a, (0, 0)), (2, (0, 0), a), (3, a, b), (3, a, a)]:
                rec = np.zeros(1, ic.CU_DTYPE)
                rec["type"], rec["mv_dir"], rec["mv"][0, 0], rec["mv"][0, 1] = 2, mv_dir, mv0, mv1
                out = np.zeros(w * w * 3 // 2, np.uint8)
                f(W, H, ext.ctypes.data, rec.ctypes.data, x, y, w, out.ctypes.data)
                pred = mc.inter_pred([ext, ext], W, H, [(x, y, w, w, mv0, mv1, mv_dir & 1, mv_dir >> 1)])
                want = np.concatenate([p[(y >> (c > 0)):(y + w) >> (c > 0), (x >> (c > 0)):(x + w) >> (c > 0)].reshape(-1) for c, (p, _) in enumerate(mc.planes_of(pred, W, H))])
                assert np.array_equal(out, want), (w, x, y, mv_dir, mv0, mv1, int((out != want).sum()))
                if mv_dir == 3 and mv0 == mv1:
                    v = mc.filter14(ext[:W * H].reshape(H, W), x, y, w, w, mv0, False)
                    twice_wraps += int((mc.uni(v) != mc.bi(mc.hi(v), mc.hi(v))).sum())
    assert twice_wraps > 50   # the equal-vector PUs sit on windows where one list and two wrapped operands differ


def test_fuzz_of_the_device_program_against_the_oracle(hostsim_lib):
    """tools/fuzz_inter.py on the rounds of inter_common.draw_fuzz_case: pictures from 8x8 to 264x264 in steps of 8, --qp 0..51, ultrafast / superfast / veryfast / faster,
    GOPs of 2 / 3 / 4 / 8, loop filters / motion restriction / WPP on and off, the textured clip and binary / block / noise / flat / full-range content -- the simulated
    device program must equal the oracle on every B picture, its coder must write the oracle's slice data, and no 24-bit multiply may meet an operand that does not fit
    (the tool exits non-zero on that count)"""
    import sys
    r = subprocess.run([sys.executable, os.path.join(flatapi.ROOT, "tools", "fuzz_inter.py"), "200", "9"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "0 of 200 rounds differ" in r.stdout
    assert "\n0 operands of 24-bit multiplies did not fit\n" in r.stdout


def device_pass(lib, dev, w, h, srcs, refs, ref_cus, prm):
    n = len(srcs)
    lib.kvz_hip_dev_inter_ctu_pass.restype = C.c_int
    lib.kvz_hip_dev_inter_ctu_pass.argtypes = [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_void_p]
    fs, cells = w * h * 3 // 2, (w // 4) * (h // 4)
    d_src, d_ref, d_rcu = dev.put(np.concatenate(srcs)), dev.put(np.concatenate(refs)), dev.put(np.concatenate([c.reshape(-1) for c in ref_cus]))
    d_rec, d_cu = dev.empty(n * fs), dev.empty(n * cells * ic.CU_DTYPE.itemsize)
    rc = lib.kvz_hip_dev_inter_ctu_pass(d_src, d_ref, d_rcu, d_rec, d_cu, None, w, h, n, C.addressof(prm))
    assert rc == 0, rc
    rec = dev.get(d_rec, (n, fs), np.uint8)
    cu = dev.get(d_cu, (n, h // 4, w // 4), ic.CU_DTYPE)
    dev.free(d_src, d_ref, d_rcu, d_rec, d_cu)
    return rec, cu


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAST_COST_CASES + CABAC_COST_CASES + FASTER_CASES + EDGE_CASES + ["two-gops"] + MC_EDGE_CASES + END_CASES)
def test_device_pass_equals_oracle_picture_by_picture(oracle, name):
    import kvazaar_amd
    from kvazaar_amd.dev import Dev
    lib = kvazaar_amd.load_library()
    dev = Dev(lib)
    case = [c for c in ic.CASES if c[0] == name][0]
    _, w, h, n, qp, preset, dbk, sao, owf, src = case
    frames = ic.case_frames(case)
    rs, rf, cu, qps = ic.oracle_encode(oracle, w, h, frames, qp, preset=preset, deblock=bool(dbk), sao=bool(sao), mv_constraint=owf > 0)
    assert_covers_the_overflow(name, rf, cu, w, h)
    for k in range(1, n):
        rec, got = device_pass(lib, dev, w, h, [frames[k]], [rf[k - 1]], [cu[k - 1]], params_of(case, qps[k], k))
        d = ic.first_difference(got, cu[k][None])
        assert d is None, (k, {a: (b if a not in ("ours", "ref") else b.tolist()) for a, b in d.items()})
        assert np.array_equal(rec[0], rs[k]), k


@pytest.mark.gpu
def test_device_pass_on_baseline_config_4(oracle):
    """3840x2160 `--preset veryfast --gop lp-g4d3t1 -q 22`, SURVEY's own clip: the three B pictures, each from the oracle's reference"""
    import kvazaar_amd
    from kvazaar_amd.dev import Dev
    lib = kvazaar_amd.load_library()
    dev = Dev(lib)
    case = [c for c in ic.CASES if c[0] == "baseline-c4-2160p"][0]
    _, w, h, n, qp, preset, dbk, sao, owf, src = case
    frames = ic.case_frames(case)
    rs, rf, cu, qps = ic.oracle_encode(oracle, w, h, frames, qp, preset=preset, deblock=bool(dbk), sao=bool(sao), mv_constraint=owf > 0)
    assert ic.digests(rf, cu)["cu"] == json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inter_recon.json")))["baseline-c4-2160p"]["cu"]
    for k in range(1, n):
        rec, got = device_pass(lib, dev, w, h, [frames[k]], [rf[k - 1]], [cu[k - 1]], params_of(case, qps[k], k))
        assert ic.first_difference(got, cu[k][None]) is None, k
        assert np.array_equal(rec[0], rs[k]), k


CHAIN_CASES = ["deblock-only", "ultrafast", "pan", "vertical-pan-owf", "static-qp17", "no-loop-filters", "survey-416x240", "survey-1080p", "baseline-c4-2160p",
               "noisy-qp27", "cabac-coeff-cost-qp32", "ultrafast-fast-pan-owf-qp30", "faster-pan", "faster-qp32"] + END_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("name", CHAIN_CASES)
def test_device_chains_its_own_pictures(oracle, name):
    """A whole sequence on the device from the I picture's search result on: its loop filters, then every B picture from the device's own previous picture -- CTU pass ->
    kvz_hip_dev_cu_dbk_from_info -> kvz_hip_dev_loop_filters_inter (deblocking with motion-based strengths, the SAO decision on the partly deblocked picture, SAO) -> reference
    of the next picture.  Every picture before and after its loop filters, every CU decision and every SAO decision must equal the oracle's (= the reference encoder's), up to
    BASELINE config 4's own 3840x2160 sequence."""
    import kvazaar_amd
    from kvazaar_amd.dev import Dev
    lib = kvazaar_amd.load_library()
    dev = Dev(lib)
    case = [c for c in ic.CASES if c[0] == name][0]
    _, w, h, n, qp, preset, dbk, sao, owf, src = case
    frames = ic.case_frames(case)
    rs, rf, cu, qps = ic.oracle_encode(oracle, w, h, frames, qp, preset=preset, deblock=bool(dbk), sao=bool(sao), mv_constraint=owf > 0)
    lib.kvz_hip_dev_inter_ctu_pass.restype = C.c_int
    lib.kvz_hip_dev_inter_ctu_pass.argtypes = [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_void_p]
    lib.kvz_hip_dev_cu_dbk_from_info.restype = None
    lib.kvz_hip_dev_cu_dbk_from_info.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.kvz_hip_dev_loop_filters_inter.restype = C.c_int
    lib.kvz_hip_dev_loop_filters_inter.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 3
    fs, cells = w * h * 3 // 2, (w // 4) * (h // 4)
    d_rec, d_cu, d_dbk = dev.empty(fs), dev.empty(cells * ic.CU_DTYPE.itemsize), dev.empty(cells * 20)
    d_ref, d_rcu = dev.empty(fs), dev.empty(cells * ic.CU_DTYPE.itemsize)

    def loop_filters(k, d_src):
        lib.kvz_hip_dev_cu_dbk_from_info(d_cu, cells, d_dbk)
        assert lib.kvz_hip_dev_loop_filters_inter(d_src, d_rec, w, h, 1, d_dbk, int(qps[k]), int(k > 0), int(dbk), 0, 0, int(sao), 0, None, None, None) == 0
        assert np.array_equal(dev.get(d_rec, (fs,), np.uint8), rf[k]), k

    # the I picture: the oracle's search result (the all-intra pass has its own tests), filtered here
    d_src = dev.put(frames[0])
    dev.copy_in(d_rec, rs[0]); dev.copy_in(d_cu, cu[0].reshape(-1))
    loop_filters(0, d_src)
    dev.free(d_src)
    for k in range(1, n):
        d_ref, d_rec = d_rec, d_ref      # the filtered picture is the next reference
        d_rcu, d_cu = d_cu, d_rcu
        d_src = dev.put(frames[k])
        prm = params_of(case, qps[k], k)
        assert lib.kvz_hip_dev_inter_ctu_pass(d_src, d_ref, d_rcu, d_rec, d_cu, None, w, h, 1, C.addressof(prm)) == 0
        assert np.array_equal(dev.get(d_rec, (fs,), np.uint8), rs[k]), k
        assert ic.first_difference(dev.get(d_cu, (1, h // 4, w // 4), ic.CU_DTYPE), cu[k][None]) is None, k
        loop_filters(k, d_src)
        dev.free(d_src)
    dev.free(d_ref, d_rcu, d_rec, d_cu, d_dbk)


@pytest.mark.gpu
def test_device_pass_on_several_sequences_at_once(oracle):
    """picture k of three independent sequences in one launch (the ticket list interleaves their CTUs) == each of them alone"""
    import kvazaar_amd
    from kvazaar_amd.dev import Dev
    lib = kvazaar_amd.load_library()
    dev = Dev(lib)
    w, h, n, qp = 264, 200, 3, 22
    seqs = []
    for seed in (31, 32, 33):
        frames = ic.clip(w, h, n, seed, 1.5, (1.0 + seed % 3, -0.75))
        seqs.append((frames,) + ic.oracle_encode(oracle, w, h, frames, qp, preset="veryfast", deblock=True, sao=True, mv_constraint=True))
    case = ("x", w, h, n, qp, "veryfast", 1, 1, 2, None)
    for k in range(1, n):
        rec, got = device_pass(lib, dev, w, h, [s[0][k] for s in seqs], [s[2][k - 1] for s in seqs], [s[3][k - 1] for s in seqs], params_of(case, seqs[0][4][k], k))
        for i, s in enumerate(seqs):
            assert ic.first_difference(got[i][None], s[3][k][None]) is None, (k, i)
            assert np.array_equal(rec[i], s[1][k]), (k, i)


@pytest.mark.gpu
def test_device_pass_rejects_what_it_does_not_cover():
    import kvazaar_amd
    lib = kvazaar_amd.load_library()
    lib.kvz_hip_dev_inter_ctu_pass.restype = C.c_int
    lib.kvz_hip_dev_inter_ctu_pass.argtypes = [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_void_p]
    ok = InterParams(qp=25, poc=1, mv_constraint=0, sao=1, deblock=1, fme_level=2, pu_depth_inter_max=3, no_wpp=0, fast_residual_cost=28)
    for bad in (dict(qp=52), dict(qp=-1), dict(fme_level=5), dict(fast_residual_cost=52), dict(poc=0), dict(pu_depth_inter_max=4)):
        p = InterParams(**{**{n: getattr(ok, n) for n, _ in InterParams._fields_}, **bad})
        assert lib.kvz_hip_dev_inter_ctu_pass(None, None, None, None, None, None, 64, 64, 1, C.addressof(p)) == -1
    # 2^23 or more 4x4 cells in the picture or in the reference frame, a reference frame beyond 255 CTUs a side: refused before anything is launched
    # (inter_pass_geometry_refused; test_inter_pass_geometry_check_at_its_borders walks the borders on the CPU)
    assert lib.kvz_hip_dev_inter_ctu_pass(None, None, None, None, None, None, 16320, 8256, 1, C.addressof(ok)) == -1
    for bad in (dict(ref_width=16320, ref_height=8256), dict(ref_width=16384, ref_height=64)):
        p = InterParams(**{**{n: getattr(ok, n) for n, _ in InterParams._fields_}, **bad})
        assert lib.kvz_hip_dev_inter_ctu_pass(None, None, None, None, None, None, 64, 64, 1, C.addressof(p)) == -1


@pytest.mark.gpu
@pytest.mark.parametrize("clip", ["tiles2x1-pan", "tiles2x2-fast-pan-qp27"])
def test_device_tile_pass_in_the_tiled_chain(clip):
    """kvazaar --tiles CxR --preset veryfast --gop lp-g4d3t1: the DEVICE's inter CTU pass with the tile geometry of kvz_hip_inter_params (the pictures are tiles, the reference
    a whole frame: motion vectors and the co-located starting point reach into the other tiles; no TMVP) inside the chain of tests/tile_common.py -- every tile's
    reconstruction and CU records equal the device sources in host simulation, and the assembled pictures / CU decisions of the sequence equal the REFERENCE ENCODER's
    (tests/golden/inter_tiles.json).  Several copies of the tile per launch, so that workgroups of different sequences interleave."""
    import kvazaar_amd
    from kvazaar_amd.dev import Dev
    import golden.make_golden as mg
    import tile_common as tc
    lib = kvazaar_amd.load_library()
    dev = Dev(lib)
    sim = tc.load_hostsim()
    host = tc.hostsim_tile_pass(sim)
    copies = 3

    def device_tile_pass(tw, th, pq, k, src, ref_frame, ref_cu, w, h, tx, ty):
        prm = InterParams(qp=int(pq), poc=k, mv_constraint=0, sao=1, deblock=1, fme_level=2, pu_depth_inter_max=3, no_wpp=1, fast_residual_cost=28,
                          ref_width=w, ref_height=h, tile_x=tx, tile_y=ty, no_tmvp=1)
        rec, cu = device_pass(lib, dev, tw, th, [src] * copies, [ref_frame] * copies, [ref_cu] * copies, prm)
        want_rec, want_cu = host(tw, th, pq, k, src, ref_frame, ref_cu, w, h, tx, ty)
        for i in range(copies):
            assert ic.first_difference(cu[i][None], want_cu[None]) is None, (k, tx, ty, i)
            assert np.array_equal(rec[i], want_rec), (k, tx, ty, i)
        return rec[0], cu[0]

    spec = [c for c in mg.INTER_TILE_CLIPS if c[0] == clip][0]
    sim.kvz_hostsim_mul24_reset()
    pictures, records = tc.tiled_inter_chain(spec, 0, 1, None, device_tile_pass, sim)
    assert mul24_violations(sim) == 0
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inter_tiles.json")))[clip]
    got = ic.digests(pictures, records)
    assert got["rec"] == want["rec"] and got["cu"] == want["cu"]


@pytest.mark.gpu
def test_device_pass_refuses_a_tile_outside_its_frame():
    import kvazaar_amd
    from kvazaar_amd.dev import Dev
    lib = kvazaar_amd.load_library()
    dev = Dev(lib)
    lib.kvz_hip_dev_inter_ctu_pass.restype = C.c_int
    lib.kvz_hip_dev_inter_ctu_pass.argtypes = [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_void_p]
    d = dev.empty(64 * 64 * 3)
    for bad in (dict(ref_width=128, ref_height=64, tile_x=128, tile_y=0), dict(ref_width=128, ref_height=64, tile_x=4, tile_y=0), dict(ref_width=100, ref_height=64, tile_x=0, tile_y=0)):
        prm = InterParams(qp=22, poc=1, mv_constraint=0, sao=1, deblock=1, fme_level=2, pu_depth_inter_max=3, no_wpp=1, fast_residual_cost=28, no_tmvp=1, **bad)
        assert lib.kvz_hip_dev_inter_ctu_pass(d, d, d, d, d, None, 64, 64, 1, C.addressof(prm)) == -1
    dev.free(d)
