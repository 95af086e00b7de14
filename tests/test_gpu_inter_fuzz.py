"""Randomised device-vs-oracle comparison of the inter path on the MI355X (-m gpu): kvz_hip_dev_inter_ctu_pass[_tiles], kvz_hip_dev_loop_filters_inter and
kvz_hip_dev_entropy_code_inter on the rounds of inter_common.draw_fuzz_case -- pictures from 8x8 to 264x264 in steps of 8, --qp 0..51, the four presets with --subme and
--fast-residual-cost overrides, four low-delay GOPs, every switch on / off, and six kinds of content (the textured clip, per-sample 0 / 255, 0 / 255 in 4x4 blocks, uniform
noise, flat, full-range smooth texture).  The same rounds run on the CPU through tools/fuzz_inter_oracle.py (oracle == reference encoder) and tools/fuzz_inter.py (host
simulation == oracle); but the host simulation executes the DPP reductions as loops and the 24-bit multiplies through a model, so only here do the instructions
themselves see this content.  Everything is bit-exact, no tolerance.

Fixed seed, no round skipped or filtered.  Every round: each B picture through the pass from the oracle's reference picture and CU records.  Every third round also as
the chain pass (with levels) -> loop filters -> entropy coder from the device's own pictures; every fourth with 2..5 different clips of one size in one launch; every
eighth as a tile of its frame (ref_width / ref_height / tile_x / tile_y / no_tmvp) against the device sources in host simulation.

test_seed_set_covers_the_inter_path needs no GPU: it checks on the ORACLE's output alone that the seed set reaches what it is meant to reach.

The lowest B-picture QP.  `--qp 0` gives the I picture QP 0, but a B picture of a low-delay GOP runs at --qp + layer (+ the GOP's QP model), layer >= 1
(kvz_oracle_lowdelay_qp, cfg.c:1455-1463), so the lowest B-picture QP a sequence reaches is 1: the coverage test asserts that one and the I picture at QP 0 (whose loop
filters the chain runs on the device), and test_device_pass_at_picture_qp_0_equals_host_simulation hands the pass QP 0 directly, against the host simulation."""
import ctypes as C
import time

import numpy as np
import pytest

import ctu_common as cc
import inter_common as ic

SEED = 20261064  # the first seed from 20261016 on whose 64 rounds pass test_seed_set_covers_the_inter_path
ROUNDS = 64


def drawn_cases():
    rng = np.random.default_rng(SEED)
    return [ic.draw_fuzz_case(rng, max_frames=3) for _ in range(ROUNDS)]


def role(i):
    """(chain, sequences per launch, tile) of round i"""
    return i % 3 == 0, (2 + (i // 4) % 4) if i % 4 == 1 else 1, i % 8 == 7


def tile_of(c):
    """a tile of the case's frame on the 8-sample grid, drawn from the case's seed"""
    rng = np.random.default_rng(c["seed"] ^ 0x7115)
    tw, th = 8 * int(rng.integers(1, c["w"] // 8 + 1)), 8 * int(rng.integers(1, c["h"] // 8 + 1))
    return 8 * int(rng.integers(0, (c["w"] - tw) // 8 + 1)), 8 * int(rng.integers(0, (c["h"] - th) // 8 + 1)), tw, th


def params_of(c, qp, poc, **tile):
    from kvazaar_amd.inter import InterParams
    p = ic.fuzz_options(c)
    return InterParams(qp=int(qp), poc=poc, mv_constraint=c["owf"], sao=c["sao"], deblock=c["deblock"], fme_level=p["fme_level"], pu_depth_inter_max=p["pu_depth_inter_max"],
                       no_wpp=c["no_wpp"], fast_residual_cost=p["fast_residual_cost"], **tile)


def test_seed_set_covers_the_inter_path(oracle):
    """the drawn rounds, and what the oracle decides on them, reach every family and decision kind the device test is there for"""
    cases = drawn_cases()
    assert {c["kind"] for c in cases} == set(ic.FUZZ_CONTENT)
    assert {c["preset"] for c in cases} == set(ic.PRESETS) and {c["gop"] for c in cases} == set(ic.FUZZ_GOPS)
    for key in ("owf", "sao", "deblock", "no_wpp"):
        assert {c[key] for c in cases} == {0, 1}, key
    assert {ic.fuzz_options(c)["fme_level"] for c in cases} == {0, 1, 2, 3, 4}
    assert {ic.fuzz_options(c)["fast_residual_cost"] for c in cases} == {0, 20, 28, 35, 51}
    assert min(c["qp"] for c in cases) == 0 and max(c["qp"] for c in cases) == 51
    assert sum(c["w"] < 64 or c["h"] < 64 for c in cases) * 4 >= len(cases)
    assert any(c["w"] == 8 for c in cases) and any(c["h"] == 8 for c in cases) and any(c["w"] < 64 and c["h"] < 64 for c in cases)
    assert any(c["w"] > 200 for c in cases) and any(c["h"] > 200 for c in cases)
    assert {role(i)[0] for i in range(ROUNDS)} == {False, True} and {role(i)[1] for i in range(ROUNDS)} == {1, 2, 3, 4, 5} and sum(role(i)[2] for i in range(ROUNDS)) >= 4
    seen = {k: 0 for k in ("intra", "skipped", "merged", "amvp", "bipred", "fractional", "depth1", "depth2", "depth3", "inter_residual", "b_qp_1", "i_qp_0", "b_qp_51",
                           "b_qp_50_frc_51", "b_qp_below_28_fast", "b_qp_from_28_cabac", "small_with_inter")}
    for c in cases:
        rs, rf, cu, qps = ic.oracle_encode(oracle, c["w"], c["h"], ic.fuzz_frames(c), c["qp"], **ic.fuzz_oracle_kwargs(c))
        frc = ic.fuzz_options(c)["fast_residual_cost"]
        b = cu[1:]
        inter = b["type"] == 2
        coded = inter & (b["skipped"] == 0) & (b["merged"] == 0)
        frac = np.zeros(inter.shape, bool)
        for l in range(2):
            frac |= inter & ((b["mv_dir"] >> l) & 1 > 0) & ((b["mv"][..., l, :] & 3) != 0).any(axis=-1)
        seen["intra"] += int((b["type"] == 1).sum())
        seen["skipped"] += int((inter & (b["skipped"] == 1)).sum())
        seen["merged"] += int((inter & (b["merged"] == 1) & (b["skipped"] == 0)).sum())
        seen["amvp"] += int(coded.sum())
        seen["bipred"] += int((inter & (b["mv_dir"] == 3)).sum())
        seen["fractional"] += int(frac.sum())
        for d in (1, 2, 3):  # (no preset of the inter pass keeps a 64x64 CU)
            seen["depth%d" % d] += int((b["depth"] == d).sum())
        seen["inter_residual"] += int((inter & (b["cbf"] != 0)).sum())
        seen["i_qp_0"] += int(qps[0] == 0)
        seen["b_qp_1"] += int((qps[1:] == 1).sum())
        seen["b_qp_51"] += int((qps[1:] == 51).sum())
        seen["b_qp_50_frc_51"] += int((qps[1:] >= 50).sum()) if frc == 51 else 0
        seen["b_qp_below_28_fast"] += int((qps[1:] < min(28, frc)).sum())
        seen["b_qp_from_28_cabac"] += int(((qps[1:] >= 28) & (qps[1:] < 50)).sum())
        seen["small_with_inter"] += int(c["w"] < 64 and c["h"] < 64 and inter.any())
    print("inter fuzz seed set:", seen)
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.gpu
def test_device_inter_path_fuzz_equals_oracle(oracle):
    import kvazaar_amd
    from kvazaar_amd import inter
    from kvazaar_amd.dev import Dev
    import tile_common as tc
    from test_gpu_inter_ctu import device_pass
    lib = kvazaar_amd.load_library()
    dev = Dev(lib)
    sim = tc.load_hostsim()
    sim.kvz_hostsim_mul24_violations.restype = C.c_ulonglong
    sim.kvz_hostsim_mul24_reset()
    mc = cc.model_constants()
    fb = np.array(mc["entropy_fbits"], np.float32)
    bad, counts, t0 = [], {}, time.time()

    def differs(what, i, c, detail):
        bad.append((what, i, ic.describe_fuzz_case(c), detail))
        print("DIFFERENT", bad[-1], flush=True)

    for i, c in enumerate(drawn_cases()):
        chain, n_seq, tile = role(i)
        w, h, n = c["w"], c["h"], c["n"]
        kw = ic.fuzz_oracle_kwargs(c)
        seqs = []
        for j in range(n_seq):  # sequence 0 is the drawn one, the others the same family from other seeds
            frames = ic.fuzz_frames(c, c["seed"] + 7919 * j)
            seqs.append((frames,) + ic.oracle_encode(oracle, w, h, frames, c["qp"], **kw))
        qps = seqs[0][4]
        for key in (c["kind"], "chain" * chain, "several" * (n_seq > 1), "tile" * tile, "below-64" * (w < 64 or h < 64), "qp<=5" * (c["qp"] <= 5), "qp>=46" * (c["qp"] >= 46)):
            counts[key] = counts.get(key, 0) + 1
        # the pass, picture by picture, from the oracle's reference picture and CU records (a non-zero return code ends the test in device_pass)
        for k in range(1, n):
            rec, got = device_pass(lib, dev, w, h, [s[0][k] for s in seqs], [s[2][k - 1] for s in seqs], [s[3][k - 1] for s in seqs], params_of(c, qps[k], k))
            for j, s in enumerate(seqs):
                d = ic.first_difference(got[j][None], s[3][k][None])
                if d is not None:
                    differs("pass: CU records", i, c, (k, j, {a: (b if a not in ("ours", "ref") else b.tolist()) for a, b in d.items()}))
                elif not np.array_equal(rec[j], s[1][k]):
                    differs("pass: reconstruction", i, c, (k, j, int((rec[j] != s[1][k]).sum())))
        if chain:  # pass with levels -> loop filters -> entropy coder, the device's own picture the next reference
            frames, rs, rf, cu, _ = seqs[0]
            bits = ic.oracle_encode_bits(oracle, w, h, frames, c["qp"], **kw)
            ip = inter.InterPictures(lib, w, h, 1, with_levels=True)
            try:
                ip.upload(0, frames[1], rf[0], cu[0].reshape(-1))  # the I picture after its loop filters, from the oracle
                for k in range(1, n):
                    prm = params_of(c, qps[k], k)
                    if k > 1:
                        ip.advance()
                        ip.upload_source(0, frames[k])
                    ip.run(prm)
                    rec, got = ip.download(0)
                    d = ic.first_difference(got[None], cu[k][None])
                    if d is not None or not np.array_equal(rec, rs[k]):
                        differs("chain: pass", i, c, (k, d if d is None else {a: (b if a not in ("ours", "ref") else b.tolist()) for a, b in d.items()}))
                    ip.loop_filters(prm)
                    rec, _ = ip.download(0)
                    if not np.array_equal(rec, rf[k]):
                        differs("chain: picture after the loop filters", i, c, (k, int((rec != rf[k]).sum())))
                    data, sizes = ip.entropy_code(prm)
                    if bytes(data) != bits[k][0] or [int(v) for v in sizes[0]] != list(bits[k][1]):
                        differs("chain: slice data", i, c, (k, [int(v) for v in sizes[0]], list(bits[k][1])))
            finally:
                ip.close()
        if tile:  # the picture as a tile of its frame: prediction and the co-located starting point reach beyond the tile, no TMVP, --no-wpp (tiles imply it)
            frames, rs, rf, cu, _ = seqs[0]
            tx, ty, tw, th = tile_of(c)
            p = ic.fuzz_options(c)
            for k in range(1, n):
                src = tc.tile_sub(frames[k], tx, ty, tw, th, w, h)
                ref_frame, ref_cu = np.ascontiguousarray(rf[k - 1]), np.ascontiguousarray(cu[k - 1])
                want_rec, want_cu = np.zeros(tw * th * 3 // 2, np.uint8), np.zeros((th // 4, tw // 4), ic.CU_DTYPE)
                sim.kvz_hostsim_inter_tile(tw, th, int(qps[k]), k, int(mc["coeff_weights"][str(int(qps[k]))]), fb.ctypes.data, 0, c["sao"], c["deblock"], p["fme_level"],
                                           p["pu_depth_inter_max"], 1, p["fast_residual_cost"], src.ctypes.data, ref_frame.ctypes.data, ref_cu.ctypes.data, want_rec.ctypes.data,
                                           want_cu.ctypes.data, w, h, tx, ty, 1)
                prm = params_of(dict(c, owf=0, no_wpp=1), qps[k], k, ref_width=w, ref_height=h, tile_x=tx, tile_y=ty, no_tmvp=1)
                rec, got = device_pass(lib, dev, tw, th, [src] * 2, [ref_frame] * 2, [ref_cu] * 2, prm)
                for j in range(2):
                    d = ic.first_difference(got[j][None], want_cu[None])
                    if d is not None or not np.array_equal(rec[j], want_rec):
                        differs("tile (%d, %d) %dx%d" % (tx, ty, tw, th), i, c, (k, j, d if d is None else {a: (b if a not in ("ours", "ref") else b.tolist()) for a, b in d.items()}))
    print("inter fuzz on the device: %d rounds in %.1f s, per family %s" % (ROUNDS, time.time() - t0, {k: v for k, v in sorted(counts.items()) if k}), flush=True)
    assert sim.kvz_hostsim_mul24_violations() == 0
    assert not bad, bad[:6]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,w,h", [("noise", 72, 40), ("binary", 136, 64), ("motion", 200, 136), ("smooth", 8, 8)])
def test_device_pass_at_picture_qp_0_equals_host_simulation(oracle, kind, w, h):
    """picture QP 0 on a B picture, which no --qp reaches in a low-delay sequence (see the module's docstring): the pass and the device sources in host
    simulation are handed QP 0 on the second picture of a `--qp 0` sequence, `veryfast` and `faster`"""
    import kvazaar_amd
    from kvazaar_amd.dev import Dev
    import tile_common as tc
    from test_gpu_inter_ctu import device_pass
    lib = kvazaar_amd.load_library()
    dev = Dev(lib)
    sim = tc.load_hostsim()
    sim.kvz_hostsim_mul24_violations.restype = C.c_ulonglong
    sim.kvz_hostsim_mul24_reset()
    mc = cc.model_constants()
    fb = np.array(mc["entropy_fbits"], np.float32)
    for preset in ("veryfast", "faster"):
        c = dict(w=w, h=h, n=2, qp=0, preset=preset, deblock=1, sao=1, no_wpp=0, owf=0, gop=(4, 3), kind=kind, seed=77, pan=(2.5, -1.0), noise=1.5, overrides={})
        frames = ic.fuzz_frames(c)
        rs, rf, cu, qps = ic.oracle_encode(oracle, w, h, frames, 0, **ic.fuzz_oracle_kwargs(c))
        assert qps[0] == 0
        p = ic.fuzz_options(c)
        want_rec, want_cu = np.zeros(w * h * 3 // 2, np.uint8), np.zeros((h // 4, w // 4), ic.CU_DTYPE)
        src, ref_frame, ref_cu = np.ascontiguousarray(frames[1]), np.ascontiguousarray(rf[0]), np.ascontiguousarray(cu[0])
        sim.kvz_hostsim_inter_tile(w, h, 0, 1, int(mc["coeff_weights"]["0"]), fb.ctypes.data, 0, 1, 1, p["fme_level"], p["pu_depth_inter_max"], 0, p["fast_residual_cost"], src.ctypes.data,
                                   ref_frame.ctypes.data, ref_cu.ctypes.data, want_rec.ctypes.data, want_cu.ctypes.data, 0, 0, 0, 0, 0)
        rec, got = device_pass(lib, dev, w, h, [src], [ref_frame], [ref_cu], params_of(c, 0, 1))
        assert ic.first_difference(got, want_cu[None]) is None, preset
        assert np.array_equal(rec[0], want_rec), preset
    assert sim.kvz_hostsim_mul24_violations() == 0
