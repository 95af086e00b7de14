"""Per-coefficient scaling lists in the inter CTU pass (kvz_hip_dev_inter_ctu_pass_lists, kvazaar's --scaling-list on B pictures) without a GPU: the device sources
compiled for the host with both forms of the inter program (tests/hostsim/hostsim_inter_lists.cpp).  The references exist independently of the code under test: the
reference encoder run with --gop lp-g4d3t1 --scaling-list default (tests/golden/inter_scaling_lists.json, made by tests/golden/make_inter_scaling_lists_golden.py)
for the pictures, the CU decisions and the slice data; tests/scaling_lists.py's tables (pinned to the compiled reference by tests/test_oracle_vs_ref.py) for the
factors of one block; the sequence oracle for the launch without sets."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import flatapi
import inter_common as ic
import inter_lists_common as ilc
import scaling_lists as sl
import scaling_lists_common as slc

NEW_SYMBOL = "kvz_hip_dev_inter_ctu_pass_lists"


@pytest.fixture(scope="module")
def sim():
    return ilc.load_sim()


@pytest.fixture(scope="module")
def intra_sim():
    return slc.load_sim()


@pytest.fixture(scope="module")
def hiplib():
    """libkvz_hip.so for its host-side functions only (the cost model of a QP): nothing here touches a device"""
    import kvazaar_amd
    return C.CDLL(kvazaar_amd.build_library())


@pytest.fixture(scope="module")
def gold():
    return ilc.fixture()


@pytest.fixture()
def in_range(sim):
    """the simulation's count of 24-bit multiplies with an operand out of range is zero over the test"""
    ilc.mul24_violations(sim, reset=True)
    yield
    assert ilc.mul24_violations(sim) == 0


@pytest.fixture(scope="module")
def flat_pan(oracle):
    """the `pan` clip encoded WITHOUT lists by the oracle: inputs of launches that need no chain (a B picture from the flat previous picture) and the flat truth"""
    clip = ilc.clip_named("pan")
    name, w, h, n, qp, preset, dbk, sao, owf, _ = clip
    frames = ic.case_frames(clip)
    rs, rf, cu, qps = ic.oracle_encode(oracle, w, h, frames, qp, preset=preset, deblock=bool(dbk), sao=bool(sao), mv_constraint=owf > 0)
    for a in (rs, rf, cu):
        a.setflags(write=False)
    return dict(clip=clip, frames=frames, rs=rs, rf=rf, cu=cu, qps=[int(q) for q in qps], w=w, h=h)


def _picture(seq, k):
    return dict(src=seq["frames"][k], ref=seq["rf"][k - 1], ref_cu=seq["cu"][k - 1])


# ---------------------------------------------------------------------------------------------------- 1. the chain against the reference encoder
@pytest.mark.parametrize("name", [c[0] for c in ilc.CLIPS])
def test_simulated_chain_equals_the_reference_encoder(sim, intra_sim, oracle, hiplib, gold, in_range, name):
    """I picture through the LISTS simulation of the all-intra pass, loop filters by the oracle, B pictures through kvz_hostsim_inter_pass_lists, loop filters, the
    B-slice coder == kvazaar --gop lp-g4d3t1 --scaling-list default: every final picture, every CU decision, the slice data of the pinned clip; and the levels
    populate the cells of the coverage table exactly as the fixture's generator counted them"""
    from kvazaar_amd import inter
    clip, g = ilc.clip_named(name), gold[name]
    _, w, h, n, *_ = clip
    chain = ilc.sim_chain(sim, intra_sim, oracle, hiplib, clip, "default", slice_data=name == ilc.PINNED)
    assert chain["qps"] == g["qps"]
    for k in range(n):
        assert ilc.sha(chain["final"][k]) == g["rec"][k], (name, k)
        assert inter.cu_digest(chain["cu"][k]) == g["cu"][k], (name, k)
    if name == ilc.PINNED:
        for k in range(1, n):
            data, sizes = chain["slices"][k]
            assert sizes == g["entropy"][k]["sizes"] and ilc.sha(np.frombuffer(data, np.uint8)) == g["entropy"][k]["sha"], (name, k)
    assert ilc.coverage(chain["cu"][1:], chain["coeff"][1:], w, h, chain["qps"][1:]) == g["coverage"], name


def test_coverage_table_has_no_empty_cell(gold):
    """inter and intra-in-B blocks of every transform size, on both sides of the dequantiser's branch, hold non-zero levels where the list entry is not 16"""
    total = {cell: sum(gold[c[0]]["coverage"].get(cell, 0) for c in ilc.CLIPS) for cell in ilc.CELLS}
    assert total == gold["coverage"] and all(v > 0 for v in total.values()), total
    assert all(changed > 0 for c in ilc.CLIPS for changed in gold[c[0]]["samples_changed_by_the_lists"][1:])


# ---------------------------------------------------------------------------------------------------- 2. no sets, other sets
def test_no_sets_through_the_new_twin_is_the_pictures_twin(sim, flat_pan, in_range):
    """n_sets == 0: kvz_hostsim_inter_pass_lists == kvz_hostsim_inter_pass_pictures of the library built without the switch, byte for byte, == the oracle"""
    import inter_mixed_common as imc
    flat_lib = ilc.load_flat_sim()
    s, clip = flat_pan, flat_pan["clip"]
    for k in (1, 2):
        pics, prm = [_picture(s, k)], ilc.params_of(clip, s["qps"][k], k)
        rc, rec, cu, coeff = ilc.sim_pass(sim, pics, prm, None, [], None, s["w"], s["h"])
        rc2, rec2, cu2, coeff2 = imc.hostsim_pass(flat_lib, pics, prm, None, w=s["w"], h=s["h"])
        assert rc == 0 and rc2 == 0
        assert rec.tobytes() == rec2.tobytes() and cu.tobytes() == cu2.tobytes() and coeff.tobytes() == coeff2.tobytes(), k
        assert np.array_equal(rec[0], s["rs"][k]) and ic.first_difference(cu, s["cu"][k][None]) is None, k


def test_flat_set_of_picture_is_a_launch_without_sets(sim, flat_pan, in_range):
    """a picture whose set is 0xffff runs the LISTS form on the flat list's rows: byte for byte what a launch without sets makes of it"""
    s, clip = flat_pan, flat_pan["clip"]
    pics, prm = [_picture(s, 1)], ilc.params_of(clip, s["qps"][1], 1)
    a = ilc.sim_pass(sim, pics, prm, None, [slc.lists("default")], [ilc.FLAT], s["w"], s["h"])
    b = ilc.sim_pass(sim, pics, prm, None, [], None, s["w"], s["h"])
    assert a[0] == 0 and b[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))


def test_custom_set_differs_from_default_and_from_flat(sim, flat_pan, in_range):
    s, clip = flat_pan, flat_pan["clip"]
    pics, prm = [_picture(s, 1)], ilc.params_of(clip, s["qps"][1], 1)
    outs = {name: ilc.sim_pass(sim, pics, prm, None, [slc.lists(name)] if name else [], None, s["w"], s["h"]) for name in ("default", "custom", None)}
    assert all(o[0] == 0 for o in outs.values())
    for a, b in (("default", "custom"), ("default", None), ("custom", None)):
        assert not np.array_equal(outs[a][1], outs[b][1]) and not np.array_equal(outs[a][3], outs[b][3]), (a, b)
    custom = sl.get("custom")
    assert all(not np.array_equal(custom.coeff[size, lst], custom.coeff[size, lst + 3]) for size in (0, 1, 2) for lst in range(3))  # inter lists distinct from the intra lists


# ---------------------------------------------------------------------------------------------------- 3. the factors of one block
# (intra CU of the B slice?, plane, log2 size): every block quantize_tu meets, with the inter 32x32 block -- list [3][1] through the reference's alias -- among them
BLOCKS = [(False, c, l2) for c in range(3) for l2 in (2, 3, 4, 5) if not (c and l2 == 5) and not (c == 0 and l2 == 2)] + [(True, 0, 3), (True, 0, 4), (True, 1, 2), (True, 2, 2), (True, 1, 3), (True, 2, 3)]


def _as_intra_lists(set_name, intra, c, l2):
    """a set whose INTRA list of plane c holds the list the reference takes for the block -- (intra CU ? 0 : 3) + c, the 32x32 one through its alias -- so that the
    all-intra simulation's block functions, which read lists 0-2, run on it"""
    from kvazaar_amd.batch import ScalingLists
    s = sl.get(set_name)
    lst = sl.list_type(intra, (0, 2, 3)[c])
    if l2 == 5 and lst == 3:
        lst = 1
    coeff, dc = s.coeff.copy(), s.dc.copy()
    slot = 0 if l2 == 5 else c
    coeff[l2 - 2, slot], dc[l2 - 2, slot] = s.coeff[l2 - 2, lst], s.dc[l2 - 2, lst]
    return ScalingLists(coeff, dc), lst


@pytest.mark.parametrize("set_name", ["default", "custom"])
def test_factors_of_a_block_are_those_of_the_list_the_reference_takes(sim, intra_sim, set_name):
    """quantize_tu's factors, read through the table and the records of a launch (kvz_hostsim_inter_list_factors), == tests/scaling_lists.py's quant_coeff /
    de_quant_coeff of list (intra CU ? 0 : 3) + plane at the block's qp % 6; and levels / coefficients computed from them == kvz_hostsim_lists_quant / _dequant run on
    that list (the I-slice rounding of those functions applied to both sides: the factors are what is compared)"""
    lists, tables = slc.lists(set_name), sl.get(set_name)
    rng = np.random.default_rng(3 + len(set_name))
    for qp in (0, 17, 22, 29, 30, 36, 41, 44, 47, 48, 51):
        for intra, c, l2 in BLOCKS:
            qs = qp if c == 0 else slc.flatapi_chroma_qp(qp)
            fwd, inv = ilc.list_factors(sim, lists, qp, intra, c, l2)
            moved, lst = _as_intra_lists(set_name, intra, c, l2)
            qtab, dtab = tables.tables(l2, lst, qs % 6)
            assert np.array_equal(fwd, qtab) and np.array_equal(inv, dtab), (qp, intra, c, l2)
            n = 1 << (2 * l2)
            coef, levels = rng.integers(-32768, 32768, n).astype(np.int16), rng.integers(-300, 301, n).astype(np.int16)
            q_bits, shift, per = 14 + qs // 6 + (15 - 8 - l2), 20 - 14 - (15 - 8 - l2) + 4, qs // 6
            want = (np.abs(coef.astype(np.int64)) * fwd + (171 << (q_bits - 9))) >> q_bits
            want = np.clip(np.where(coef < 0, -want, want), -32768, 32767).astype(np.int16)
            assert np.array_equal(slc.sim_block(intra_sim, "quant", moved, l2, c, qp, coef), want), (qp, intra, c, l2)
            prod = levels.astype(np.int64) * inv
            want = np.clip((prod + (1 << (shift - per - 1))) >> (shift - per), -32768, 32767) if shift > per else np.clip(np.clip(prod, -32768, 32767) << (per - shift), -32768, 32767)
            assert np.array_equal(slc.sim_block(intra_sim, "dequant", moved, l2, c, qp, levels), want.astype(np.int16)), (qp, intra, c, l2)
    fwd, inv = ilc.list_factors(sim, None, 22, False, 0, 5)  # a picture without a set: the flat list's row
    assert (fwd == (sl.QUANT_SCALES[22 % 6] << 4) // 16).all() and (inv == sl.INV_QUANT_SCALES[22 % 6] * 16).all()
    inter32, intra32 = ilc.list_factors(sim, lists, 22, False, 0, 5)[1], ilc.list_factors(sim, lists, 22, True, 0, 5)[1]
    assert not np.array_equal(inter32, intra32)  # 32x32: the inter list is not the intra one


# ---------------------------------------------------------------------------------------------------- 4. pictures of different QP, POC and set in one launch
def test_mixed_launch_in_ticket_order_equals_every_picture_alone(sim, flat_pan, in_range):
    """six pictures at three QPs, two POCs and the sets default / custom / none, walked as one persistent workgroup walks the launch -- consecutive CTUs from different
    pictures --: each picture comes out as from a launch of its own, and the flat ones as from a launch without sets"""
    from kvazaar_amd.inter import InterPictureParams
    s, clip = flat_pan, flat_pan["clip"]
    sets = [slc.lists("default"), slc.lists("custom")]
    mixed = [(1, 25, 0), (2, 30, 1), (1, 36, ilc.FLAT), (2, 25, 1), (1, 30, ilc.FLAT), (2, 36, 0)]  # (picture of the clip = POC, QP, set)
    pics = [_picture(s, k) for k, _, _ in mixed]
    prm = ilc.params_of(clip, 45, 9)  # qp / poc no picture has
    rc, rec, cu, coeff = ilc.sim_pass(sim, pics, prm, InterPictureParams([q for _, q, _ in mixed], [k for k, _, _ in mixed]), sets, [st for _, _, st in mixed], s["w"], s["h"])
    assert rc == 0
    for i, (k, qp, st) in enumerate(mixed):
        alone = ilc.sim_pass(sim, [pics[i]], ilc.params_of(clip, qp, k), None, [] if st == ilc.FLAT else [sets[st]], None, s["w"], s["h"])
        assert alone[0] == 0
        assert rec[i].tobytes() == alone[1][0].tobytes() and cu[i].tobytes() == alone[2][0].tobytes() and coeff[i].tobytes() == alone[3][0].tobytes(), (i, k, qp, st)


@pytest.mark.parametrize("qp", [44, 51])
def test_noise_at_the_left_side_qps_stays_in_range(sim, oracle, in_range, qp):
    """uniform noise handed to the pass at QP 44 (16x16 on the clip-and-shift-left side) and 51 (every size): large coefficients and levels, operands within 24 bits,
    both sets, pictures that differ from the flat ones"""
    w, h = 136, 72
    frames = ic.hard_clip("noise", w, h, 2, 60 + qp, (3.0, -2.0))
    rs, rf, cu, _ = ic.oracle_encode(oracle, w, h, frames, 22, preset="veryfast", deblock=True, sao=True)
    pic, clip = [dict(src=frames[1], ref=rf[0], ref_cu=cu[0])], ilc.clip_named("pan")
    flat = ilc.sim_pass(sim, pic, ilc.params_of(clip, qp, 1), None, [], None, w, h)
    for name in ("default", "custom"):
        got = ilc.sim_pass(sim, pic, ilc.params_of(clip, qp, 1), None, [slc.lists(name)], None, w, h)
        assert got[0] == 0 and np.count_nonzero(got[3]) > 0 and not np.array_equal(got[3], flat[3]), name


# ---------------------------------------------------------------------------------------------------- 5. refusals, the C ABI
def test_refusals(sim, flat_pan, capfd):
    """what kvz_scaling_lists.hpp refuses, through the text the library checks with: return code, message, nothing computed"""
    from kvazaar_amd.batch import ScalingLists
    s, clip = flat_pan, flat_pan["clip"]
    pics, prm = [_picture(s, 1)], ilc.params_of(clip, s["qps"][1], 1)
    entry12 = sl.get("default").coeff.copy()
    entry12[1, 3, 5] = 12
    size = slc.lists("default")
    size.struct.struct_size += 4
    dc = sl.get("default").dc.copy()
    dc[2, 4] = 300
    capfd.readouterr()
    for sets, index, message in (([ScalingLists(entry12)], None, "size 1 list 3 entry 5 is 12"), ([size], None, "struct_size"),
                                 ([ScalingLists(sl.get("default").coeff, dc)], None, "DC term is 300"), ([slc.lists("default")], [1], "set_of_picture[0] = 1 of 1")):
        rc, rec, cu, coeff = ilc.sim_pass(sim, pics, prm, None, sets, index, s["w"], s["h"])
        err = capfd.readouterr().err
        assert rc == -1 and not rec.any() and message in err and "kvz_hostsim_inter_pass_lists" in err, (message, err)
    rc, rec, _, _ = ilc.sim_pass(sim, pics, prm, None, [slc.lists("default")], [0], s["w"], s["h"])  # ... and the same arguments made right run
    assert rc == 0 and rec.any()


def test_header_declares_and_library_exports_the_entry_point():
    import kvazaar_amd
    dev = open(os.path.join(flatapi.ROOT, "include", "kvz_hip_dev.h")).read()
    m = re.search(r"\bint\s+" + NEW_SYMBOL + r"\((.*?)\);", dev, re.S)
    assert m and re.search(r"const kvz_hip_scaling_lists \*sets, int n_sets, const uint16_t \*set_of_picture\s*$", m.group(1)), m
    out = subprocess.check_output(["nm", "-D", "--defined-only", kvazaar_amd.build_library()], text=True)
    assert re.search(r"\bT " + NEW_SYMBOL + r"$", out, re.M)
