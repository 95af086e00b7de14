"""Per-coefficient scaling lists in the all-intra CTU pass (kvz_hip_batch_set_scaling_lists, kvazaar's --scaling-list) without a GPU: the device sources compiled
for the host with the LISTS instantiations of the CTU program (tests/hostsim/hostsim_scaling_lists.cpp).  The references exist independently of the code under
test: tests/scaling_lists.py's tables (pinned to the compiled reference by tests/test_oracle_vs_ref.py) applied in numpy and, where oracle/_ref is built, the
reference's own kvz_quant / kvz_dequant for one block; the reference encoder run with --scaling-list default (tests/golden/scaling_lists.json, made by
tests/golden/make_scaling_lists_golden.py) for the pass, the deblocked pictures and the slice data."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import ctu_common as cc
import deblock_common as dc
import flatapi
import inter_common as ic
import scaling_lists as sl
import scaling_lists_common as slc
import signhide_common as sc
from flatapi import A, ptr

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as mg  # noqa: E402

RECON = json.load(open(os.path.join(HERE, "golden", "encoder_recon.json")))


@pytest.fixture(scope="module")
def sim():
    return slc.load_sim()


@pytest.fixture(scope="module")
def hiplib():
    """libkvz_hip.so for its host-side functions only (the cost model of a QP, the default lists): nothing here touches a device"""
    import kvazaar_amd
    return C.CDLL(kvazaar_amd.build_library())


@pytest.fixture(scope="module")
def gold():
    return slc.fixture()


@pytest.fixture(scope="module")
def passes(sim, hiplib):
    """the host simulation of the pass with the default lists on every fixture clip, computed once: name -> (table, outputs per picture)"""
    out = {}
    for clip in slc.CLIPS:
        name, w, h, n, seed, kind, qp, preset, no_wpp = clip
        pm = slc.table(hiplib, [qp] * n, **slc.switches(clip))
        out[name] = (pm, slc.sim_pass(sim, pm, [slc.lists("default")], None, w, h, slc.clip_frames(clip)))
    return out


# ---------------------------------------------------------------------------------------------------- 1. the shared arithmetic on one block
# every (size, plane) the pass quantises: luma 4x4 .. 32x32 (4x4 luma only with NxN partitions; the arithmetic is the same), chroma 4x4 .. 16x16
BLOCKS = [(l2, c) for l2 in (2, 3, 4, 5) for c in (0, 1, 2) if not (c and l2 == 5)]


def _numpy_quant(coef, qtab, qp_scaled, l2):
    """quant-generic.c:57-81 at 8 bit, I slice, with quant_coeff[n]"""
    q_bits = 14 + qp_scaled // 6 + (15 - 8 - l2)
    a = np.abs(coef.astype(np.int64))
    level = (a * qtab.astype(np.int64) + (171 << (q_bits - 9))) >> q_bits
    return np.clip(np.where(coef < 0, -level, level), -32768, 32767).astype(np.int16)


def _numpy_dequant(levels, dtab, qp_scaled, l2):
    """quant-generic.c:309-333 at 8 bit with de_quant_coeff[n]"""
    shift, per = 20 - 14 - (15 - 8 - l2) + 4, qp_scaled // 6
    prod = levels.astype(np.int64) * dtab.astype(np.int64)
    if shift > per:
        return np.clip((prod + (1 << (shift - per - 1))) >> (shift - per), -32768, 32767).astype(np.int16)
    return np.clip(np.clip(prod, -32768, 32767) << (per - shift), -32768, 32767).astype(np.int16)


def _blocks(rng, l2, qp_scaled):
    """coefficient blocks from a fraction of a quantisation step to the int16 ends, and level blocks from 0 to the largest levels a block of that size can hold"""
    n = 1 << (2 * l2)
    step = (1 << (14 + qp_scaled // 6 + (15 - 8 - l2))) / sl.QUANT_SCALES[qp_scaled % 6]
    coefs = [np.clip(np.rint(rng.normal(0, max(2.0, step * amp), n)), -32768, 32767).astype(np.int16) for amp in (0.7, 3.0, 40.0)]
    coefs.append(rng.integers(-32768, 32768, n).astype(np.int16))
    levels = [rng.integers(-3, 4, n).astype(np.int16), rng.integers(-200, 201, n).astype(np.int16), rng.integers(-32768, 32768, n).astype(np.int16)]
    return coefs, levels


@pytest.mark.parametrize("set_name", ["default", "custom"])
def test_shared_arithmetic_equals_the_tables_applied_in_numpy(sim, set_name):
    """kvz_recon.hpp quant_level / dequant_level under the factors of kvz_scaling_lists.hpp, indexed by list_index == tests/scaling_lists.py's upsampled tables
    applied by the rule of quant-generic.c, at every size, plane and QP 0..51"""
    lists, tables = slc.lists(set_name), sl.get(set_name)
    rng = np.random.default_rng(7 + len(set_name))
    left = right = 0
    for qp in range(52):
        for l2, c in BLOCKS:
            qs = qp if c == 0 else slc.flatapi_chroma_qp(qp)
            qtab, dtab = tables.tables(l2, c, qs % 6)
            coefs, levels = _blocks(rng, l2, qs)
            for coef in coefs:
                got = slc.sim_block(sim, "quant", lists, l2, c, qp, coef)
                assert np.array_equal(got, _numpy_quant(coef, qtab, qs, l2)), (qp, l2, c)
            for lv in levels:
                got = slc.sim_block(sim, "dequant", lists, l2, c, qp, lv)
                assert np.array_equal(got, _numpy_dequant(lv, dtab, qs, l2)), (qp, l2, c)
            if l2 + 3 > qs // 6:
                right += 1
            else:
                left += 1
    assert left > 20 and right > 200  # both sides of the dequantiser's branch were walked


def test_flat_list_gives_the_flat_quantiser(sim, oracle):
    """the rows of a picture without lists (all entries 16) through the factor-taking rule == the per-call oracle's flat kvz_quant / kvz_dequant"""
    rng = np.random.default_rng(11)
    for qp in range(52):
        for l2, c in BLOCKS:
            qs = qp if c == 0 else slc.flatapi_chroma_qp(qp)
            coefs, levels = _blocks(rng, l2, qs)
            p = flatapi.QuantParams(qp=qp, bitdepth=8, slice_is_intra=1, signhide=0, scaling_list=0, cu_is_intra=1, quant_coeff=None, dequant_coeff=None)
            for coef in coefs[:3]:
                src, want = A(coef), A(np.zeros(coef.size, np.int16))
                oracle.quant(C.byref(p), ptr(src), ptr(want), 1 << l2, 1 << l2, (0, 2, 3)[c], 0, 1)
                assert np.array_equal(slc.sim_block(sim, "quant", None, l2, c, qp, coef), want), (qp, l2, c)
            for lv in levels[:2]:  # (levels a flat quantiser can produce: the flat rule's 32-bit product holds them)
                src, want = A(lv), A(np.zeros(lv.size, np.int16))
                oracle.dequant(C.byref(p), ptr(src), ptr(want), 1 << l2, 1 << l2, (0, 2, 3)[c], 1)
                assert np.array_equal(slc.sim_block(sim, "dequant", None, l2, c, qp, lv), want), (qp, l2, c)


@pytest.mark.parametrize("set_name", ["default", "custom"])
def test_shared_arithmetic_equals_the_compiled_reference(sim, reflib, set_name):
    """... == kvz_quant / kvz_dequant of the compiled reference after kvz_ref_set_scaling_list (skipped where oracle/_ref is not built)"""
    lists = slc.lists(set_name)
    rng = np.random.default_rng(13 + len(set_name))
    reflib.set_scaling_list(sl.get(set_name))
    try:
        for qp in range(52):
            p = flatapi.QuantParams(qp=qp, bitdepth=8, slice_is_intra=1, signhide=0, scaling_list=1, cu_is_intra=1, quant_coeff=None, dequant_coeff=None)
            for l2, c in BLOCKS:
                qs = qp if c == 0 else slc.flatapi_chroma_qp(qp)
                coefs, levels = _blocks(rng, l2, qs)
                for coef in coefs[:3]:
                    src, want = A(coef), A(np.zeros(coef.size, np.int16))
                    reflib.quant(C.byref(p), ptr(src), ptr(want), 1 << l2, 1 << l2, (0, 2, 3)[c], 0, 1)
                    assert np.array_equal(slc.sim_block(sim, "quant", lists, l2, c, qp, coef), want), (qp, l2, c)
                for lv in levels:
                    src, want = A(lv), A(np.zeros(lv.size, np.int16))
                    reflib.dequant(C.byref(p), ptr(src), ptr(want), 1 << l2, 1 << l2, (0, 2, 3)[c], 1)
                    assert np.array_equal(slc.sim_block(sim, "dequant", lists, l2, c, qp, lv), want), (qp, l2, c)
    finally:
        reflib.set_scaling_list(None)


def test_default_lists_of_the_library(hiplib):
    """kvz_hip_scaling_lists_default == kvz_scalinglist_get_default as tests/scaling_lists.py restates it (pinned to the reference there), DC 16"""
    from kvazaar_amd.batch import ScalingLists
    d, want = ScalingLists.default(hiplib), sl.get("default")
    assert d.struct.struct_size == C.sizeof(d.struct) == 4 + 4 * 6 * 64 * 4 + 4 * 6 * 4
    assert np.array_equal(d.coeff, want.coeff)
    assert np.array_equal(d.dc[:3], np.full((3, 6), 16)) and np.array_equal(d.dc[3], [16, 16, 0, 0, 0, 0])


# ---------------------------------------------------------------------------------------------------- 2. the pass, against the reference encoder
@pytest.mark.parametrize("clip", slc.CLIPS, ids=lambda c: c[0])
def test_host_pass_reproduces_the_reference_encoder_with_default_lists(oracle, passes, gold, clip):
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    pm, outs = passes[name]
    g = gold[name]
    assert [slc.sha(o["rec"]) for o in outs] == g["rec"]
    assert [mg.cu_digest(o["depth"].reshape(h // 8, w // 8), o["mode"].reshape(h // 8, w // 8)) for o in outs] == g["cu"]
    assert sorted({int(v) for o in outs for v in np.unique(o["depth"])}) == g["depths"]
    assert slc.coverage(outs, w, h, qp) == g["coverage"]
    if "deblock" in g:  # the host deblocking that exists, on the pictures the lists made
        deb = [dc.run_cpu(oracle.lib.kvz_oracle_deblock_frame, w, h, qp, 0, 0, o["rec"], o["depth"].reshape(h // 8, w // 8)) for o in outs]
        assert [slc.sha(d) for d in deb] == g["deblock"]
    if "entropy" in g:  # the entropy coder compiled for the host, on the pass's levels: the reference bitstream's slice data
        for i, (data, sizes) in enumerate(sc.sim_entropy(sc.load_sim(), pm, w, h, outs)):
            assert sizes == g["entropy"][i]["sizes"], i
            assert slc.sha(np.frombuffer(data, np.uint8)) == g["entropy"][i]["sha"], i
    # the lists are what makes these pictures: where the same clip has a digest without them, the two differ
    key = mg.clip_key(w, h, n, seed, kind, qp, 0, bool(no_wpp)) + ("/fast" if preset == "fast" else "")
    if key in RECON:
        assert all(a != b for i, (a, b) in enumerate(zip(g["rec"], RECON[key])) if i not in slc.UNTOUCHED_OK.get(name, ()))


def test_fixture_covers_what_it_claims(gold):
    assert slc.PINNED in gold and "deblock" in gold[slc.PINNED] and "entropy" in gold[slc.PINNED]
    assert gold["ultrafast-200x136-qp27"]["depths"] == [0, 1, 2, 3] and {1, 2, 3} <= set(gold["fast-200x136-qp27"]["depths"])
    for clip in slc.CLIPS:
        changed = gold[clip[0]]["samples_changed_by_the_lists"]
        assert all(c > 1000 for i, c in enumerate(changed) if i not in slc.UNTOUCHED_OK.get(clip[0], ())), clip[0]
        assert any(c > 1000 for c in changed), clip[0]
    # non-zero levels where the list entry is not 16, for every transform size on both sides of the dequantiser's branch
    assert sorted(gold["coverage"]) == sorted(slc.CELLS) and all(v > 0 for v in gold["coverage"].values()), gold["coverage"]
    assert gold["ultrafast-noise-qp44"]["coverage"]["luma-16-left"] > 0 and gold["ultrafast-noise-qp51"]["coverage"]["luma-32-left"] > 0  # qp / 6 == shift
    assert gold["ultrafast-noise-qp37"]["coverage"]["luma-8-left"] > 0 and gold["ultrafast-noise-qp37"]["coverage"]["chroma-4-left"] > 0


# ---------------------------------------------------------------------------------------------------- 3. pictures with and without lists in one launch
MIXED, mixed_batch = slc.MIXED, slc.mixed_batch


def test_mixed_launch_gives_every_picture_its_uniform_result(sim, hiplib, passes):
    frames, pm, sets, index = mixed_batch(hiplib)
    assert [int(pm.model_of(k).coeff_cabac) for k in range(6)] == [0, 0, 0, 0, 1, 1]  # both coefficient cost models in the one launch (coeff_cabac = qp >= 28)
    outs = slc.sim_pass(sim, pm, sets, index, 200, 136, frames)
    for k, (i, qp, s) in enumerate(MIXED):
        one = slc.table(hiplib, [qp])
        alone = slc.sim_pass(sim, one, [] if s == slc.FLAT else [sets[s]], None, 200, 136, [frames[k]])[0]  # (flat: a batch without lists, the instantiations of before)
        assert not cc.compare(outs[k], alone), (k, qp, s)
        if s == slc.FLAT:  # ... which the existing goldens pin to the reference encoder without lists
            assert slc.sha(outs[k]["rec"]) == RECON[mg.clip_key(200, 136, 2, 3, "small", qp, 0)][i]
    assert not cc.compare(outs[3], passes["ultrafast-200x136-qp27"][1][1])  # the default set at QP 27: the fixture's picture
    custom = slc.sim_pass(sim, slc.table(hiplib, [22]), [slc.lists("default")], None, 200, 136, [frames[1]])[0]
    assert slc.sha(custom["rec"]) != slc.sha(outs[1]["rec"])  # the custom set is not the default one


def test_fast_estimate_with_searched_32x32_cus(sim, hiplib, tmp_path):
    """search_32x32 without the CABAC coefficient cost (QP < 28): the LISTS instantiation <false, true>, which no preset's switches reach.  Where oracle/_ref is built,
    against the reference encoder run as `ultrafast --pu-depth-intra 1-3 --scaling-list default`; everywhere: it searches 32x32 CUs and the lists change the pictures"""
    w, h, qp = 200, 136, 22
    frames = cc.yuv_frames(w, h, 2, 3, "small")
    pm = slc.table(hiplib, [qp] * 2, search_32x32=1)
    assert all(pm.model_of(i).search_32x32 == 1 and pm.model_of(i).coeff_cabac == 0 for i in range(2))
    outs = slc.sim_pass(sim, pm, [slc.lists("default")], None, w, h, frames)
    flat = slc.sim_pass(sim, pm, [], None, w, h, frames)
    assert all(slc.sha(o["rec"]) != slc.sha(f["rec"]) for o, f in zip(outs, flat))
    assert 1 in {int(v) for o in outs for v in np.unique(o["depth"])}
    if os.path.exists(os.path.join(flatapi.ROOT, "oracle", "_ref", "kvazaar_ref")):
        recs = mg.reference_encoder_recon(w, h, frames, qp, 0, str(tmp_path), None, False, None, False, False, "ultrafast", extra=("--pu-depth-intra", "1-3", "--scaling-list", "default"))
        assert [slc.sha(o["rec"]) for o in outs] == [slc.sha(r) for r in recs]


# ---------------------------------------------------------------------------------------------------- 4. refusals
def _check(sim, sets, index, n_frames, ticket=1):
    f = sim.kvz_hostsim_lists_check
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
    arr = slc.set_array(sets)
    idx = None if index is None else (C.c_uint16 * len(index))(*index)
    return f(C.addressof(arr) if sets else None, len(sets), C.addressof(idx) if idx is not None else None, n_frames, ticket)


def test_sets_and_launches_the_library_refuses(sim, hiplib, capfd):
    from kvazaar_amd.batch import ScalingLists
    d = sl.get("default")
    ok = [slc.lists("default"), slc.lists("custom")]
    assert _check(sim, ok, [0, 1, slc.FLAT], 3) == 0 and _check(sim, ok, None, 3) == 0 and _check(sim, [], None, 3) == 0
    bad = slc.lists("default")
    bad.struct.struct_size += 4
    assert _check(sim, [bad], None, 1) == -1 and "struct_size" in capfd.readouterr().err
    for size, lst, i, v in ((1, 0, 5, 12), (2, 2, 63, 256), (0, 1, 15, 0), (3, 0, 7, -3)):  # 12: where the reference's int16 factor wraps
        coeff = d.coeff.copy()
        coeff[size, lst, i] = v
        assert _check(sim, [ScalingLists(coeff, d.dc)], None, 1) == -1 and "13 .. 255" in capfd.readouterr().err
    coeff = d.coeff.copy()
    coeff[1, 0, 5] = 13
    assert _check(sim, [ScalingLists(coeff, d.dc)], None, 1) == 0  # the lower bound itself is fine
    for v in (12, 256, -1):
        dcs = np.full((4, 6), 16, np.int32)
        dcs[2, 1] = v
        assert _check(sim, [ScalingLists(d.coeff, dcs)], None, 1) == -1 and "DC" in capfd.readouterr().err
    assert _check(sim, [ScalingLists(d.coeff, np.zeros((4, 6), np.int32))], None, 1) == 0  # DC 0 = 16
    assert _check(sim, ok, [0, 2], 2) == -1 and "set_of_picture" in capfd.readouterr().err
    assert _check(sim, ok, [0, 1], 2, ticket=0) == -1 and "scaling lists need the ticket schedule" in capfd.readouterr().err
    # a launch on a batch with lists: rdoq, search_nxn and signhide are refused, each with a message that names scaling lists, and nothing is computed
    frames = [np.zeros(64 * 64 * 3 // 2, np.uint8)]
    for sw in (dict(rdoq=1, coeff_cabac=1, search_32x32=1), dict(search_nxn=1, coeff_cabac=1, search_32x32=1), dict(signhide=1)):
        pm = slc.table(hiplib, [27], **sw)
        assert slc.sim_pass(sim, pm, [slc.lists("default")], None, 64, 64, frames) is None, sw
        assert "scaling lists" in capfd.readouterr().err
        if "signhide" not in sw:
            assert slc.sim_pass(sim, pm, [], None, 64, 64, frames) is not None  # ... and it is the lists that are refused with it
    assert slc.sim_pass(sim, slc.table(hiplib, [27]), [bad], None, 64, 64, frames) is None


def test_abi(hiplib):
    """the Python view of kvz_hip_scaling_lists is the header's struct, and kvz_hip_intra_cost_model did not grow"""
    from kvazaar_amd.batch import CostModel, ScalingListsStruct
    text = open(os.path.join(flatapi.ROOT, "include", "kvz_hip_types.h")).read()
    body = text[text.index("typedef struct kvz_hip_scaling_lists"):text.index("} kvz_hip_scaling_lists;")]
    assert [f[0] for f in ScalingListsStruct._fields_] == ["struct_size", "coeff", "dc"]
    assert "int32_t  coeff[4][6][64];" in body and "int32_t  dc[4][6];" in body
    assert ScalingListsStruct.coeff.offset == 4 and ScalingListsStruct.dc.offset == 4 + 4 * 6 * 64 * 4
    assert CostModel._fields_[-1][0] == "signhide"


# ---------------------------------------------------------------------------------------------------- 5. random cases against the encoder run live
PRESETS = slc.PRESETS


def draw_case(rng):
    """one round: a picture size (multiples of 8 from 8 to 264, a third of the draws below 64 in one or both dimensions), a QP 0..51, a preset `ultrafast`..`fast`
    and one of the content kinds of the inter fuzz (inter_common.draw_fuzz_case)"""
    w, h = int(rng.integers(1, 34)) * 8, int(rng.integers(1, 34)) * 8
    regime = int(rng.integers(0, 6))
    if regime == 0:
        w, h = int(rng.integers(1, 8)) * 8, int(rng.integers(1, 8)) * 8
    elif regime == 1:
        w = int(rng.integers(1, 8)) * 8
    elif regime == 2:
        h = int(rng.integers(1, 8)) * 8
    kinds = [k for k in ic.FUZZ_CONTENT if k != "motion" or (w > 40 and h > 40)]
    c = dict(w=w, h=h, n=2, qp=int(rng.integers(0, 52)), preset=list(PRESETS)[int(rng.integers(0, 5))], kind=kinds[int(rng.integers(0, len(kinds)))],
             seed=int(rng.integers(1, 1 << 30)), noise=float(rng.uniform(0, 3)))
    speed = float(rng.choice([3, 9]))
    c["pan"] = (float(round(rng.uniform(-speed, speed))), float(round(rng.uniform(-speed, speed))))
    return c


@pytest.mark.parametrize("round_", range(24))
def test_random_cases_against_the_reference_encoder(sim, hiplib, tmp_path, round_):
    if not os.path.exists(os.path.join(flatapi.ROOT, "oracle", "_ref", "kvazaar_ref")):
        pytest.skip("oracle/_ref not built (the GPU box): the committed digests are the check there")
    c = draw_case(np.random.default_rng(20261018 + round_))
    frames = ic.fuzz_frames(c)
    recs = mg.reference_encoder_recon(c["w"], c["h"], frames, c["qp"], 0, str(tmp_path), None, False, None, False, False, c["preset"], extra=("--scaling-list", "default"))
    pm = slc.table(hiplib, [c["qp"]] * c["n"], **PRESETS[c["preset"]])
    outs = slc.sim_pass(sim, pm, [slc.lists("default")], None, c["w"], c["h"], frames)
    assert [slc.sha(o["rec"]) for o in outs] == [slc.sha(r) for r in recs], c
