"""The inter CTU pass's choice of integer motion search (kvz_hip_inter_params me_algorithm / me_max_steps / me_early_termination: kvazaar's --me, --me-steps,
--me-early-termination) without a GPU: the device sources compiled for the host with both forms of the inter program (tests/hostsim/hostsim_inter_me.cpp).  The
reference exists independently of the code under test: the reference encoder run with --gop lp-g4d3t1 and the switches (tests/golden/inter_me.json, made by
tests/golden/make_inter_me_golden.py) for the final pictures and the slice data, which pins every CU decision, vector and level."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flatapi
import inter_common as ic
import inter_lists_common as ilc
import inter_me_common as mec
import inter_mixed_common as imc
import scaling_lists_common as slc


@pytest.fixture(scope="module")
def sim():
    return mec.load_sim()


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
    return mec.fixture()


@pytest.fixture()
def in_range(sim):
    """the simulation's count of 24-bit multiplies with an operand out of range is zero over the test"""
    ilc.mul24_violations(sim, reset=True)
    yield
    assert ilc.mul24_violations(sim) == 0


# ---------------------------------------------------------------------------------------------------- 1. the chain against the reference encoder
@pytest.mark.parametrize("clip_name,option", mec.cases(), ids=[mec.key(*c) for c in mec.cases()])
def test_simulated_chain_equals_the_reference_encoder(sim, intra_sim, oracle, hiplib, gold, in_range, clip_name, option):
    """I picture through the simulation of the all-intra pass, loop filters by the oracle, B pictures through kvz_hostsim_inter_pass_me, loop filters, the B-slice
    coder == kvazaar --gop lp-g4d3t1 with the option's switches: every final picture, the slice data of every B picture"""
    chain = mec.sim_chain(sim, intra_sim, oracle, hiplib, mec.clip_named(clip_name), option)
    mec.assert_chain_equals_fixture(chain, gold[mec.key(clip_name, option)], (clip_name, option))


def test_fixture_covers_what_it_is_there_for(gold):
    """every option differs from hexbs on some clip, the three termination settings from each other, all options of the first clip from each other; the clips lie on
    both sides of fast-residual-cost; and the generator's counters saw every branch of the searches"""
    for option in mec.ALL:
        if option != "hexbs":
            assert any(gold[mec.key(c[0], option)]["rec"] != gold[mec.key(c[0], "hexbs")]["rec"] for c, opts in mec.CLIPS if option in opts), option
    first = {o: tuple(gold[mec.key("pan11", o)]["rec"]) for o in mec.ALL}
    assert len(set(first.values())) == len(first)
    b_qps = [q for c, opts in mec.CLIPS for q in gold[mec.key(c[0], opts[0])]["qps"][1:]]
    assert min(b_qps) < 28 <= max(b_qps)
    assert {c[8] for c, _ in mec.CLIPS} == {0, 2}  # --owf
    assert all(gold["events"][k] > 0 for k in ("tz_from_zero", "star_two_rounds", "tz_distance_16", "full_extra_run", "full_extra_skipped", "merge_window_covered", "mv_refused",
                                               "leaves_left", "leaves_right", "leaves_top", "leaves_bottom", "dia_step_limit", "hex_step_limit")), gold["events"]


# ---------------------------------------------------------------------------------------------------- 2. zero members, aliases
def test_zero_members_are_the_pictures_twin(sim, oracle, in_range):
    """three zero members: kvz_hostsim_inter_pass_me == kvz_hostsim_inter_pass_pictures of the library built without the switch, byte for byte -- and a launch that
    runs the chosen form with hexbs, no step limit and `sensitive` spelt out (me_max_steps has no other spelling of "no limit": full is) gives the same bytes"""
    flat_lib = ilc.load_flat_sim()
    clip = mec.clip_named("pan11")
    name, w, h, n, qp, preset, dbk, sao, owf, _ = clip
    frames = ic.case_frames(clip)
    rs, rf, cu, qps = ic.oracle_encode(oracle, w, h, frames, qp, preset=preset, deblock=bool(dbk), sao=bool(sao), mv_constraint=owf > 0)
    for k in (1, 2):
        pics, prm = [dict(src=frames[k], ref=rf[k - 1], ref_cu=cu[k - 1])], mec.params_of(clip, int(qps[k]), k, "hexbs")
        assert (prm.me_algorithm, prm.me_max_steps, prm.me_early_termination) == (0, 0, 0)
        a = mec.sim_pass(sim, pics, prm, None, w, h)
        b = imc.hostsim_pass(flat_lib, pics, prm, None, w=w, h=h)
        assert a[0] == 0 and b[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:])), k
        assert np.array_equal(a[1][0], rs[k]) and ic.first_difference(a[2], cu[k][None]) is None, k


def test_full_is_full32(sim, oracle, in_range):
    """me_algorithm 2 (`full`) and 5 (`full32`) are the same search"""
    clip = mec.clip_named("one-ctu-qp20")
    name, w, h, n, qp, preset, dbk, sao, owf, _ = clip
    frames = ic.case_frames(clip)
    rs, rf, cu, qps = ic.oracle_encode(oracle, w, h, frames, qp, preset=preset, deblock=bool(dbk), sao=bool(sao), mv_constraint=owf > 0)
    pics, prm = [dict(src=frames[1], ref=rf[0], ref_cu=cu[0])], mec.params_of(clip, int(qps[1]), 1, "full32")
    a = mec.sim_pass(sim, pics, prm, None, w, h)
    prm.me_algorithm = 2
    b = mec.sim_pass(sim, pics, prm, None, w, h)
    assert a[0] == 0 and b[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))
    assert not np.array_equal(a[1][0], rs[1])  # ... and not the default one


def test_pictures_with_their_own_qp_and_poc_share_a_launch(sim, oracle, in_range):
    """a table of QPs and POCs (kvz_hip_inter_pictures) under tz: every picture of the one launch is what a launch of its own makes of it"""
    from kvazaar_amd.inter import InterPictureParams
    clip = mec.clip_named("pan11")
    name, w, h, n, qp, preset, dbk, sao, owf, _ = clip
    frames = ic.case_frames(clip)
    rs, rf, cu, qps = ic.oracle_encode(oracle, w, h, frames, qp, preset=preset, deblock=bool(dbk), sao=bool(sao), mv_constraint=owf > 0)
    pics = [dict(src=frames[k], ref=rf[k - 1], ref_cu=cu[k - 1]) for k in (1, 2, 1)]
    table = InterPictureParams([int(qps[1]), int(qps[2]), 22], [1, 2, 1])
    joint = mec.sim_pass(sim, pics, mec.params_of(clip, 40, 7, "tz"), table, w, h)
    assert joint[0] == 0
    for i, (q, poc) in enumerate(zip(table.qps, table.pocs)):
        alone = mec.sim_pass(sim, [pics[i]], mec.params_of(clip, int(q), int(poc), "tz"), None, w, h)
        assert alone[0] == 0 and all(x[i].tobytes() == y[0].tobytes() for x, y in zip(joint[1:], alone[1:])), i


# ---------------------------------------------------------------------------------------------------- 3. what is refused
def test_refusals(sim, capfd):
    """the twin of the entry points' argument check: an algorithm outside 0 .. 7, negative steps, a termination value outside 0 .. 2, and a non-zero member together
    with tiles, with scaling lists or in a joint launch -- each with a message that names the member; everything else passes"""
    clip = mec.clip_named("pan11")

    def prm(**kw):
        p = mec.params_of(clip, 27, 1, "hexbs")
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    capfd.readouterr()
    for kw, where, message in ((dict(me_algorithm=8), {}, "me_algorithm 8 outside 0..7"), (dict(me_algorithm=-1), {}, "me_algorithm -1 outside 0..7"),
                               (dict(me_max_steps=-1), {}, "me_max_steps -1 is negative"), (dict(me_early_termination=3), {}, "me_early_termination 3 outside 0..2"),
                               (dict(me_early_termination=-1), {}, "me_early_termination -1 outside 0..2"),
                               (dict(me_algorithm=1), dict(has_tiles=True), "tiles"), (dict(me_max_steps=2, ref_width=136, ref_height=72), {}, "tiles"),
                               (dict(me_early_termination=1), dict(n_sets=1), "scaling lists"), (dict(me_algorithm=7), dict(joint=True), "a joint launch"),
                               (dict(me_algorithm=9), dict(joint=True), "me_algorithm 9 outside 0..7")):
        assert mec.me_check(sim, prm(**kw), **where) == -1, (kw, where)
        err = capfd.readouterr().err
        assert message in err and "kvz_hip_dev_inter_ctu_pass" in err, (kw, where, err)
    for kw, where in ((dict(), dict(has_tiles=True)), (dict(), dict(n_sets=2)), (dict(), dict(joint=True)), (dict(me_algorithm=7, me_max_steps=1000, me_early_termination=2), {}),
                      (dict(me_algorithm=0, me_max_steps=1), {}), (dict(me_algorithm=6), {})):
        assert mec.me_check(sim, prm(**kw), **where) == 0, (kw, where)
    assert capfd.readouterr().err == ""


def test_the_struct_from_before_the_members_is_still_taken(sim, oracle, capfd):
    """a caller compiled before the three members hands over the struct that ends with no_tmvp (struct_size 60): accepted, and whatever lies behind those bytes is not
    read -- its launch is the default search's, byte for byte; every other size is refused"""
    from kvazaar_amd.inter import InterParams
    clip = mec.clip_named("one-ctu-qp20")
    name, w, h, n, qp, preset, dbk, sao, owf, _ = clip
    frames = ic.case_frames(clip)
    rs, rf, cu, qps = ic.oracle_encode(oracle, w, h, frames, qp, preset=preset, deblock=bool(dbk), sao=bool(sao), mv_constraint=owf > 0)
    pics = [dict(src=frames[1], ref=rf[0], ref_cu=cu[0])]
    before = InterParams.me_algorithm.offset
    assert before == 60 and C.sizeof(InterParams) == 72
    old = mec.params_of(clip, int(qps[1]), 1, "tz-et-off")  # the members are set, but lie behind what the caller says it filled
    old.struct_size = before
    assert mec.me_check(sim, old) == 0 and mec.me_check(sim, old, has_tiles=True) == 0 and mec.me_check(sim, old, joint=True) == 0
    a = mec.sim_pass(sim, pics, old, None, w, h)
    b = mec.sim_pass(sim, pics, mec.params_of(clip, int(qps[1]), 1, "hexbs"), None, w, h)
    assert a[0] == 0 and b[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))
    assert np.array_equal(a[1][0], rs[1])
    capfd.readouterr()
    for size in (0, 56, 64, 68, 76):
        old.struct_size = size
        assert mec.me_check(sim, old) == -1 and mec.sim_pass(sim, pics, old, None, w, h)[0] == -1, size
        assert "kvz_hip_inter_params.struct_size" in capfd.readouterr().err


def test_a_refused_launch_computes_nothing(sim):
    clip = mec.clip_named("one-ctu-qp20")
    name, w, h, n, qp, *_ = clip
    frames = ic.case_frames(clip)
    from kvazaar_amd import inter
    pic = dict(src=frames[1], ref=frames[0], ref_cu=inter.intra_picture_cu_info(w, h))
    p = mec.params_of(clip, 22, 1, "tz")
    p.me_algorithm = 8
    rc, rec, cu, coeff = mec.sim_pass(sim, [pic], p, None, w, h)
    assert rc == -1 and not rec.any() and not coeff.any() and not cu["type"].any()


# ---------------------------------------------------------------------------------------------------- 4. the interface as a text
def test_header_binding_and_build_list_agree():
    """kvz_hip_inter_params ends with the three members, in the binding's order; the helper maps kvazaar's words; the build has the two ME units"""
    from kvazaar_amd import build, inter
    text = open(os.path.join(flatapi.ROOT, "include", "kvz_hip_dev.h")).read()
    body = text[text.index("typedef struct kvz_hip_inter_params {"):text.index("} kvz_hip_inter_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [n.strip() for decl in re.findall(r"(?:uint32_t|int32_t)\s+([^;]+);", body) for n in decl.split(",")]
    assert members == [f[0] for f in inter.InterParams._fields_] and members[-3:] == ["me_algorithm", "me_max_steps", "me_early_termination"]
    assert inter.me_search_fields() == dict(me_algorithm=0, me_max_steps=0, me_early_termination=0)
    assert inter.me_search_fields(me="tz", me_steps=2, me_early_termination="on") == dict(me_algorithm=1, me_max_steps=2, me_early_termination=1)
    assert [inter.ME_ALGORITHMS[k] for k in ("hexbs", "tz", "full", "full8", "full16", "full32", "full64", "dia")] == list(range(8))  # kvazaar.h enum kvz_ime_algorithm
    for bad in (dict(me="umh"), dict(me_steps=0), dict(me_steps=-2), dict(me_early_termination="maybe")):
        with pytest.raises(ValueError):
            inter.me_search_fields(**bad)
    units = {name: defs for name, _, defs in build.UNITS}
    assert units["kvz_inter_tu6"] == ["-DKVZ_ICTU_ME=1", "-DKVZ_ICTU_CABAC=0"] and units["kvz_inter_tu7"] == ["-DKVZ_ICTU_ME=1", "-DKVZ_ICTU_CABAC=1"]
