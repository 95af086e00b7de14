"""P pictures (kvazaar's --no-bipred: kvz_hip_dev_inter_ctu_pass_slices, kvz_hip_dev_loop_filters_inter_slices and kvz_hip_dev_entropy_code_inter_slices with
KVZ_HIP_SLICE_P) without a GPU: the device sources compiled for the host with both forms of the inter program (tests/hostsim/hostsim_inter_p.cpp).  The reference
exists independently of the code under test: the reference encoder run with --no-bipred (tests/golden/inter_p.json, made by tests/golden/make_inter_p_golden.py)
for the final pictures and the slice data, which pins every CU decision, vector and level.  Every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flatapi
import inter_common as ic
import inter_lists_common as ilc
import inter_mixed_common as imc
import inter_p_common as pc
import scaling_lists_common as slc


@pytest.fixture(scope="module")
def sim():
    return pc.load_sim()


@pytest.fixture(scope="module")
def intra_sim():
    return slc.load_sim()


@pytest.fixture(scope="module")
def hiplib():
    """libkvz_hip.so for its host-side functions and its symbol table only: nothing here touches a device"""
    import kvazaar_amd
    return C.CDLL(kvazaar_amd.build_library())


@pytest.fixture(scope="module")
def gold():
    return pc.fixture()


@pytest.fixture()
def in_range(sim):
    """the simulation's count of 24-bit multiplies with an operand out of range is zero over the test"""
    ilc.mul24_violations(sim, reset=True)
    yield
    assert ilc.mul24_violations(sim) == 0


@pytest.fixture(scope="module")
def b_sequence(oracle):
    """pan11 as the oracle's B encode: reference pictures and records for launches that are compared with each other, not with a fixture"""
    clip = pc.clip_named("pan11")
    name, w, h, n, qp, preset, dbk, sao, owf, _ = clip
    frames = ic.case_frames(clip)
    rs, rf, cu, qps = ic.oracle_encode(oracle, w, h, frames, qp, preset=preset, deblock=bool(dbk), sao=bool(sao), mv_constraint=owf > 0)
    return clip, frames, rs, rf, cu, [int(q) for q in qps]


# ---------------------------------------------------------------------------------------------------- 1. the chain against the reference encoder
@pytest.mark.parametrize("clip_name", pc.names())
def test_simulated_chain_equals_the_reference_encoder(sim, intra_sim, oracle, hiplib, gold, in_range, clip_name):
    """I picture through the simulation of the all-intra pass, loop filters by the oracle, P pictures through kvz_hostsim_inter_pass_slices, the oracle's loop filters
    under the rule of a slice that is not B from the P row's SAO states, the P-slice coder == kvazaar --no-bipred: every final picture, the slice data of every
    P picture.  No record of a P picture moves by list 1"""
    counts = {}
    chain = pc.sim_chain(sim, intra_sim, oracle, hiplib, pc.clip_named(clip_name), pc.gop_of(clip_name), pc.P, counts)
    pc.assert_chain_equals_fixture(chain, gold[clip_name], clip_name)
    assert counts["mv_dir_not_1"] == 0 and counts["merge_list_unknown"] == 0, counts
    for cu in chain["cu"][1:]:
        inter = cu["type"] == 2
        assert not (cu["mv"][inter][:, 1] != 0).any() and set(np.unique(cu["mv_ref"][inter][:, 1])) <= {0, 255} and not cu["mv_cand"][inter][:, 1].any()


def test_fixture_covers_what_it_is_there_for(gold):
    """the generator's census: every event at least 16 times, no mv_dir other than 1; P pictures on both sides of fast-residual-cost 28 and at both ends of the QP
    range; with and without the MV constraint, SAO and deblocking; the --gop 0 case at one QP; every case's pictures differ from the B encode's (asserted by the
    generator, which recorded both encodes' sizes)"""
    assert all(gold["census"][k] >= pc.CENSUS_MIN for k in pc.CENSUS_REQUIRED), gold["census"]
    assert gold["census"]["mv_dir_not_1"] == 0 and gold["census"]["merge_list_unknown"] == 0
    p_qps = [q for name in pc.names() for q in gold[name]["qps"][1:]]
    assert min(p_qps) < 28 <= max(p_qps) and min(p_qps) <= 3 and max(p_qps) == 51
    assert {c[8] for c, _ in pc.CLIPS} == {0, 2} and {c[7] for c, _ in pc.CLIPS} == {0, 1} and {c[6] for c, _ in pc.CLIPS} == {0, 1}
    assert len(set(gold["pan11-gop0"]["qps"])) == 1 and gold["pan11-gop0"]["rec"] != gold["pan11"]["rec"]
    assert all(gold[name]["b_encode"]["bytes"] > 0 for name in pc.names())


# ---------------------------------------------------------------------------------------------------- 2. B through the new entries; P is not B
def test_slice_type_b_is_the_pictures_twin(sim, oracle, b_sequence, in_range):
    """KVZ_HIP_SLICE_B: kvz_hostsim_inter_pass_slices == kvz_hostsim_inter_pass_pictures of the library built without the switch, and the coder's twin == the B-slice
    coder simulation, byte for byte; the same launch as P gives other bytes"""
    flat_lib = ilc.load_flat_sim()
    clip, frames, rs, rf, cu, qps = b_sequence
    name, w, h, n, *_ = clip
    for k in (1, 2):
        pics, prm = [dict(src=frames[k], ref=rf[k - 1], ref_cu=cu[k - 1])], pc.params_of(clip, qps[k], k)
        a = pc.sim_pass(sim, pics, prm, None, w, h, pc.B)
        b = imc.hostsim_pass(flat_lib, pics, prm, None, w=w, h=h)
        assert a[0] == 0 and b[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:])), k
        assert np.array_equal(a[1][0], rs[k]) and ic.first_difference(a[2], cu[k][None]) is None, k
        p = pc.sim_pass(sim, pics, prm, None, w, h, pc.P)
        assert p[0] == 0 and p[1].tobytes() != a[1].tobytes() and (p[2]["mv_dir"][p[2]["type"] == 2] == 1).all(), k
        final, recs, merge = ilc.oracle_loop_filters(oracle, clip, qps[k], True, frames[k], a[1][0], a[2][0])
        want = ilc.sim_slice_data(sim, oracle, w, h, qps[k], k, a[2][0], cu[k - 1], a[3][0], recs, merge)
        assert pc.sim_slice_data(sim, pc.B, w, h, [qps[k]], [k], a[2][0], cu[k - 1], a[3][0], recs, merge) == want, k
        assert pc.sim_slice_data(sim, pc.P, w, h, [qps[k]], [k], a[2][0], cu[k - 1], a[3][0], recs, merge) != want, k


def test_b_rows_are_the_oracles_and_p_rows_differ_where_the_tables_do(sim, oracle):
    """the coder's initial states: the B row is the oracle's at every QP; the P row differs from it in the contexts whose initType-1 values differ -- merge flag and
    index, pred-mode flag, abs_mvd_greater0, the intra luma mode, cbf_cb / cbf_cr at depth 1, residual contexts, sao_type_idx -- and in nothing else"""
    differ = set()
    for qp in range(52):
        b, p = pc.slice_contexts(sim, pc.B, qp), pc.slice_contexts(sim, pc.P, qp)
        assert np.array_equal(b[:166], ic.b_slice_context_states(oracle, qp)[:166]), qp  # (through KVZ_EB_CX_ROOT_CBF: the two entries behind it are no contexts)
        differ |= set(np.flatnonzero(b != p).tolist())
    syntax = {4, 9, 149, 153, 154, 155, 156}  # KVZ_HIP_CX_INTRA, _CBF_CHROMA + 1, _SAO_TYPE; KVZ_EB_CX_MERGE_FLAG, _MERGE_IDX, _PRED_MODE, _MVD
    assert syntax <= differ and all(10 <= i < 146 for i in differ - syntax), sorted(differ)
    f = sim.kvz_hostsim_sao_type_init_value
    f.restype = C.c_int
    assert [f(t) for t in (pc.B, pc.P, pc.I)] == [160, 185, 200]


# ---------------------------------------------------------------------------------------------------- 3. pictures with their own QP and POC
def test_p_pictures_with_their_own_qp_and_poc_share_a_launch(sim, b_sequence, in_range):
    """a table of QPs and POCs (kvz_hip_inter_pictures) under KVZ_HIP_SLICE_P, fast and CABAC pricing side by side: every picture of the one launch, and of the one
    coder call, is what a launch of its own makes of it"""
    from kvazaar_amd.inter import InterPictureParams
    clip, frames, rs, rf, cu, qps = b_sequence
    name, w, h, n, *_ = clip
    pics = [dict(src=frames[k], ref=rf[k - 1], ref_cu=cu[k - 1]) for k in (1, 2, 1)]
    table = InterPictureParams([qps[1], 33, 22], [1, 2, 1])
    joint = pc.sim_pass(sim, pics, pc.params_of(clip, 40, 7), table, w, h, pc.P)
    assert joint[0] == 0
    data, sizes = pc.sim_slice_data(sim, pc.P, w, h, table.qps, table.pocs, joint[2], np.stack([p["ref_cu"] for p in pics]), joint[3], None, None)
    rows, at = (h + 63) // 64, 0
    for i, (q, poc) in enumerate(zip(table.qps, table.pocs)):
        alone = pc.sim_pass(sim, [pics[i]], pc.params_of(clip, int(q), int(poc)), None, w, h, pc.P)
        assert alone[0] == 0 and all(x[i].tobytes() == y[0].tobytes() for x, y in zip(joint[1:], alone[1:])), i
        own, own_sizes = pc.sim_slice_data(sim, pc.P, w, h, [int(q)], [int(poc)], alone[2], pics[i]["ref_cu"], alone[3], None, None)
        assert sizes[i * rows:(i + 1) * rows] == own_sizes and data[at:at + len(own)] == own, i
        at += len(own)
    assert at == len(data)


# ---------------------------------------------------------------------------------------------------- 4. what is refused
def test_refusals(sim, capfd):
    """the twins of the three entry points' checks: a slice type that is none of the three everywhere; I for the pass and the coder; P together with tiles or with a
    non-zero me_* member -- each -1 with a message that names the entry point and the reason; everything else passes without a word"""
    clip = pc.clip_named("pan11")

    def prm(**kw):
        p = pc.params_of(clip, 27, 1)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    capfd.readouterr()
    refused = [(dict(), 3, "pass", {}, "slice type 3 is none of"), (dict(), -1, "coder", {}, "slice type -1 is none of"), (dict(), 7, "loop_filters", {}, "slice type 7 is none of"),
               (dict(), pc.I, "pass", {}, "slice type I"), (dict(), pc.I, "coder", {}, "slice type I"),
               (dict(ref_width=136, ref_height=72), pc.P, "pass", {}, "together with tiles"), (dict(tile_x=8), pc.P, "pass", {}, "together with tiles"),
               (dict(tile_y=8), pc.P, "pass", {}, "together with tiles"), (dict(), pc.P, "pass", dict(has_tile_xy=True), "together with tiles"),
               (dict(me_algorithm=1), pc.P, "pass", {}, "together with me_algorithm"), (dict(me_max_steps=2), pc.P, "pass", {}, "together with me_algorithm"),
               (dict(me_early_termination=1), pc.P, "pass", {}, "together with me_algorithm")]
    for kw, slice_type, stage, where, message in refused:
        assert pc.slices_check(sim, prm(**kw), slice_type, stage, **where) == -1, (kw, slice_type, stage)
        err = capfd.readouterr().err
        entry = {"pass": "kvz_hip_dev_inter_ctu_pass_slices", "loop_filters": "kvz_hip_dev_loop_filters_inter_slices", "coder": "kvz_hip_dev_entropy_code_inter_slices"}[stage]
        assert message in err and entry in err, (kw, slice_type, stage, err)
    for kw, slice_type, stage, where in ((dict(), pc.P, "pass", {}), (dict(), pc.B, "pass", dict(has_tile_xy=True)), (dict(me_algorithm=1), pc.B, "pass", {}),
                                         (dict(ref_width=136, ref_height=72), pc.B, "pass", {}), (dict(), pc.I, "loop_filters", {}), (dict(), pc.P, "loop_filters", {}),
                                         (dict(), pc.B, "loop_filters", {}), (dict(), pc.P, "coder", {}), (dict(), pc.B, "coder", {})):
        assert pc.slices_check(sim, prm(**kw), slice_type, stage, **where) == 0, (kw, slice_type, stage)
    assert capfd.readouterr().err == ""


def test_a_refused_launch_computes_nothing(sim, capfd):
    """every refusal of the pass's twin returns -1 and leaves the output buffers as they were; the coder's twin returns nothing for a slice type it refuses"""
    from kvazaar_amd import inter
    clip = pc.clip_named("one-ctu-qp20")
    name, w, h, n, qp, *_ = clip
    frames = ic.case_frames(clip)
    pic = dict(src=frames[1], ref=frames[0], ref_cu=inter.intra_picture_cu_info(w, h))
    fs, cells = w * h * 3 // 2, (w // 4) * (h // 4)
    for kw, slice_type, tile_xy in ((dict(), 3, None), (dict(), pc.I, None), (dict(me_algorithm=1), pc.P, None), (dict(ref_width=w, ref_height=h), pc.P, None), (dict(), pc.P, [[0, 0]]),
                                    (dict(struct_size=64), pc.P, None)):
        p = pc.params_of(clip, 22, 1)
        for k, v in kw.items():
            setattr(p, k, v)
        out = (np.full(fs, 0xa5, np.uint8), np.frombuffer(bytes([0x5a]) * (cells * ic.CU_DTYPE.itemsize), ic.CU_DTYPE).copy(), np.full(6144, 0x1234, np.int16))
        rc, rec, cu, coeff = pc.sim_pass(sim, [pic], p, None, w, h, slice_type, tile_xy=tile_xy, out=out)
        assert rc == -1 and (rec == 0xa5).all() and (coeff == 0x1234).all() and cu.tobytes() == bytes([0x5a]) * cu.nbytes, (kw, slice_type)
        assert "kvz_hip_dev_inter_ctu_pass" in capfd.readouterr().err
    cu = inter.intra_picture_cu_info(w, h)
    assert pc.sim_slice_data(sim, pc.I, w, h, [22], [1], cu, cu, np.zeros(6144, np.int16), None, None) is None
    assert pc.sim_slice_data(sim, 5, w, h, [22], [1], cu, cu, np.zeros(6144, np.int16), None, None) is None


# ---------------------------------------------------------------------------------------------------- 5. the interface as a text
def test_header_library_binding_and_build_list_agree(hiplib):
    """the headers declare the three entry points and the three constants with kvazaar's values, the library exports the entry points, the binding knows the
    values, kvz_hip_inter_params is what it was, and the build has the two P units"""
    from kvazaar_amd import build, inter
    dev = open(os.path.join(flatapi.ROOT, "include", "kvz_hip_dev.h")).read()
    types = open(os.path.join(flatapi.ROOT, "include", "kvz_hip_types.h")).read()
    for name, ret in (("kvz_hip_dev_inter_ctu_pass_slices", "int"), ("kvz_hip_dev_loop_filters_inter_slices", "int"), ("kvz_hip_dev_entropy_code_inter_slices", "long")):
        decl = re.search(ret + r"\s+" + name + r"\(([^;]*)\);", dev)
        assert decl and "int slice_type" in decl.group(1), name
        assert hasattr(hiplib, name), name
    assert re.search(r"kvz_hip_dev_inter_ctu_pass_slices\([^;]*const kvz_hip_inter_pictures \*pictures, int slice_type\);", dev)
    assert re.search(r"kvz_hip_dev_entropy_code_inter_slices\([^;]*const kvz_hip_inter_pictures \*pictures, int slice_type\);", dev)
    assert re.search(r"kvz_hip_dev_loop_filters_inter_slices\([^;]*int qp,\s+const int32_t \*qp_of_picture, int slice_type, int deblock", dev)
    assert re.search(r"enum \{ KVZ_HIP_SLICE_B = 0, KVZ_HIP_SLICE_P = 1, KVZ_HIP_SLICE_I = 2 \};", types)
    assert inter.SLICE_TYPES == dict(B=0, P=1, I=2) and (pc.B, pc.P, pc.I) == (0, 1, 2)
    assert inter.slice_type_value("P") == 1 and inter.slice_type_value(2) == 2
    with pytest.raises(ValueError):
        inter.slice_type_value("X")
    assert C.sizeof(inter.InterParams) == 72
    units = {name: defs for name, _, defs in build.UNITS}
    assert units["kvz_inter_tu8"] == ["-DKVZ_ICTU_P=1", "-DKVZ_ICTU_CABAC=0"] and units["kvz_inter_tu9"] == ["-DKVZ_ICTU_P=1", "-DKVZ_ICTU_CABAC=1"]
    kernels = open(os.path.join(flatapi.ROOT, "kvazaar_amd", "csrc", "kvz_inter_kernels.hpp")).read()
    builds = open(os.path.join(flatapi.ROOT, "kvazaar_amd", "csrc", "kvz_inter_builds.hpp")).read()  # the kernels' names: inter_ctu_ticket_kernel_ and the suffix of a row of the list
    assert "KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_##suffix);" in kernels and re.search(r"\bX\(8, p_fast, ", builds) and re.search(r"\bX\(9, p_cabac, ", builds)
    assert re.search(r"#if KVZ_ICTU_P && \(KVZ_ICTU_LISTS \|\| KVZ_ICTU_JOINT \|\| KVZ_ICTU_ME\)\n#error", kernels)


def test_python_defaults_leave_the_existing_callers_untouched():
    """InterPictures.run / .loop_filters / .entropy_code: slice_type defaults to "B" / None / "B", behind the arguments they have always had"""
    import inspect
    from kvazaar_amd.inter import InterPictures
    run, lf, ec_ = (inspect.signature(getattr(InterPictures, n)) for n in ("run", "loop_filters", "entropy_code"))
    assert list(run.parameters) == ["self", "params", "pictures", "slice_type"] and run.parameters["slice_type"].default == "B"
    assert list(lf.parameters) == ["self", "params", "slice_is_b", "pictures", "slice_type"] and lf.parameters["slice_type"].default is None and lf.parameters["slice_is_b"].default is True
    assert list(ec_.parameters) == ["self", "params", "pictures", "slice_type"] and ec_.parameters["slice_type"].default == "B"
