"""P pictures with reference lists of 1 to 4 pictures (kvazaar's --no-bipred --ref N: kvz_hip_dev_inter_ctu_pass_refs, kvz_hip_dev_loop_filters_inter_refs and
kvz_hip_dev_entropy_code_inter_refs) without a GPU: the device sources compiled for the host with every form of the inter program
(tests/hostsim/hostsim_inter_refs.cpp).  The reference exists independently of the code under test: the reference encoder run with --no-bipred --ref N
(tests/golden/inter_refs.json, made by tests/golden/make_inter_refs_golden.py) for the final pictures and the slice data, which pins every CU decision, reference
index, vector and level; H.265 and kvazaar's cfg.c, read and typed in here, for the scaling, the contexts and the lists.  Every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flatapi
import inter_common as ic
import inter_lists_common as ilc
import inter_p_common as pc
import inter_refs_common as rc
import scaling_lists_common as slc


@pytest.fixture(scope="module")
def sim():
    return rc.load_sim()


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
    return rc.fixture()


@pytest.fixture()
def in_range(sim):
    """the simulation's count of 24-bit multiplies with an operand out of range is zero over the test"""
    ilc.mul24_violations(sim, reset=True)
    yield
    assert ilc.mul24_violations(sim) == 0


@pytest.fixture(scope="module")
def alt_chain(sim, intra_sim, oracle, hiplib):
    """the alternating clip under --gop 0 --ref 3 through the simulated chain: pictures with lists of one, two and three entries for launches that are compared with
    each other"""
    return rc.sim_chain(sim, intra_sim, oracle, hiplib, rc.case_named("alt-gop0-ref3"))


# ---------------------------------------------------------------------------------------------------- 1. the chain against the reference encoder
@pytest.mark.parametrize("name", rc.names())
def test_simulated_chain_equals_the_reference_encoder(sim, intra_sim, oracle, hiplib, gold, in_range, name):
    """I picture through the simulation of the all-intra pass, loop filters by the oracle, P pictures through kvz_hostsim_inter_pass_refs from the pool of the
    chain's own earlier pictures, the oracle's loop filters of a P slice, the coder with the lists == kvazaar --no-bipred --ref N: every final picture, the slice
    data of every P picture.  No record carries a reference index outside its picture's list"""
    counts = {}
    chain = rc.sim_chain(sim, intra_sim, oracle, hiplib, rc.case_named(name), counts)
    rc.assert_chain_equals_fixture(chain, gold[name], name)
    assert chain["lists"] == gold[name]["lists"] and counts["ref_idx_outside_list"] == 0, counts
    for k, cu in enumerate(chain["cu"][1:], 1):
        inter = cu["type"] == 2
        assert (cu["mv_dir"][inter] == 1).all() and (cu["mv_ref"][inter][:, 0] < len(chain["lists"][k])).all(), k


def test_fixture_covers_what_it_is_there_for(gold):
    """the generator's census reaches every event as often as asked; lists of one, two, three and four entries occur; both GOP shapes and --gop 0; the MV constraint;
    P pictures on both sides of fast-residual-cost 28; every encode differs from its --ref 1 twin (asserted by the generator, which recorded both sizes)"""
    assert all(gold["census"][k] >= least for k, least in rc.CENSUS_MIN.items()), gold["census"]
    assert gold["census"]["ref_idx_outside_list"] == 0
    assert {len(l) for name in rc.names() for l in gold[name]["lists"][1:]} == {1, 2, 3, 4}
    assert {gold[name]["gop"] for name in rc.names()} == {"0", "lp-g4d3t1", "lp-g8d4t1"} and {gold[name]["ref"] for name in rc.names()} == {2, 3, 4}
    assert not any(gold[name]["gop"] == "lp-g4d3t1" and gold[name]["ref"] == 4 for name in rc.names())  # (kvazaar's fixed lowdelay4 table: another matter)
    p_qps = [q for name in rc.names() for q in gold[name]["qps"][1:]]
    assert min(p_qps) < 28 <= max(p_qps) and min(p_qps) <= 3 and max(p_qps) == 51
    assert {c[1][8] for c in rc.CASES} == {0, 2}
    assert all(gold[name]["ref1_encode"]["bytes"] > 0 for name in rc.names())


# ---------------------------------------------------------------------------------------------------- 2. no lists, and lists of one
def test_null_and_lists_of_one_are_the_slices_twin(sim, oracle, alt_chain, in_range):
    """refs == NULL: kvz_hostsim_inter_pass_refs IS kvz_hostsim_inter_pass_slices; a list of one entry over a pool of one frame per picture gives the same pictures,
    records and levels byte for byte, and the coder the same slice data -- for two pictures of different QPs in one launch"""
    from kvazaar_amd.inter import InterPictureParams
    clip = rc.case_named("alt-gop0-ref3")[1]
    name, w, h, n, *_ = clip
    frames = rc.case_frames(clip)
    ks, qps = (1, 2), (27, 33)  # (their reference pictures -- the I picture, and picture 1 with its list of one -- hold no reference index above 0)
    pics = [dict(src=frames[k], ref=alt_chain["final"][k - 1], ref_cu=alt_chain["cu"][k - 1]) for k in ks]
    table = InterPictureParams(qps, ks)
    want = pc.sim_pass(sim, pics, pc.params_of(clip, 40, 9), table, w, h, pc.P)
    assert want[0] == 0
    pool_frames, pool_cus = [p["ref"] for p in pics], [p["ref_cu"] for p in pics]
    null = rc.sim_pass(sim, [p["src"] for p in pics], pool_frames, pool_cus, pc.params_of(clip, 40, 9), table, None, w, h)
    ones = rc.references_of([(0, []), (1, [0])], [[0], [1]])
    got = rc.sim_pass(sim, [p["src"] for p in pics], pool_frames, pool_cus, pc.params_of(clip, 40, 9), table, ones, w, h)
    for other in (null, got):
        assert other[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(want[1:], other[1:]))
    ref_cu = np.stack(pool_cus)
    data = pc.sim_slice_data(sim, pc.P, w, h, table.qps, table.pocs, want[2], ref_cu, want[3], None, None)
    assert rc.sim_slice_data(sim, w, h, table.qps, table.pocs, want[2], pool_cus, want[3], None, None, None) == data
    assert rc.sim_slice_data(sim, w, h, table.qps, table.pocs, want[2], pool_cus, want[3], None, None, ones) == data


# ---------------------------------------------------------------------------------------------------- 3. pictures with lists of different lengths share a launch
def test_pictures_with_different_lists_and_qps_share_a_launch(sim, alt_chain, in_range):
    """pictures with lists of one, two and three entries at different QPs and POCs over ONE pool: every picture of the one launch, and of the one coder call, is what
    a launch of its own over a pool of just its list's frames makes of it"""
    from kvazaar_amd.inter import InterPictureParams
    clip = rc.case_named("alt-gop0-ref3")[1]
    name, w, h, n, *_ = clip
    frames = rc.case_frames(clip)
    ks, qps = (3, 1, 2), (22, 33, 27)
    pool_pocs = [2, 0, 1]  # (not in POC order: the lists name frames by pool index)
    pool = [(p, alt_chain["lists"][p]) for p in pool_pocs]
    lists = [[pool_pocs.index(p) for p in alt_chain["lists"][k]] for k in ks]
    assert [len(l) for l in lists] == [3, 1, 2]
    table, refs = InterPictureParams(qps, ks), rc.references_of(pool, lists)
    pool_frames, pool_cus = [alt_chain["final"][p] for p in pool_pocs], [alt_chain["cu"][p] for p in pool_pocs]
    joint = rc.sim_pass(sim, [frames[k] for k in ks], pool_frames, pool_cus, pc.params_of(clip, 40, 9), table, refs, w, h)
    assert joint[0] == 0
    data, sizes = rc.sim_slice_data(sim, w, h, table.qps, table.pocs, joint[2], pool_cus, joint[3], None, None, refs)
    rows, at = (h + 63) // 64, 0
    for i, (k, q) in enumerate(zip(ks, qps)):
        own_pocs = alt_chain["lists"][k]
        own_refs = rc.references_of([(p, alt_chain["lists"][p]) for p in own_pocs], [list(range(len(own_pocs)))])
        own_frames, own_cus = [alt_chain["final"][p] for p in own_pocs], [alt_chain["cu"][p] for p in own_pocs]
        alone = rc.sim_pass(sim, [frames[k]], own_frames, own_cus, pc.params_of(clip, q, k), InterPictureParams([q], [k]), own_refs, w, h)
        assert alone[0] == 0 and all(x[i].tobytes() == y[0].tobytes() for x, y in zip(joint[1:], alone[1:])), k
        own, own_sizes = rc.sim_slice_data(sim, w, h, [q], [k], alone[2], own_cus, alone[3], None, None, own_refs)
        assert sizes[i * rows:(i + 1) * rows] == own_sizes and data[at:at + len(own)] == own, k
        at += len(own)
    assert at == len(data)
    assert (joint[2][0]["mv_ref"][joint[2][0]["type"] == 2][:, 0] > 0).any()  # (the launch did use a second entry)


# ---------------------------------------------------------------------------------------------------- 4. what is refused
def _tables():
    """a valid launch of two pictures (POCs 3 and 2) over a pool of three frames, and the ways it can be wrong"""
    pool = [(2, [1, 0]), (1, [0]), (0, [])]
    return pool, [[0, 1, 2], [1, 2]]


def test_refusals(sim, capfd):
    """the twins of the three entry points' checks, each -1 with a message that names the entry point and the reason: an unknown struct_size, another n_pictures, a
    list length outside 1..4, a frame outside the pool, two entries of one POC, a reference POC not below the picture's, lists without `pictures`, lists with a
    slice type other than P, lists with tiles or a non-zero me_* member; a valid table passes without a word, and so does no table at all"""
    from kvazaar_amd.inter import InterPictureParams
    clip = pc.clip_named("pan11")
    pool, lists = _tables()
    table = InterPictureParams([27, 30], [3, 2])

    def prm(**kw):
        p = pc.params_of(clip, 27, 1)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def refs(pool=pool, lists=lists, **kw):
        r = rc.references_of(pool, lists)
        for k, v in kw.items():
            setattr(r.struct, k, v)
        return r

    entry = {"pass": "kvz_hip_dev_inter_ctu_pass_refs", "loop_filters": "kvz_hip_dev_loop_filters_inter_refs", "coder": "kvz_hip_dev_entropy_code_inter_refs"}
    five = refs()
    five.n_refs[0] = 5
    none = refs()
    none.n_refs[1] = 0
    capfd.readouterr()
    for stage in ("pass", "loop_filters", "coder"):
        bad = [(refs(struct_size=40), pc.P, table, {}, "struct_size 40 is not this library's"), (refs(n_pictures=3), pc.P, table, {}, "n_pictures 3 is not the call's 2"),
               (five, pc.P, table, {}, "a list of 5 references"), (none, pc.P, table, {}, "a list of 0 references"),
               (refs(lists=[[0, 1, 3], [1, 2]]), pc.P, table, {}, "frame 3 is outside the pool of 3"), (refs(lists=[[0, -1], [1, 2]]), pc.P, table, {}, "frame -1 is outside the pool"),
               (refs(pool=[(2, [1, 0]), (1, [0]), (1, [0])], lists=[[0, 1, 2], [1]]), pc.P, table, {}, "both have POC 1"),
               (refs(n_frames=0), pc.P, table, {}, "the pool is empty"), (refs(frame_poc=None), pc.P, table, {}, "is NULL"),
               (refs(), pc.B, table, {}, "KVZ_HIP_SLICE_P only"), (refs(), pc.I, table, {}, "slice type")]
        if stage != "loop_filters":  # (the filters take a QP array where the others take the table, and read no POC)
            bad += [(refs(lists=[[0, 1, 2], [0, 1]]), pc.P, table, {}, "not below the picture's"), (refs(), pc.P, None, {}, "need `pictures`")]
        if stage == "pass":
            bad += [(refs(), pc.P, table, dict(ref_width=136, ref_height=72), "together with tiles"), (refs(), pc.P, table, dict(has_tile_xy=True), "together with tiles"),
                    (refs(), pc.P, table, dict(me_algorithm=1), "together with me_algorithm"), (refs(), pc.P, table, dict(me_max_steps=3), "together with me_algorithm")]
        for r, slice_type, pictures, kw, message in bad:
            has_tile_xy = kw.pop("has_tile_xy", False) if "has_tile_xy" in kw else False
            assert rc.refs_check(sim, prm(**kw), slice_type, stage, 2, pictures, r, has_tile_xy=has_tile_xy) == -1, (stage, message)
            err = capfd.readouterr().err
            assert message in err and ("kvz_hip_dev_" in err), (stage, message, err)
            assert entry[stage] in err or entry[stage].replace("_refs", "_slices") in err, (stage, message, err)
        assert rc.refs_check(sim, prm(), pc.P, stage, 2, table, refs()) == 0 and rc.refs_check(sim, prm(), pc.P, stage, 2, table, None) == 0
        assert rc.refs_check(sim, prm(), pc.B, stage, 2, table, None) == 0
        assert capfd.readouterr().err == ""


def test_a_refused_launch_computes_nothing(sim, alt_chain, capfd):
    """a refusal of the pass's twin returns -1 and leaves nothing computed (its outputs stay zero); the coder's twin returns nothing"""
    from kvazaar_amd.inter import InterPictureParams
    clip = rc.case_named("alt-gop0-ref3")[1]
    name, w, h, n, *_ = clip
    frames = rc.case_frames(clip)
    pool_frames, pool_cus = [alt_chain["final"][p] for p in (1, 0)], [alt_chain["cu"][p] for p in (1, 0)]
    for pool, lists, pocs in (([(1, [0]), (0, [])], [[0, 2]], [2]), ([(1, [0]), (0, [])], [[0, 1]], [1]), ([(1, [0]), (1, [0])], [[0, 1]], [2])):
        bad = rc.references_of(pool, lists)
        rc_, rec, cu, coeff = rc.sim_pass(sim, [frames[2]], pool_frames, pool_cus, pc.params_of(clip, 27, 2), InterPictureParams([27], pocs), bad, w, h)
        assert rc_ == -1 and not rec.any() and not coeff.any() and not cu["type"].any()
        assert "kvz_hip_dev_inter_ctu_pass_refs" in capfd.readouterr().err
        assert rc.sim_slice_data(sim, w, h, [27], pocs, alt_chain["cu"][2], pool_cus, alt_chain["coeff"][2], None, None, bad) is None
        assert "kvz_hip_dev_entropy_code_inter_refs" in capfd.readouterr().err


# ---------------------------------------------------------------------------------------------------- 5. the scaling, the contexts, the lists
def _clip(lo, hi, v):
    return max(lo, min(hi, v))


def _c_div(a, b):
    """C's integer division: towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _scaled(mv, tb, td):
    """inter.c:1078-1103 in plain Python: apply_mv_scaling_pocs on one component, get_scaled_mv"""
    if tb == td:
        return mv
    tb, td = _clip(-128, 127, tb), _clip(-128, 127, td)
    scale = _clip(-4096, 4095, (tb * _c_div(0x4000 + (abs(td) >> 1), td) + 32) >> 6)
    scaled = scale * mv
    return _clip(-32768, 32767, (scaled + 127 + (1 if scaled < 0 else 0)) >> 8)


def test_mv_scaling_is_the_references_over_every_pair_of_distances(sim):
    """kvz_inter_refs.hpp's scale of (tb, td) and its multiply against a plain-Python statement of inter.c:1078-1103: every tb, td in -128 .. 127 (td != 0) and
    beyond the clips, vectors at the ends of int16 and around zero; equal distances and the scale 256 leave every vector as it is"""
    of, one, packed = sim.kvz_hostsim_mv_scale_of_distances, sim.kvz_hostsim_mv_scale, sim.kvz_hostsim_mv_scale_packed
    of.restype, one.restype, packed.restype = C.c_int, C.c_int, C.c_uint
    of.argtypes, one.argtypes, packed.argtypes = [C.c_int, C.c_int], [C.c_int, C.c_int], [C.c_uint, C.c_int]
    vectors = (-32768, -32767, -4097, -129, -3, -2, -1, 0, 1, 2, 3, 128, 4096, 32766, 32767)
    distances = list(range(-128, 128)) + [-1000, -129, 128, 500]
    for tb in distances:
        for td in distances:
            if td == 0:
                continue
            scale = of(tb, td)
            assert -4096 <= scale <= 4095
            for mv in vectors:
                assert one(mv, scale) == _scaled(mv, tb, td), (tb, td, mv, scale)
    assert all(of(d, d) == 256 and of(d, 0) == 256 for d in distances)
    for mv in range(-32768, 32768, 97):
        assert one(mv, 256) == mv
    assert packed((0x8000 << 16) | 0x7fff, 512) == (0x8000 << 16) | 0x7fff  # both components at the clips
    assert packed((0xfffd << 16) | 0x0005, 128) == ((_scaled(-3, 1, 2) & 0xffff) << 16) | _scaled(5, 1, 2)
    # the record of a picture: POC 6 with the list 5, 4, 2; frame 5 referred to 4 and 3, frame 4 to 3, frame 2 to 1 and 0
    refs = rc.references_of([(5, [4, 3]), (4, [3]), (2, [1, 0])], [[0, 1, 2]])
    rec = np.zeros(116, np.uint8)
    f = sim.kvz_hostsim_inter_refs_record
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    f(refs.ptr, 0, 6, rec.ctypes.data)
    assert rec[:20].view(np.int32).tolist() == [3, 0, 1, 2, 0]
    spatial, temporal, start = (rec[20 + 32 * i:52 + 32 * i].view(np.int16).reshape(4, 4) for i in range(3))
    dist = [1, 2, 4]
    for r in range(3):
        assert [int(v) for v in spatial[r][:3]] == [of(dist[r], dist[c]) for c in range(3)]
        assert [int(v) for v in temporal[r][:2]] == [of(dist[r], 1), of(dist[r], 2)]  # the co-located picture is frame 5: its vectors span 1 and 2
    assert [int(v) for v in start[1][:1]] == [of(2, 1)] and [int(v) for v in start[2][:2]] == [of(4, 1), of(4, 2)]
    assert (spatial[3] == 256).all() and (temporal[3] == 256).all() and (start[3] == 256).all()


def _ctx_state(qp, init_value):
    """H.265 9.3.2.2 (9-4 .. 9-6): the state of a context from its initValue at SliceQpY, as kvazaar packs it (state << 1 | MPS)"""
    slope, offset = (init_value >> 4) * 5 - 45, ((init_value & 15) << 3) - 16
    st = _clip(1, 126, ((slope * _clip(0, 51, qp)) >> 4) + offset)
    return ((st - 64) << 1) + 1 if st >= 64 else (63 - st) << 1


def test_ref_idx_contexts_come_from_the_standard(sim):
    """ref_idx_l0's two contexts start from initValue 153, 153 (H.265 Table 9-17, initType 1) at every QP, in the coder's set (KVZ_EB_CX_REF_IDX = 166, 167) and in the
    search's (IX_REF_IDX = 25, 26); without lists both sets are byte for byte what they were, and nothing else of them moves with lists"""
    with_refs, search = sim.kvz_hostsim_slice_contexts_refs, sim.kvz_hostsim_search_contexts_refs
    with_refs.restype = search.restype = None
    with_refs.argtypes, search.argtypes = [C.c_int, C.c_int, C.c_void_p], [C.c_int, C.c_int, C.c_int, C.c_void_p]
    for qp in range(52):
        plain, refs = pc.slice_contexts(sim, pc.P, qp), np.zeros(176, np.uint8)
        with_refs(pc.P, qp, refs.ctypes.data)
        assert [int(v) for v in refs[166:168]] == [_ctx_state(qp, 153)] * 2 and np.array_equal(refs[:166], plain[:166]), qp
        assert [int(v) for v in plain[166:168]] == [_ctx_state(qp, 154)] * 2, qp
        a, b = np.zeros(168, np.uint8), np.zeros(168, np.uint8)
        search(pc.P, qp, 0, a.ctypes.data)
        search(pc.P, qp, 1, b.ctypes.data)
        assert [int(v) for v in b[25:27]] == [_ctx_state(qp, 153)] * 2 and [int(v) for v in a[25:27]] == [_ctx_state(qp, 154)] * 2, qp
        assert np.array_equal(np.delete(a, [25, 26]), np.delete(b, [25, 26])), qp


def test_reference_lists_of_the_gop_are_cfg_c():
    """kvazaar_amd.inter.reference_pocs against lists typed in from reading cfg.c:1468-1507 (the previous picture, then the previous key pictures) and
    encoderstate.c:1040-1182 (the decoded picture buffer keeps what the current picture asks for; L0 by descending POC) for g4 and g8, and --gop 0"""
    from kvazaar_amd import inter
    # the distances a picture of the GOP asks for: g = 1 .. gop_len
    assert [inter.lowdelay_ref_distances(g, 2, 4) for g in (1, 2, 3, 4)] == [[1, 5], [1, 2], [1, 3], [1, 4]]
    assert [inter.lowdelay_ref_distances(g, 3, 4) for g in (1, 2, 3, 4)] == [[1, 5, 9], [1, 2, 6], [1, 3, 7], [1, 4, 8]]
    assert [inter.lowdelay_ref_distances(g, 4, 8) for g in (1, 2, 3, 8)] == [[1, 9, 17, 25], [1, 2, 10, 18], [1, 3, 11, 19], [1, 8, 16, 24]]
    # lp-g4d3t1 --ref 2: the previous picture and the last key picture (POC 0, 4, 8)
    assert [inter.reference_pocs(p, 2, "lp-g4d3t1") for p in range(1, 11)] == [[0], [1, 0], [2, 0], [3, 0], [4, 0], [5, 4], [6, 4], [7, 4], [8, 4], [9, 8]]
    # --ref 3: the key picture before that as well, once the buffer has kept it
    assert [inter.reference_pocs(p, 3, "lp-g4d3t1") for p in range(1, 11)] == [[0], [1, 0], [2, 0], [3, 0], [4, 0], [5, 4, 0], [6, 4, 0], [7, 4, 0], [8, 4, 0], [9, 8, 4]]
    # lp-g8d4t1 --ref 4: key pictures at 0, 8, 16; four entries only once three key pictures exist
    assert [inter.reference_pocs(p, 4, "lp-g8d4t1") for p in (1, 2, 5, 8, 9, 10, 16, 17, 18)] == [[0], [1, 0], [4, 0], [7, 0], [8, 0], [9, 8, 0], [15, 8, 0], [16, 8, 0], [17, 16, 8, 0]]
    # --gop 0: the previous N pictures, as far as they exist
    assert [inter.reference_pocs(p, 3, "0") for p in range(0, 6)] == [[], [0], [1, 0], [2, 1, 0], [3, 2, 1], [4, 3, 2]]
    assert inter.reference_pocs(7, 1, "0") == [6] and inter.reference_pocs(7, 1, "lp-g4d3t1") == [6]
    with pytest.raises(ValueError):
        inter.reference_pocs(3, 2, "8")


# ---------------------------------------------------------------------------------------------------- 6. the interface as a text
def test_header_library_binding_and_build_list_agree(hiplib):
    """the headers declare the struct and the three entry points, the library exports them, the binding's struct is the header's, and the build has the two units
    behind kvz_inter_tu9"""
    from kvazaar_amd import build, inter
    dev = open(os.path.join(flatapi.ROOT, "include", "kvz_hip_dev.h")).read()
    types = open(os.path.join(flatapi.ROOT, "include", "kvz_hip_types.h")).read()
    for name, ret in (("kvz_hip_dev_inter_ctu_pass_refs", "int"), ("kvz_hip_dev_loop_filters_inter_refs", "int"), ("kvz_hip_dev_entropy_code_inter_refs", "long")):
        decl = re.search(ret + r"\s+" + name + r"\(([^;]*)\);", dev)
        assert decl and decl.group(1).rstrip().endswith("const kvz_hip_inter_refs *refs"), name
        twin = re.search(ret + r"\s+" + name.replace("_refs", "_slices") + r"\(([^;]*)\);", dev)
        assert re.sub(r"\s+", " ", decl.group(1)).startswith(re.sub(r"\s+", " ", twin.group(1))), name  # the twin's arguments, then refs
        assert hasattr(hiplib, name), name
    struct = re.search(r"typedef struct kvz_hip_inter_refs \{(.*?)\} kvz_hip_inter_refs;", types, re.S).group(1)
    fields = re.findall(r"^\s*(?:const )?(?:uint32_t|int32_t)\s+\*?(\w+);", struct, re.M)
    assert fields == [n for n, _ in inter.InterRefsStruct._fields_] == ["struct_size", "n_pictures", "n_frames", "frame_poc", "frame_ref_poc", "n_refs", "ref_frame"]
    assert C.sizeof(inter.InterRefsStruct) == 48 and inter.MAX_REFS == 4 and "#define KVZ_HIP_MAX_REFS 4" in types
    units = [name for name, _, _ in build.UNITS]
    defs = {name: d for name, _, d in build.UNITS}
    assert units[units.index("kvz_inter_tu9") + 1:units.index("kvz_inter_tu9") + 3] == ["kvz_inter_tu10", "kvz_inter_tu11"]
    assert defs["kvz_inter_tu10"] == ["-DKVZ_ICTU_P=1", "-DKVZ_ICTU_REFS=1", "-DKVZ_ICTU_CABAC=0"] and defs["kvz_inter_tu11"] == ["-DKVZ_ICTU_P=1", "-DKVZ_ICTU_REFS=1", "-DKVZ_ICTU_CABAC=1"]
    kernels = open(os.path.join(flatapi.ROOT, "kvazaar_amd", "csrc", "kvz_inter_kernels.hpp")).read()
    builds = open(os.path.join(flatapi.ROOT, "kvazaar_amd", "csrc", "kvz_inter_builds.hpp")).read()  # the kernels' names: inter_ctu_ticket_kernel_ and the suffix of a row of the list
    assert "KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_##suffix);" in kernels and re.search(r"\bX\(10, refs_fast, ", builds) and re.search(r"\bX\(11, refs_cabac, ", builds)
    assert re.search(r"#if KVZ_ICTU_REFS && !KVZ_ICTU_P\n#error", kernels)
