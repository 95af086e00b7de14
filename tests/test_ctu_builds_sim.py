"""The builds of the all-intra CTU pass and the rule that picks one for a launch (kvazaar_amd/csrc/kvz_ctu_builds.hpp), the ticket lists of a batch on its own and the
hand-off error tag (kvz_joint.hpp) -- through the host simulation, which compiles the text the library compiles.  What the launch path did before it asked these
functions is written out here: the ladder of `if`s in its order of precedence, the two lists of kvz_hip_batch_create item by item, the masks of the tag."""
import ctypes as C
import itertools

import pytest

import joint_common as jc

# (CABAC, S32, RDOQ, SH, LISTS, JOINT) -> translation unit: the kernels as kvz_ctu_tu.hip instantiated them one by one
UNIT_OF = {
    (0, 0, 0, 0, 0, 0): 0, (1, 0, 0, 0, 0, 0): 1, (0, 1, 0, 0, 0, 0): 3, (1, 1, 0, 0, 0, 0): 4,  # intra_ctu_ticket_kernel<CABAC, S32>
    (1, 1, 1, 0, 0, 0): 5,                                                                      # intra_ctu_ticket_kernel_rdoq
    (1, 0, 0, 1, 0, 0): 6, (1, 1, 0, 1, 0, 0): 7,                                                # intra_ctu_ticket_kernel_signhide<S32>
    (0, 0, 0, 0, 1, 0): 8, (1, 0, 0, 0, 1, 0): 9, (0, 1, 0, 0, 1, 0): 10, (1, 1, 0, 0, 1, 0): 11,  # intra_ctu_ticket_kernel_lists<CABAC, S32>
    (0, 0, 0, 0, 0, 1): 12, (1, 0, 0, 0, 0, 1): 13, (0, 1, 0, 0, 0, 1): 14, (1, 1, 0, 0, 0, 1): 15,  # intra_ctu_joint_kernel<CABAC, S32, false>
    (1, 0, 0, 1, 0, 1): 16, (1, 1, 0, 1, 0, 1): 17,                                              # intra_ctu_joint_kernel<true, S32, true>
}
NONE = -1


def ladder(s32, rdoq, nxn, any_cabac, any_signhide, lists, joint):
    """the build of a launch the entry points have accepted, as kvz_intra_frames_queue and kvz_hip_batch_group_intra_frames picked it: lists, then rdoq / nxn, then
    sign hiding, then 32x32, then CABAC; the joint variants likewise"""
    if joint:
        if any_signhide:
            return (1, 1, 0, 1, 0, 1) if s32 else (1, 0, 0, 1, 0, 1)
        if s32:
            return (1, 1, 0, 0, 0, 1) if any_cabac else (0, 1, 0, 0, 0, 1)
        return (1, 0, 0, 0, 0, 1) if any_cabac else (0, 0, 0, 0, 0, 1)
    if lists:
        if s32:
            return (1, 1, 0, 0, 1, 0) if any_cabac else (0, 1, 0, 0, 1, 0)
        return (1, 0, 0, 0, 1, 0) if any_cabac else (0, 0, 0, 0, 1, 0)
    if rdoq or nxn:
        return (1, 1, 1, 0, 0, 0)
    if any_signhide:
        return (1, 1, 0, 1, 0, 0) if s32 else (1, 0, 0, 1, 0, 0)
    if s32:
        return (1, 1, 0, 0, 0, 0) if any_cabac else (0, 1, 0, 0, 0, 0)
    return (1, 0, 0, 0, 0, 0) if any_cabac else (0, 0, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def sim():
    return jc.load_sim()


@pytest.fixture(scope="module")
def hiplib():
    """libkvz_hip.so for its host-side functions only (the cost model of a QP): nothing here touches a device"""
    import kvazaar_amd
    return C.CDLL(kvazaar_amd.build_library())


def _builds(sim):
    rows, mask = (C.c_int * (64 * 7))(), C.c_ulonglong(0)
    n = sim.kvz_hostsim_ctu_builds(rows, C.byref(mask))
    return {tuple(rows[7 * i + 1:7 * i + 7]): rows[7 * i] for i in range(n)}, n, mask.value


def test_the_choice_is_the_ladder_and_none_is_what_the_checks_refuse(sim, hiplib, capfd):
    """all 128 combinations of what a launch knows"""
    listed, n, _ = _builds(sim)
    assert listed == UNIT_OF and n == len(UNIT_OF) == 17  # no build twice, each on the unit it was on (eighteen units: unit 2 holds the older schedule's kernel alone)
    check = sim.kvz_hostsim_ctu_launch_check
    check.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    chosen, refused = set(), 0
    for combo in itertools.product((0, 1), repeat=7):
        s32, rdoq, nxn, any_cabac, any_signhide, lists, joint = combo
        got = sim.kvz_hostsim_ctu_build_choose(*combo)
        # an equivalent launch: a table of two pictures, the second of which prices with CABAC / hides signs when any does
        pm = jc.table(hiplib, [22, 27], search_32x32=s32, rdoq=rdoq, search_nxn=nxn, signhide=[0, any_signhide])
        pm.models[1].coeff_cabac = any_cabac
        accepted = check(C.addressof(pm.struct), 2, lists, joint) == 0
        assert (got != NONE) == accepted, combo
        if accepted:
            assert got == UNIT_OF[ladder(*combo)], combo
            chosen.add(got)
        else:
            refused += 1
    assert chosen == set(UNIT_OF.values())  # no build that nothing launches
    assert refused == 128 - (20 + 4 + 8)  # launches: 32 plain ones less the 12 that hide signs under rdoq / nxn; s32 x CABAC with lists; s32 x CABAC x sign hiding of a group
    assert "kvz_hostsim_ctu_launch_check" in capfd.readouterr().err  # the checks say why; the choice is silent


def test_the_choice_never_prints(sim, capfd):
    capfd.readouterr()
    for combo in itertools.product((0, 1), repeat=7):
        sim.kvz_hostsim_ctu_build_choose(*combo)
    out = capfd.readouterr()
    assert out.out == "" and out.err == ""


def test_build_py_compiles_the_units_of_the_list(sim):
    import kvazaar_amd.build as build
    listed, _, mask = _builds(sim)
    named = {int(name[len("kvz_ctu_tu"):]): defs for name, _, defs in build.UNITS if name.startswith("kvz_ctu_tu")}
    assert sorted(named) == sorted(set(listed.values()) | {0, 2}) and mask == sum(1 << k for k in named)  # (0 and 2: the units of the older schedule's two kernels)
    for k, defs in named.items():
        assert f"-DKVZ_CTU_KERNEL_TU={k}" in defs and f"-DKVZ_CTU_UNITS_BUILT={mask}ull" in defs  # the header refuses another set of units when it compiles


# (CTUs across, CTUs down, pictures) -> (the list with WPP, the list without), as kvz_hip_batch_create built them: picture << 16 | y << 8 | x, anti-diagonal x + 2y by
# anti-diagonal (every picture's CTUs of it, rows ascending) / CTU by CTU in raster order, every picture's
BATCH_LISTS = {
    (1, 1, 1): ([0x00000],
                [0x00000]),
    (1, 1, 3): ([0x00000, 0x10000, 0x20000],
                [0x00000, 0x10000, 0x20000]),
    (3, 1, 1): ([0x00000, 0x00001, 0x00002],
                [0x00000, 0x00001, 0x00002]),
    (3, 1, 3): ([0x00000, 0x10000, 0x20000, 0x00001, 0x10001, 0x20001, 0x00002, 0x10002, 0x20002],
                [0x00000, 0x10000, 0x20000, 0x00001, 0x10001, 0x20001, 0x00002, 0x10002, 0x20002]),
    (1, 3, 1): ([0x00000, 0x00100, 0x00200],
                [0x00000, 0x00100, 0x00200]),
    (1, 3, 3): ([0x00000, 0x10000, 0x20000, 0x00100, 0x10100, 0x20100, 0x00200, 0x10200, 0x20200],
                [0x00000, 0x10000, 0x20000, 0x00100, 0x10100, 0x20100, 0x00200, 0x10200, 0x20200]),
    (3, 2, 1): ([0x00000, 0x00001, 0x00002, 0x00100, 0x00101, 0x00102],
                [0x00000, 0x00001, 0x00002, 0x00100, 0x00101, 0x00102]),
    (3, 2, 3): ([0x00000, 0x10000, 0x20000, 0x00001, 0x10001, 0x20001, 0x00002, 0x00100, 0x10002, 0x10100, 0x20002, 0x20100, 0x00101, 0x10101, 0x20101, 0x00102, 0x10102, 0x20102],
                [0x00000, 0x10000, 0x20000, 0x00001, 0x10001, 0x20001, 0x00002, 0x10002, 0x20002, 0x00100, 0x10100, 0x20100, 0x00101, 0x10101, 0x20101, 0x00102, 0x10102, 0x20102]),
}


@pytest.mark.parametrize("shape", list(BATCH_LISTS), ids=lambda s: "x".join(str(v) for v in s))
def test_a_group_of_one_gets_the_lists_of_a_batch(sim, shape):
    wc, hc, n_frames = shape
    wpp, raster, pictures = jc.sim_lists(sim, [(wc * 64 - 8, hc * 64 - 8, n_frames)])  # (partial CTUs at the right and the bottom)
    assert ([int(v) for v in wpp], [int(v) for v in raster]) == BATCH_LISTS[shape]
    assert [int(p) for p in pictures] == list(range(n_frames))  # batch 0: a group picture is the batch's picture


class HandoffTag(C.Structure):
    """kvz::HandoffTag (kvz_joint.hpp)"""
    _fields_ = [("x", C.c_uint), ("y", C.c_uint), ("picture", C.c_uint), ("neighbour", C.c_char_p)]


@pytest.mark.parametrize("bits,words", [(0, "its left neighbour"), (0x20000000, "its above-right neighbour"), (0x40000000, "the end of the row above")])
def test_the_hand_off_tag_round_trip(sim, bits, words):
    """what ticket_loop wrote with literal masks: kind | ((picture << 16 | y << 8 | x) & 0x1fffffff), and what both diagnostics read out of it"""
    f = sim.kvz_hostsim_handoff_tag
    f.restype = C.c_uint
    for picture, y, x in [(8191, 255, 255), (0, 0, 0), (5, 1, 3), (8192, 2, 7), (8193 + 8192, 255, 0)]:
        read = HandoffTag()
        tag = f(bits, picture, y, x, C.byref(read))
        assert tag == bits | ((picture << 16 | y << 8 | x) & 0x1fffffff)
        assert tag & 0x80000000 == 0  # bit 31 is wait_done's own
        assert (read.x, read.y, read.picture, read.neighbour.decode()) == (x, y, picture % 8192, words)


def test_the_joint_diagnostic_says_modulo_8192_for_a_picture_the_tag_cannot_hold(sim):
    f = sim.kvz_hostsim_joint_fan_out
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_char_p, C.c_size_t]
    sim.kvz_hostsim_handoff_tag.restype = C.c_uint
    tag = sim.kvz_hostsim_handoff_tag(0x40000000, 8192, 1, 0, C.byref(HandoffTag()))
    err, failed, msg = (C.c_uint * 3)(0x80000000 | tag, 0, 0), jc._ints([0, 0]), C.create_string_buffer(640)
    assert f(err, 2, jc._ints([64, 8]), jc._ints([64, 8]), jc._ints([9000, 1]), failed, msg, 640) == -1 and list(failed) == [1, 1]
    assert "(group picture 0 modulo 8192; the end of the row above)" in msg.value.decode()
