"""The builds of the inter CTU pass and the rule that picks one for a launch (kvazaar_amd/csrc/kvz_inter_builds.hpp) -- through the host simulation, which compiles the
text the library compiles.  What the launch path did before it asked that function is written out here: the twelve kernels with their translation units and switches,
and the ladder of `?:` in its order of precedence."""
import ctypes as C
import itertools

import pytest

import inter_me_common as mec
import inter_p_common as pc
import inter_refs_common as rc

# unit -> (the kernel's name behind inter_ctu_ticket_kernel_, (CABAC, LISTS, JOINT, ME, P, REFS)): the kernels as kvazaar_amd/build.py compiled them one by one
BUILDS = {
    0: ("fast", (0, 0, 0, 0, 0, 0)), 1: ("cabac", (1, 0, 0, 0, 0, 0)),
    2: ("lists_fast", (0, 1, 0, 0, 0, 0)), 3: ("lists_cabac", (1, 1, 0, 0, 0, 0)),
    4: ("joint_fast", (0, 0, 1, 0, 0, 0)), 5: ("joint_cabac", (1, 0, 1, 0, 0, 0)),
    6: ("me_fast", (0, 0, 0, 1, 0, 0)), 7: ("me_cabac", (1, 0, 0, 1, 0, 0)),
    8: ("p_fast", (0, 0, 0, 0, 1, 0)), 9: ("p_cabac", (1, 0, 0, 0, 1, 0)),
    10: ("refs_fast", (0, 0, 0, 0, 1, 1)), 11: ("refs_cabac", (1, 0, 0, 0, 1, 1)),
}
UNIT_OF = {name: unit for unit, (name, _) in BUILDS.items()}
NONE = -1


def ladder(any_cabac, lists, joint, me, p_slice, refs):
    """the kernel of a launch the entry points have accepted, as kvz_hip_dev_inter_ctu_pass_groups (joint) and kvz_inter_ctu_pass_run (refs, then P, then me, then lists,
    then plain) picked it, `_cabac` when any picture prices with the residual coder's contexts"""
    kind = "joint_" if joint else "refs_" if refs else "p_" if p_slice else "me_" if me else "lists_" if lists else ""
    return kind + ("cabac" if any_cabac else "fast")


@pytest.fixture(scope="module")
def sim():
    """every form of the inter program but the chosen searches: the twins of the checks of a slice type and of reference lists"""
    return rc.load_sim()


@pytest.fixture(scope="module")
def me_sim():
    """the twin of the check of the me_* members, with tiles, scaling lists and in a joint launch"""
    return mec.load_sim()


def _builds(sim):
    rows, mask = (C.c_int * (64 * 7))(), C.c_ulonglong(0)
    n = sim.kvz_hostsim_inter_builds(rows, C.byref(mask))
    sim.kvz_hostsim_inter_build_suffix.restype = C.c_char_p
    return [(rows[7 * i], sim.kvz_hostsim_inter_build_suffix(rows[7 * i]).decode(), tuple(rows[7 * i + 1:7 * i + 7])) for i in range(n)], mask.value


def test_the_list_is_the_twelve_kernels(sim, me_sim):
    listed, mask = _builds(sim)
    assert len(listed) == len(BUILDS) == 12 and {u: (name, sw) for u, name, sw in listed} == BUILDS  # no build twice, each on the unit it was on, under its name
    assert len({sw for _, _, sw in listed}) == 12 and mask == sum(1 << u for u in BUILDS)
    assert _builds(me_sim) == (listed, mask)  # (every inter simulation library holds the same list)
    assert sim.kvz_hostsim_inter_build_suffix(12) == b"" and sim.kvz_hostsim_inter_build_suffix(NONE) == b""


def _library_refuses(sim, me_sim, combo):
    """what the twins of the entry points' checks say of a launch of this kind: True refused, False accepted, None where no entry point takes the two together (a slice
    type or reference lists with scaling lists or groups; scaling lists with groups)"""
    from kvazaar_amd.inter import InterPictureParams
    _, lists, joint, me, p_slice, refs = combo
    prm = pc.params_of(pc.clip_named("pan11"), 27, 1)
    prm.me_algorithm = 1 if me else 0
    if p_slice or refs:  # kvz_hip_dev_inter_ctu_pass_slices / _refs: two pictures of POCs 3 and 2 over a pool of three frames
        if lists or joint:
            return None
        references = rc.references_of([(2, [1, 0]), (1, [0]), (0, [])], [[0, 1, 2], [1, 2]]) if refs else None
        return rc.refs_check(sim, prm, pc.P if p_slice else pc.B, "pass", 2, InterPictureParams([27, 30], [3, 2]), references) == -1
    if lists and joint:
        return None
    return mec.me_check(me_sim, prm, n_sets=lists, joint=bool(joint)) == -1  # kvz_hip_dev_inter_ctu_pass[_lists] / _groups


def test_the_choice_is_the_ladder_and_none_is_what_the_checks_refuse(sim, me_sim, capfd):
    """all 64 combinations of what a launch knows"""
    chosen, refused, asked = set(), 0, 0
    for combo in itertools.product((0, 1), repeat=6):
        any_cabac, lists, joint, me, p_slice, refs = combo
        got = sim.kvz_hostsim_inter_build_choose(*combo)
        one_kind = lists + joint + me + (p_slice or refs) <= 1 and (p_slice or not refs)  # "refs" is P and REFS together
        assert (got != NONE) == bool(one_kind), combo
        verdict = _library_refuses(sim, me_sim, combo)
        if verdict is not None:
            asked += 1
            assert verdict == (got == NONE), combo  # the library refuses exactly where no build serves
        if got != NONE:
            assert verdict is False and got == UNIT_OF[ladder(*combo)] and BUILDS[got][1] == combo, combo
            chosen.add(got)
        else:
            refused += 1
    assert chosen == set(BUILDS) and refused == 52  # no build that nothing launches
    assert asked == 24  # P / refs x me x CABAC, and plain / lists / groups x me x CABAC
    err = capfd.readouterr().err  # the checks say why; the choice is silent
    assert "P pictures are not covered together with me_algorithm" in err and "KVZ_HIP_SLICE_P only" in err and "scaling lists" in err and "a joint launch" in err


def test_the_choice_never_prints(sim, capfd):
    capfd.readouterr()
    for combo in itertools.product((0, 1), repeat=6):
        sim.kvz_hostsim_inter_build_choose(*combo)
    out = capfd.readouterr()
    assert out.out == "" and out.err == ""


def test_build_py_compiles_the_units_of_the_list(sim):
    import kvazaar_amd.build as build
    listed, mask = _builds(sim)
    named = {int(name[len("kvz_inter_tu"):]): (src, defs) for name, src, defs in build.UNITS if name.startswith("kvz_inter_tu")}
    assert sorted(named) == sorted(u for u, _, _ in listed) == list(range(12))
    for unit, (src, defs) in named.items():  # a switch that is 1 by its name, in the list's order, then CABAC with its value
        _, (cabac, *others) = BUILDS[unit]
        assert src == "kvz_inter_tu.hip" and defs == [f"-DKVZ_ICTU_{n}=1" for n, v in zip(("LISTS", "JOINT", "ME", "P", "REFS"), others) if v] + [f"-DKVZ_ICTU_CABAC={cabac}"], unit
    main = [defs for name, _, defs in build.UNITS if name == "kvz_hip"]
    assert len(main) == 1 and f"-DKVZ_ICTU_UNITS_BUILT={mask}ull" in main[0]  # the header refuses another set of units when the library's main unit compiles
