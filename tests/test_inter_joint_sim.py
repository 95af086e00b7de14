"""B pictures of different sizes in ONE launch of the inter CTU pass (kvz_hip_dev_inter_ctu_pass_groups), without a GPU: the device sources compiled for the host
(tests/hostsim/hostsim_inter_joint.cpp) walk a joint launch in the launch's real ticket order with ONE program state, as a persistent workgroup does -- consecutive
CTUs belong to pictures of different sizes, QPs and POCs.  Every picture is an ordinary constant-QP picture, so its reference exists already: the oracle's encode of
its own sequence alone (tests/inter_mixed_common.py, pinned to the reference encoder).  All comparisons are exact."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import flatapi
import inter_joint_common as jc
import inter_mixed_common as mx
from kvazaar_amd.inter import InterGroupStruct, InterPictureParams

ENTRY = "kvz_hip_dev_inter_ctu_pass_groups"


@pytest.fixture(scope="module")
def sim():
    """tests/hostsim/libkvz_hostsim_inter_joint.so: hostsim.cpp and hostsim_inter_models.cpp plus the twin of the joint entry point, rebuilt when a source is newer"""
    d, csrc = os.path.join(flatapi.ROOT, "tests", "hostsim"), os.path.join(flatapi.ROOT, "kvazaar_amd", "csrc")
    so = os.path.join(d, "libkvz_hostsim_inter_joint.so")
    srcs = [os.path.join(d, f) for f in ("hostsim_inter_joint.cpp", "hostsim_inter_models.cpp", "hostsim.cpp")] + [os.path.join(flatapi.ROOT, "include", f) for f in ("kvz_hip_types.h", "kvz_hip_dev.h")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = os.path.join(d, f".libkvz_hostsim_inter_joint.{os.getpid()}.so")
        # -Bsymbolic: as tests/test_inter_mixed_qp_sim.py -- this library's copy of the program must run on its own workgroup-scope state
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wl,-Bsymbolic", "-o", tmp, os.path.join(d, "hostsim_inter_joint.cpp")])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.kvz_hostsim_mul24_violations.restype = C.c_ulonglong
    return lib


@pytest.fixture(scope="module")
def four_groups(sim):
    """the launch of the four sizes, run once and shared (never modified): (the launch, the multiply counter after it)"""
    launch = jc.HostLaunch(jc.veryfast_groups())
    sim.kvz_hostsim_mul24_reset()
    assert launch.run(sim, mx.launch_params("veryfast")) == 0
    return launch, int(sim.kvz_hostsim_mul24_violations())


def test_four_sizes_in_one_launch_equal_each_sequences_own_encode(sim, four_groups):
    """40x24, 72x40, 136x72 and 264x136 with 2, 2, 3 and 1 pictures (`veryfast`, loop-filter switches on, picture QPs on both sides of 28, POC 1, 2 and 3): reconstruction
    and CU records of every picture, the slice data of every group through the per-group coder, and no 24-bit multiply whose operand does not fit"""
    launch, violations = four_groups
    print("picture QPs", [[p["qp"] for p in g[2]] for g in launch.groups], "POCs", [[p["poc"] for p in g[2]] for g in launch.groups])
    jc.assert_groups_equal_the_oracle(launch)
    assert violations == 0
    for i, (w, h, pics) in enumerate(launch.groups):
        _, cu, coeff = launch.outputs(i)
        mx.assert_slice_data(pics, *mx.hostsim_slice_data(sim, pics, cu, coeff, w, h))


def test_no_wpp_launch_of_the_four_sizes(sim):
    """no_wpp = 1 (the raster list, the wait for the end of the row above, contexts from there) and mv_constraint = 0 over the same sizes and counts"""
    launch = jc.HostLaunch(jc.no_wpp_groups())
    sim.kvz_hostsim_mul24_reset()
    assert launch.run(sim, mx.launch_params("veryfast", no_wpp=1, mv_constraint=0)) == 0
    jc.assert_groups_equal_the_oracle(launch)
    assert int(sim.kvz_hostsim_mul24_violations()) == 0


def test_faster_launch_of_two_groups_one_without_a_coefficient_buffer(sim):
    """`faster`: every picture on the residual coder (the `_cabac` build's program), quarter-sample search; the 72x40 group has coeff == NULL"""
    groups = jc.faster_groups()
    launch = jc.HostLaunch(groups, with_coeff=[True, False])
    sim.kvz_hostsim_mul24_reset()
    assert launch.run(sim, mx.launch_params("faster")) == 0
    jc.assert_groups_equal_the_oracle(launch)
    assert int(sim.kvz_hostsim_mul24_violations()) == 0
    w, h, pics = groups[0]
    _, cu, coeff = launch.outputs(0)
    mx.assert_slice_data(pics, *mx.hostsim_slice_data(sim, pics, cu, coeff, w, h))


def test_a_launch_of_one_group_is_the_pictures_entry_point_byte_for_byte(sim):
    """rec, cu and coeff of one group against kvz_hostsim_inter_pass_pictures on the same pictures: with the group's table, and with pictures == NULL where every
    picture runs at params->qp / params->poc"""
    w, h, pics = jc.veryfast_groups()[2]
    prm = mx.launch_params("veryfast")
    launch = jc.HostLaunch(((w, h, pics),))
    assert launch.run(sim, prm) == 0
    rc, rec, cu, coeff = mx.hostsim_pass(sim, pics, prm, jc.table_of(pics), w=w, h=h)
    assert rc == 0
    got = launch.outputs(0)
    assert np.array_equal(got[0], rec) and got[1].tobytes() == cu.tobytes() and np.array_equal(got[2], coeff)
    same = (pics[1], pics[1])
    prm.qp, prm.poc = same[0]["qp"], same[0]["poc"]
    launch = jc.HostLaunch(((w, h, same),), tables=[False])
    assert launch.structs[0].pictures is None
    assert launch.run(sim, prm) == 0
    rc, rec, cu, coeff = mx.hostsim_pass(sim, same, prm, None, w=w, h=h)
    assert rc == 0
    got = launch.outputs(0)
    assert np.array_equal(got[0], rec) and got[1].tobytes() == cu.tobytes() and np.array_equal(got[2], coeff)
    mx.assert_pictures_equal_the_oracle(same, got[0], got[1])


def test_the_order_and_the_cut_of_the_groups_do_not_matter(sim, four_groups):
    """the four groups in reversed order, and the 136x72 group split into two groups of that size: every picture gets the bytes it got in the first launch"""
    first, _ = four_groups
    groups = jc.veryfast_groups()
    want = {}
    for i, (w, h, pics) in enumerate(groups):
        rec, cu, coeff = first.outputs(i)
        for k, p in enumerate(pics):
            want[id(p)] = (rec[k].tobytes(), cu[k].tobytes(), coeff[k].tobytes())
    w, h, pics = groups[2]
    split = (groups[0], (w, h, pics[:2]), groups[1], (w, h, pics[2:]), groups[3])
    for other in (tuple(reversed(groups)), split):
        launch = jc.HostLaunch(other)
        assert launch.run(sim, mx.launch_params("veryfast")) == 0
        for i, (w, h, pics) in enumerate(other):
            rec, cu, coeff = launch.outputs(i)
            for k, p in enumerate(pics):
                assert (rec[k].tobytes(), cu[k].tobytes(), coeff[k].tobytes()) == want[id(p)], (len(other), i, k)


def _tickets(sim, geometry, no_wpp):
    g = np.ascontiguousarray(geometry, np.int32).reshape(-1, 3)
    f = sim.kvz_hostsim_inter_joint_tickets
    f.restype, f.argtypes = C.c_long, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    out = np.zeros(int(sum(wc * hc * n for wc, hc, n in g)), np.uint32)
    assert f(g.ctypes.data, len(g), no_wpp, out.ctypes.data) == out.size
    return out


def test_ticket_lists_hold_every_ctu_once_behind_what_it_waits_for(sim):
    """for every set of groups drawn from the grids 1x1, 2x1, 3x2, 5x3 and 1x3 with 1 to 3 pictures each, both lists: every CTU of every picture once; a CTU's left
    neighbour and its above-right neighbour (the above one at the right edge) hold lower tickets, in the list without WPP the last CTU of the row above too; and a
    launch of one group has exactly inter_ticket_items's list"""
    grids = ((1, 1), (2, 1), (3, 2), (5, 3), (1, 3))
    one = sim.kvz_hostsim_inter_ticket_items
    one.restype, one.argtypes = C.c_long, [C.c_int] * 4 + [C.c_void_p]
    sets = 0
    for k in range(1, len(grids) + 1):
        for subset in itertools.combinations(grids, k):
            for counts in itertools.product((1, 2, 3), repeat=k):
                geometry = [(wc, hc, n) for (wc, hc), n in zip(subset, counts)]
                size_of = [(wc, hc) for wc, hc, n in geometry for _ in range(n)]
                sets += 1
                for no_wpp in (0, 1):
                    items = _tickets(sim, geometry, no_wpp)
                    at = {(int(v) >> 16, int(v) & 0xff, (int(v) >> 8) & 0xff): t for t, v in enumerate(items)}
                    assert len(at) == len(items) and set(at) == {(p, x, y) for p, (wc, hc) in enumerate(size_of) for y in range(hc) for x in range(wc)}, (geometry, no_wpp)
                    for (p, x, y), t in at.items():
                        wc, _ = size_of[p]
                        if x > 0:
                            assert at[(p, x - 1, y)] < t, (geometry, no_wpp, p, x, y)
                        if y > 0:
                            assert at[(p, min(x + 1, wc - 1), y - 1)] < t, (geometry, no_wpp, p, x, y)
                            if no_wpp:
                                assert at[(p, wc - 1, y - 1)] < t, (geometry, p, x, y)
                    if k == 1:
                        wc, hc, n = geometry[0]
                        alone = np.zeros(wc * hc * n, np.uint32)
                        assert one(wc, hc, n, no_wpp, alone.ctypes.data) == alone.size and np.array_equal(items, alone), (geometry, no_wpp)
    assert sets == 4 ** 5 - 1


def test_refusals_return_minus_one_say_why_and_touch_nothing(sim, capfd):
    """everything kvz_hip_dev_inter_ctu_pass_groups refuses, through the text it refuses with (kvz_inter_joint.hpp)"""
    groups = jc.veryfast_groups()[:2]
    fill = 0x5a

    def fresh():
        return jc.HostLaunch(groups, fill=fill), mx.launch_params("veryfast")

    def group_size(l, p): l.structs[1].struct_size = C.sizeof(InterGroupStruct) + 8
    def params_size(l, p): p.struct_size = p.struct_size - 4
    def geometry(l, p): l.structs[1].width = 68
    def too_wide(l, p): l.structs[0].width = 64 * 256
    def no_pictures(l, p): l.structs[0].n_pictures = 0
    def table(l, p):
        l.keep = InterPictureParams([22, 23, 24], [1, 1, 1])
        l.structs[1].pictures = l.keep.ptr
    def table_qp(l, p):
        l.keep = InterPictureParams([22, 52], [1, 1])
        l.structs[0].pictures = l.keep.ptr
    def no_table_bad_qp(l, p):
        l.structs[0].pictures = None
        p.qp = 52
    def same_rec(l, p): l.structs[1].rec = l.structs[0].rec
    def same_cu(l, p): l.structs[1].cu = l.structs[0].cu
    def many(l, p):
        for g in l.structs:
            g.n_pictures, g.pictures = 32768, None
        p.qp, p.poc = 30, 1
    cases = [(group_size, "group 1: kvz_hip_inter_group.struct_size"), (params_size, "kvz_hip_inter_params.struct_size"), (geometry, "group 1: bad geometry"),
             (too_wide, "group 0: bad geometry"), (no_pictures, "group 0: bad geometry"), (table, "n_pictures 3 is not the call's 2"), (table_qp, "QP 52 outside 0..51"),
             (no_table_bad_qp, "group 0 has no table and params holds QP 52"), (same_rec, "group 1 has the rec buffer of group 0"), (same_cu, "group 1 has the cu buffer of group 0"),
             (many, "65536 pictures in all")]
    for name in ("src", "ref", "ref_cu", "rec", "cu"):
        cases.append((lambda l, p, name=name: setattr(l.structs[1], name, None), f"group 1: {name} is NULL"))
    for name in ("ref_width", "ref_height", "tile_x", "tile_y"):
        cases.append((lambda l, p, name=name: setattr(p, name, 64), "tiles are not part of joint launches"))
    capfd.readouterr()
    for change, message in cases:
        launch, prm = fresh()
        change(launch, prm)
        assert launch.run(sim, prm) == -1, message
        err = capfd.readouterr().err
        assert message in err and "kvz_hostsim_inter_pass_groups" in err, (message, err)
        assert launch.untouched(fill), message
    for n_groups in (0, -1):
        launch, prm = fresh()
        assert launch.run(sim, prm, n_groups=n_groups) == -1
        assert "at least one group" in capfd.readouterr().err and launch.untouched(fill)
    # ... and the launch as it stands is accepted, coeff == NULL included
    launch, prm = fresh()
    launch.structs[0].coeff = None
    check = sim.kvz_hostsim_inter_joint_check
    check.restype, check.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_void_p]
    assert check(C.addressof(launch.structs), 2, C.addressof(prm)) == 0


def test_the_header_declares_and_the_library_exports_the_entry_point():
    dev = open(os.path.join(flatapi.ROOT, "include", "kvz_hip_dev.h")).read()
    types = open(os.path.join(flatapi.ROOT, "include", "kvz_hip_types.h")).read()
    assert re.search(r"\bint\s+" + ENTRY + r"\(const kvz_hip_inter_group \*groups, int n_groups, const kvz_hip_inter_params \*params\);", dev)
    m = re.search(r"typedef struct kvz_hip_inter_group \{(.*?)\} kvz_hip_inter_group;", types, re.S)
    assert m
    names = re.findall(r"\*?(\w+)\s*[,;]", m.group(1))
    assert names == ["struct_size", "width", "height", "n_pictures", "src", "ref", "ref_cu", "rec", "cu", "coeff", "pictures"], names
    assert [n for n, _ in InterGroupStruct._fields_] == names and C.sizeof(InterGroupStruct) == 16 + 7 * 8  # the binding's struct is the header's
    import kvazaar_amd
    out = subprocess.check_output(["nm", "-D", "--defined-only", kvazaar_amd.build_library()], text=True)
    assert re.search(r"\bT " + ENTRY + r"$", out, re.M)
