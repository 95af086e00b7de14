"""B pictures of different sizes in ONE launch of the inter CTU pass on the MI355X (kvz_hip_dev_inter_ctu_pass_groups through kvazaar_amd.inter.InterGroup).  Every
picture stays an ordinary constant-QP picture, so its reference exists already: the oracle's encode of its own sequence alone (tests/inter_joint_common.py,
tests/inter_mixed_common.py; the oracle is pinned to the reference encoder).  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest

import inter_joint_common as jc
import inter_mixed_common as mx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import kvazaar_amd
    return kvazaar_amd.load_library()


def _close(members):
    for m in members:
        m.close()


def test_four_sizes_in_one_launch_then_each_members_filters_and_coder(lib):
    """the launch of the CPU test (40x24, 72x40, 136x72, 264x136 with 2, 2, 3 and 1 pictures; QPs on both sides of 28; POC 1, 2, 3): every picture equals the oracle's,
    then every member's own loop_filters + entropy_code give its sequences' final pictures and slice data"""
    from kvazaar_amd import inter
    groups = jc.veryfast_groups()
    members = jc.device_members(lib, groups)
    group = inter.InterGroup(lib, members)
    prm = mx.launch_params("veryfast")
    tables = [jc.table_of(pics) for _, _, pics in groups]
    assert group.run(prm, tables) == 0
    for ip, (w, h, pics), table in zip(members, groups, tables):
        jc.assert_member_equals_the_oracle(ip, pics)
        ip.loop_filters(prm, pictures=table)
        for i, p in enumerate(pics):
            assert np.array_equal(ip.download(i)[0], p["final"]), (w, h, i)
        data, sizes = ip.entropy_code(prm, pictures=table)
        mx.assert_slice_data(pics, data, sizes)
    group.close()
    _close(members)  # (close() of the group left them open)


@pytest.mark.parametrize("no_wpp", [0, 1])
def test_workgroups_move_between_sizes_on_the_device(lib, no_wpp, monkeypatch):
    """one workgroup per CU and at least 1.25 x as many CTUs as CUs: the pictures of the four groups replicated until every workgroup must draw again, so persistent
    workgroups move between pictures of different sizes, QPs and POCs.  Every copy equals its original's expected bytes"""
    import torch
    from kvazaar_amd import inter
    base = jc.no_wpp_groups() if no_wpp else jc.veryfast_groups()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_copy = sum(jc.grid(w, h)[0] * jc.grid(w, h)[1] * len(pics) for w, h, pics in base)
    copies = -(-int(1.25 * cus + 1) // per_copy)
    groups = tuple((w, h, pics * copies) for w, h, pics in base)
    assert sum(jc.grid(w, h)[0] * jc.grid(w, h)[1] * len(pics) for w, h, pics in groups) >= 1.25 * cus
    members = jc.device_members(lib, groups, with_levels=[False] * len(groups))
    monkeypatch.setenv("KVZ_HIP_INTER_WG_PER_CU", "1")
    prm = mx.launch_params("veryfast", no_wpp=1, mv_constraint=0) if no_wpp else mx.launch_params("veryfast")
    assert inter.InterGroup(lib, members).run(prm, [jc.table_of(pics) for _, _, pics in groups]) == 0
    for ip, (w, h, pics) in zip(members, groups):
        jc.assert_member_equals_the_oracle(ip, pics)
    _close(members)


def test_one_group_is_the_members_own_run_byte_for_byte(lib):
    """rec, cu and coeff of a group of one member against InterPictures.run on the same pictures; then a launch whose second group has coeff == NULL"""
    from kvazaar_amd import inter
    w, h, pics = jc.veryfast_groups()[2]
    prm = mx.launch_params("veryfast")
    table = jc.table_of(pics)
    outs = []
    for joint in (False, True):
        (ip,) = jc.device_members(lib, ((w, h, pics),))
        zeros = np.zeros(len(pics) * ip.ctus * 6144, np.int16)
        lib.kvz_hip_dev_upload(ip.d_coeff, zeros.ctypes.data, zeros.nbytes)
        if joint:
            assert inter.InterGroup(lib, [ip]).run(prm, [table]) == 0
        else:
            ip.run(prm, pictures=table)
        outs.append(([ip.download(i) for i in range(len(pics))], ip.dev.get(ip.d_coeff, (zeros.size,), np.int16)))
        ip.close()
    (a, la), (b, lb) = outs
    assert np.array_equal(la, lb)
    for (ra, ca), (rb, cb) in zip(a, b):
        assert np.array_equal(ra, rb) and ca.tobytes() == cb.tobytes()
    groups = jc.faster_groups()
    members = jc.device_members(lib, groups, with_levels=[True, False])
    assert members[1].d_coeff is None
    assert inter.InterGroup(lib, members).run(mx.launch_params("faster"), [jc.table_of(pics) for _, _, pics in groups]) == 0
    for ip, (_, _, pics) in zip(members, groups):
        jc.assert_member_equals_the_oracle(ip, pics)
    _close(members)


def test_a_refused_launch_leaves_the_members_alone_and_the_next_one_is_right(lib, capfd):
    from kvazaar_amd import inter
    from kvazaar_amd.inter import InterPictureParams
    groups = jc.veryfast_groups()[1:3]
    members = jc.device_members(lib, groups)
    marks = []
    for ip in members:
        mark = np.full(ip.n * ip.fs, 0x5a, np.uint8)
        lib.kvz_hip_dev_upload(ip.d_rec, mark.ctypes.data, mark.nbytes)
        marks.append(mark)
    group = inter.InterGroup(lib, members)
    prm = mx.launch_params("veryfast")
    tables = [jc.table_of(pics) for _, _, pics in groups]
    capfd.readouterr()
    assert group.run(prm, [tables[0], InterPictureParams([22, 52, 30], [1, 1, 1])]) == -1
    err = capfd.readouterr().err
    assert "QP 52 outside 0..51" in err and "kvz_hip_dev_inter_ctu_pass_groups" in err and "group 1" in err, err
    tiled = mx.launch_params("veryfast", ref_width=264, ref_height=136)
    assert group.run(tiled, tables) == -1 and "tiles are not part of joint launches" in capfd.readouterr().err
    from kvazaar_amd.batch import ScalingLists
    members[1].set_scaling_lists([ScalingLists.default(lib)])  # a member with scaling lists: refused by the binding, with the reason
    with pytest.raises(ValueError, match="member 1 has scaling lists set: they are not part of joint launches"):
        group.run(prm, tables)
    members[1].clear_scaling_lists()
    members[0].sync()
    for ip, mark in zip(members, marks):
        assert np.array_equal(ip.dev.get(ip.d_rec, (mark.size,), np.uint8), mark)
    assert group.run(prm, tables) == 0
    for ip, (_, _, pics) in zip(members, groups):
        jc.assert_member_equals_the_oracle(ip, pics)
    _close(members)
