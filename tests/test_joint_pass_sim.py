"""Batches of different picture sizes in ONE launch of the all-intra CTU pass (kvz_hip_batch_group), without a GPU: the device sources compiled for the host
(tests/hostsim/hostsim_joint.cpp) walk the group's joint ticket list in ticket order, find the record of every drawn picture's batch through the functions the kernel
uses and run the CTU program on that record.  Every picture stays an ordinary picture of its own size and QP, so every output has a truth that exists already: the
reference encoder's digests under tests/golden/ and the unchanged oracle run on that picture alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ctu_common as cc
import flatapi
import joint_common as jc

NEW_SYMBOLS = ["kvz_hip_batch_group_create", "kvz_hip_batch_group_destroy", "kvz_hip_batch_group_intra_frames", "kvz_hip_batch_group_last_kernel_ms"]


@pytest.fixture(scope="module")
def sim():
    return jc.load_sim()


@pytest.fixture(scope="module")
def hiplib():
    """libkvz_hip.so for its host-side functions only (the cost model of a QP): nothing here touches a device"""
    import kvazaar_amd
    return C.CDLL(kvazaar_amd.build_library())


def _tables(hiplib, specs, **switches):
    return [jc.table(hiplib, s.qps, **switches) for s in specs]


# ---------------------------------------------------------------------------------------------------- 1. the lists
SETS = {
    "lone-8x8": [(8, 8, 1)],
    "three-sizes": [(64, 64, 2), (72, 88, 2), (200, 136, 4)],
    "one-ctu-wide+832x480": [(64, 136, 1), (48, 40, 3), (832, 480, 2)],
    "equal-geometries": [(200, 136, 2), (64, 64, 1), (200, 136, 3)],
}


@pytest.mark.parametrize("name", list(SETS))
def test_joint_lists_hold_every_ctu_once_behind_its_dependencies(sim, name):
    """both lists: every CTU of every picture exactly once; the left neighbour, the above-right one (the above one at the right edge, as ticket_loop clamps it) and --
    raster list -- the end of the row above hold lower tickets"""
    sizes = SETS[name]
    wpp, raster, pictures = jc.sim_lists(sim, sizes)
    geo = [((w + 63) // 64, (h + 63) // 64) for w, h, n in sizes for _ in range(n)]  # per group picture
    assert [int(p) for p in pictures] == [b << 16 | f for b, (w, h, n) in enumerate(sizes) for f in range(n)]
    everything = sorted(p << 16 | y << 8 | x for p, (wc, hc) in enumerate(geo) for y in range(hc) for x in range(wc))
    for items, no_wpp in ((wpp, False), (raster, True)):
        assert sorted(int(v) for v in items) == everything
        ticket = {int(v): t for t, v in enumerate(items)}
        for v, t in ticket.items():
            p, y, x = v >> 16, (v >> 8) & 0xff, v & 0xff
            wc = geo[p][0]
            deps = []
            if x > 0:
                deps.append((y, x - 1))
            if y > 0:
                deps.append((y - 1, x + 1 if x + 1 < wc else x))
            if no_wpp and x == 0 and y > 0:
                deps.append((y - 1, wc - 1))
            for dy, dx in deps:
                assert ticket[p << 16 | dy << 8 | dx] < t, (name, no_wpp, p, y, x, dy, dx)
    # the WPP list is anti-diagonal by anti-diagonal across ALL pictures: small pictures do not trail behind the large ones
    diag = [((int(v) & 0xff) + 2 * ((int(v) >> 8) & 0xff)) for v in wpp]
    assert diag == sorted(diag)


# ---------------------------------------------------------------------------------------------------- 2.-4. against the reference encoder
def test_joint_pass_reproduces_the_reference_encoder(sim, hiplib):
    """three sizes, four QPs, both coefficient pricings in one walk: every picture's reconstruction and CU digests are the reference encoder's"""
    specs = jc.main_group()
    rc, outs = jc.sim_joint(sim, specs, _tables(hiplib, specs))
    assert rc == 0
    for s, o in zip(specs, outs):
        assert [jc.sha(p["rec"]) for p in o] == s.want(), (s.w, s.h)
        assert [jc.cu_digest(p, s.w, s.h) for p in o] == s.want("/cu"), (s.w, s.h)


def test_joint_pass_with_32x32_search_and_cabac_reproduces_preset_fast(sim, hiplib):
    specs = jc.main_group(qp_200=(27, 27, 27, 27))  # (the fixture has no /fast digest of 200x136 at QP 37)
    rc, outs = jc.sim_joint(sim, specs, _tables(hiplib, specs, search_32x32=1, coeff_cabac=1))
    assert rc == 0
    for s, o in zip(specs, outs):
        assert [jc.sha(p["rec"]) for p in o] == s.want("/fast"), (s.w, s.h)


def test_joint_pass_without_wpp_equals_the_oracle_and_the_digests(oracle, sim, hiplib):
    """the raster list: the main group and, for the digests that exist, 200x136 at QP 32 -- a second batch of that geometry -- and 64x136 (one CTU wide) at QP 22"""
    specs = jc.main_group() + [jc.clip_spec(200, 136, 2, 3, "small", [32, 32]), jc.clip_spec(64, 136, 1, 3, "small", [22])]
    rc, outs = jc.sim_joint(sim, specs, _tables(hiplib, specs, no_wpp=1))
    assert rc == 0
    for s, o in zip(specs, outs):
        for i, p in enumerate(o):
            m = jc.oracle_model(oracle, s.qps[i], no_wpp=1)
            assert not cc.compare(p, cc.run_oracle(oracle, m, s.w, s.h, s.frames[i])), (s.w, s.h, i)
    for s, o in zip(specs[3:], outs[3:]):
        assert [jc.sha(p["rec"]) for p in o] == s.want("", 0, no_wpp=True), (s.w, s.h)


# ---------------------------------------------------------------------------------------------------- 5. the sizes the movers treat differently
def test_sizes_the_wide_movers_treat_differently_equal_the_oracle_output_by_output(oracle, sim, hiplib):
    """8x8 (a lone partial CTU), 48x40 (width a multiple of 16, not 32), 72x88 (of 8 only), 192x136 (of 64) in one group at QPs 27, 22, 12, 45: the width test of the
    movers is uniform per workgroup but differs between the workgroups of the walk"""
    specs = [jc.oracle_spec(8, 8, 1, 4, 27), jc.oracle_spec(48, 40, 2, 6, 22), jc.oracle_spec(72, 88, 1, 1, 12), jc.oracle_spec(192, 136, 1, 5, 45)]
    rc, outs = jc.sim_joint(sim, specs, _tables(hiplib, specs))
    assert rc == 0
    for s, o in zip(specs, outs):
        for i, p in enumerate(o):
            want = cc.run_oracle(oracle, jc.oracle_model(oracle, s.qps[i]), s.w, s.h, s.frames[i])
            assert not cc.compare(p, want), (s.w, s.h, i, cc.compare(p, want))


# ---------------------------------------------------------------------------------------------------- 6. sign hiding per batch
def test_sign_hiding_in_some_batches_of_a_group(sim, hiplib):
    """hidden 64x64 and plain 200x136 with plain 64x64 and hidden 200x136, one walk through the sign-hiding instantiation: the switch is the drawn picture's model's"""
    a, b = jc.clip_spec(64, 64, 2, 9, "small", [22, 22]), jc.clip_spec(200, 136, 2, 3, "small", [27, 27])
    specs, hide = [a, b, a, b], [1, 0, 0, 1]
    tables = [jc.table(hiplib, s.qps, signhide=h) for s, h in zip(specs, hide)]
    rc, outs = jc.sim_joint(sim, specs, tables)
    assert rc == 0
    hidden = {64: jc.SIGNHIDE["ultrafast-64x64-qp22"]["rec"], 200: jc.SIGNHIDE["ultrafast-200x136-qp27"]["rec"]}
    for s, h, o in zip(specs, hide, outs):
        assert [jc.sha(p["rec"]) for p in o] == (hidden[s.w] if h else s.want()), (s.w, h)
    assert hidden[64] != a.want() and hidden[200] != b.want()


# ---------------------------------------------------------------------------------------------------- 7. the coder
def test_the_entropy_coder_on_a_joint_pass_gives_the_reference_encoders_bytes(sim, hiplib):
    specs = jc.main_group()
    tables = _tables(hiplib, specs)
    rc, outs = jc.sim_joint(sim, specs, tables)
    assert rc == 0
    coded = jc.sim_entropy(sim, tables[2], 200, 136, outs[2])
    jc.check_slice_data([coded[0], coded[3]], jc.ENTROPY["partial-ctus-qp27"])  # the QP 27 pictures: 0 of the clip, then 1


# ---------------------------------------------------------------------------------------------------- 8. refusals, the error word
def test_groups_and_launches_the_library_refuses(sim, hiplib, capfd):
    """through the checks the library and the simulation share (kvz_joint.hpp): -1, a message, nothing computed"""
    a, b = jc.clip_spec(64, 64, 2, 9, "small", [22, 22]), jc.clip_spec(72, 88, 2, 1, "small", [12, 12])
    specs = [a, b]

    def refused(tables, specs=specs, **kw):
        capfd.readouterr()
        rc, outs = jc.sim_joint(sim, specs, tables, **kw)
        err = capfd.readouterr().err
        nothing = all(not p[k].any() for o in outs for p in o for k in ("rec", "coeff", "depth", "mode"))
        return rc == -1 and "kvz_hostsim_joint_intra_frames" in err and nothing
    ok = _tables(hiplib, specs)
    assert jc.sim_joint(sim, specs, ok)[0] == 0
    assert refused(_tables(hiplib, specs, rdoq=1, coeff_cabac=1, search_32x32=1))
    assert refused(_tables(hiplib, specs, search_nxn=1, search_32x32=1, coeff_cabac=1))
    assert refused([jc.table(hiplib, a.qps, search_32x32=1), jc.table(hiplib, b.qps)])
    assert refused([jc.table(hiplib, a.qps), jc.table(hiplib, b.qps, no_wpp=1)])
    assert not refused([jc.table(hiplib, a.qps, coeff_cabac=1), jc.table(hiplib, b.qps, signhide=1)])  # run-time switches may differ
    short = jc.table(hiplib, [22, 30])
    short.index[1] = 5  # a row the table does not have: what a table made for another batch looks like to the library
    assert refused([short, ok[1]])
    assert refused(ok, has_lists=[0, 1])
    assert refused(ok, failed=[1, 0])
    assert refused([ok[0], ok[0]], specs=[a, a], same_buffers=[(1, 0)])  # the same batch twice
    assert jc.sim_joint(sim, [], [])[0] == -1  # n = 0
    # kvz_hip_batch_group_create's own checks
    check = sim.kvz_hostsim_joint_group_check
    check.restype = C.c_int
    check.argtypes = [C.c_int] + [C.c_void_p] * 4

    def group(ids, devices=None, ticket=None, frames=None):
        n = len(ids)
        return check(n, (C.c_size_t * max(n, 1))(*ids), jc._ints(devices or [0] * n), jc._ints(ticket or [1] * n), jc._ints(frames or [2] * n))
    assert group([11, 12, 13]) == 0
    assert group([]) == -1
    assert group([11, 0]) == -1           # a NULL batch
    assert group([11, 12, 11]) == -1      # repeated
    assert group([11, 12], devices=[0, 1]) == -1
    assert group([11, 12], ticket=[1, 0]) == -1  # KVZ_HIP_SCHED=wave
    assert group([11, 12], frames=[65000, 535]) == 0 and group([11, 12], frames=[65000, 536]) == -1
    assert "kvz_hostsim_joint_group_check" in capfd.readouterr().err


def test_a_timed_out_hand_off_reaches_every_batch_of_the_group(sim):
    """the host function that fans the error word of a joint pass out (kvz_batch.hpp joint_check calls it), on hand-written words"""
    f = sim.kvz_hostsim_joint_fan_out
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_char_p, C.c_size_t]
    sizes = [(64, 64, 2), (72, 88, 2), (200, 136, 4)]

    def fan(words, sizes=sizes):
        err, failed, msg = (C.c_uint * 3)(*words), jc._ints([0] * len(sizes)), C.create_string_buffer(640)
        rc = f(err, len(sizes), jc._ints([s[0] for s in sizes]), jc._ints([s[1] for s in sizes]), jc._ints([s[2] for s in sizes]), failed, msg, 640)
        return rc, list(failed), msg.value.decode()
    assert fan([0, 9, 9]) == (-2, [0, 0, 0], "")  # a clear word marks nobody
    # the above-right neighbour x 3 y 1 of group picture 5 = picture 1 of batch 2
    rc, failed, msg = fan([0x80000000 | 0x20000000 | 5 << 16 | 1 << 8 | 3, 41, 17])
    assert rc == 2 and failed == [1, 1, 1]
    assert "picture 1 of batch 2" in msg and "x 3 y 1" in msg and "above-right" in msg and "ALL 3 batches" in msg and "41" in msg and "17" in msg
    rc, failed, msg = fan([0x80000000 | 2 << 16 | 0 << 8 | 0, 0, 3])
    assert rc == 1 and failed == [1, 1, 1] and "picture 0 of batch 1" in msg and "left neighbour" in msg
    # the tag keeps 13 bits of the picture: a group beyond 8192 pictures is told so, and every batch is marked all the same
    rc, failed, msg = fan([0x80000000 | 7 << 16], sizes=[(64, 64, 9000), (8, 8, 1)])
    assert rc == -1 and failed == [1, 1] and "modulo 8192" in msg


def test_library_exports_the_group_entry_points(hiplib):
    text = open(os.path.join(flatapi.ROOT, "include", "kvz_hip_batch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(kvz_hip_[a-z0-9_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(hiplib, name), name
    from kvazaar_amd.batch import BatchGroup
    assert all(hasattr(BatchGroup, k) for k in ("launch", "run", "kernel_ms", "close"))
