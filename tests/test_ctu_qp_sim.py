"""A cost model per CTU (kvz_hip_ctu_models, cu_qp_delta with one quantisation group per CTU) without a GPU: the host simulation (tests/hostsim/hostsim_ctu_qp.cpp, which
compiles the text the library compiles) against tests/golden/ctu_qp.json -- what the reference encoder wrote under --roi maps -- and against the statements the GPU
test leans on: the rule of the CU QPs in plain Python, the deblocking filter with a QP per edge over tests/deblock_reference.py, the checks, the ABI, the build list."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest

import ctu_common as cc
import ctu_qp_common as cq

sys.path.insert(0, os.path.join(cq.HERE, "golden"))
import make_golden as mg  # noqa: E402

FIXTURE = cq.fixture()


@pytest.fixture(scope="module")
def sim():
    return cq.load_sim()


@pytest.fixture(scope="module")
def lib():
    """libkvz_hip.so for its host-side functions only (the cost model of a QP): nothing here touches a device"""
    import kvazaar_amd
    return C.CDLL(kvazaar_amd.build_library())


@pytest.fixture(scope="module")
def oracle():
    return cq.flatapi.load_oracle()


@pytest.fixture(scope="module")
def passes(sim, lib):
    """every clip through the simulation's pass and CU-QP step, once"""
    return {name: cq.sim_pass(sim, cq.models(lib, name), *cq.CLIPS[name][:2], cq.clip_frames(name)) for name in cq.CLIPS}


@pytest.mark.parametrize("name", list(cq.CLIPS))
def test_the_simulation_reproduces_the_reference_encoder(passes, name):
    w, h = cq.CLIPS[name][:2]
    outs, want = passes[name], FIXTURE[name]
    assert [cq.sha(o["rec"]) for o in outs] == want["rec"]
    assert [mg.cu_digest(o["depth"].reshape(h // 8, w // 8), o["mode"].reshape(h // 8, w // 8)) for o in outs] == want["cu"]
    assert [cq.sha(o["cu_qp"]) for o in outs] == want["cu_qp"] and [[int(v) for v in o["ctu_qp"]] for o in outs] == want["ctu_qp"]


@pytest.mark.parametrize("name", list(cq.CLIPS))
def test_the_loop_filters_at_the_cu_qps_reproduce_the_reference_encoder(sim, lib, oracle, passes, name):
    """the per-edge-QP statement over tests/deblock_reference.py, on the pre-filter pictures: what the GPU test's deblocked digests stand on -- and behind it the
    simulation's SAO decision with every CTU under its own lambda"""
    w, h = cq.CLIPS[name][:2]
    frames, cm = cq.clip_frames(name), cq.models(lib, name)
    filtered = [cq.sim_loop_filters(sim, oracle, cm, i, w, h, frames[i], o) for i, o in enumerate(passes[name])]
    got = [cq.sha(d) for d, _ in filtered]
    assert got == FIXTURE[name]["deblock"]
    assert [cq.sha(s) for _, s in filtered] == FIXTURE[name]["sao"]
    assert got != FIXTURE[name]["rec"] or name == "low"  # (beta and tc are 0 below QP 16: nothing to filter there)


def _entropy(got):
    return [{"sha": cq.sha(np.frombuffer(data, np.uint8)), "sizes": sizes} for data, sizes in got]


@pytest.mark.parametrize("name", list(cq.CLIPS))
def test_the_coder_reproduces_the_slice_data_of_the_reference_bitstream(sim, lib, passes, name):
    """cu_qp_delta_abs / sign in the first transform unit with a coded block flag of every CTU that has one: deltas 0, +-1 .. +-4, beyond 5 and +-25 among the clips"""
    w, h = cq.CLIPS[name][:2]
    assert _entropy(cq.sim_entropy(sim, cq.models(lib, name), w, h, passes[name])) == FIXTURE[name]["entropy"]


def test_an_all_zero_map_codes_a_delta_of_zero_per_coded_ctu(sim, lib):
    """the reference's encode under an all-zero --roi map: the plain encode's reconstruction (asserted below with the uniform maps), other slice data"""
    name = cq.ZERO_MAP
    w, h = cq.CLIPS[name][:2]
    cm = cq.models(lib, name, zero=True)
    got = _entropy(cq.sim_entropy(sim, cm, w, h, cq.sim_pass(sim, cm, w, h, cq.clip_frames(name))))
    assert got == FIXTURE[name]["entropy_zero_map"] and got != FIXTURE[name]["entropy"]


def test_the_record_of_the_census(passes):
    entries = [FIXTURE[name]["census"] for name in cq.CLIPS]
    assert entries == [cq.census(name, [o["ctu_qp"] for o in passes[name]]) for name in cq.CLIPS]
    assert cq.census_complete({name: FIXTURE[name]["census"] for name in cq.CLIPS})
    wc = cq.grid("3x3")[0]
    wpp, raster = FIXTURE["3x3"]["ctu_qp"], FIXTURE["3x3-nowpp"]["ctu_qp"]
    assert any((a & 255) != (b & 255) for pa, pb in zip(wpp, raster) for i, (a, b) in enumerate(zip(pa, pb)) if i % wc == 0)  # a row start whose predictor differs without WPP
    assert FIXTURE[cq.ZERO_MAP]["plain_rec"] != FIXTURE[cq.ZERO_MAP]["rec"]  # every picture differs from its encode without the map (asserted per clip by the generator)


@pytest.mark.parametrize("name", ["3x3", "3x3-nowpp", "fast-5x2"])
def test_a_map_that_repeats_each_pictures_model_is_the_launch_with_a_model_per_picture(sim, lib, name):
    from kvazaar_amd.batch import CtuModels, PictureModels
    w, h, _, qp = cq.CLIPS[name][:4]
    frames, qps = cq.clip_frames(name), [qp, qp + 4]
    ctus = cq.grid(name)[0] * cq.grid(name)[1]
    outs = cq.sim_pass(sim, CtuModels(lib, qps, [[q] * ctus for q in qps], weights=cq.weights, **cq.switches(name)), w, h, frames)
    want = cq.sim_pass_models(sim, PictureModels(lib, qps, weights=cq.weights, **cq.switches(name)), w, h, frames)
    for i in range(2):
        assert not cc.compare(outs[i], want[i]), i
        assert set(outs[i]["cu_qp"].tolist()) == {qps[i]}
    if name == cq.ZERO_MAP:  # the reference's encode under an all-zero --roi map: the plain encode's reconstruction
        zero = cq.sim_pass(sim, cq.models(lib, name, zero=True), w, h, frames)
        assert [cq.sha(o["rec"]) for o in zero] == FIXTURE[name]["plain_rec"]


def test_pictures_with_maps_and_uniform_pictures_in_one_table_each_come_out_as_if_alone(sim, lib, passes):
    from kvazaar_amd.batch import CtuModels, PictureModels
    name = "3x3"
    w, h, _, qp = cq.CLIPS[name][:4]
    p, maps = cq.clip_frames(name), cq.ctu_qps(name)
    outs = cq.sim_pass(sim, CtuModels(lib, [qp, 37, 22, qp], [maps[0], [37] * 9, [22] * 9, maps[1]], weights=cq.weights), w, h, [p[0], p[0], p[1], p[1]])
    alone = cq.sim_pass_models(sim, PictureModels(lib, [37, 22], weights=cq.weights), w, h, p)
    assert not cc.compare(outs[1], alone[0]) and not cc.compare(outs[2], alone[1])
    for got, want in ((outs[0], passes[name][0]), (outs[3], passes[name][1])):
        assert not cc.compare(got, want) and np.array_equal(got["cu_qp"], want["cu_qp"]) and np.array_equal(got["ctu_qp"], want["ctu_qp"])


@pytest.mark.parametrize("no_wpp", [0, 1])
def test_the_chain_of_the_cu_qps_is_the_rule_on_random_patterns(sim, no_wpp):
    """random CU trees, random coded block flags (many CTUs without any), random maps: the three device steps against the plain-Python rule"""
    rng = np.random.default_rng(11 + no_wpp)
    for w, h in ((64, 64), (200, 136), (264, 72)):
        w8, h8, wc, hc = w // 8, h // 8, (w + 63) // 64, (h + 63) // 64
        n = 3
        depth, coeff = np.zeros((n, h8, w8), np.uint8), np.zeros((n, wc * hc, 6144), np.int16)
        qp_of_ctu, slice_qps = rng.integers(10, 36, (n, hc, wc)).astype(np.uint8), rng.integers(10, 36, n).astype(np.int32)
        for f in range(n):
            for cy, cx in itertools.product(range(hc), range(wc)):
                p_coded = 0.0 if rng.random() < 0.4 else 0.35  # four CTUs in ten have no level at all

                def tree(x8, y8, d):
                    size = 8 >> d
                    if x8 >= w8 or y8 >= h8:
                        return
                    if d < 3 and (x8 + size > w8 or y8 + size > h8 or rng.random() < 0.5):
                        for dy, dx in itertools.product((0, size // 2), repeat=2):
                            tree(x8 + dx, y8 + dy, d + 1)
                        return
                    depth[f, y8:y8 + size, x8:x8 + size] = d
                    if rng.random() < p_coded:  # a level somewhere in one plane of the CU
                        z = sum(((x8 % 8 >> b) & 1) << (2 * b) | ((y8 % 8 >> b) & 1) << (2 * b + 1) for b in range(3))
                        plane = int(rng.integers(0, 3))
                        base, per = ((0, 64), (4096, 16), (5120, 16))[plane]
                        coeff[f, cy * wc + cx, base + z * per + int(rng.integers(0, size * size * per))] = int(rng.integers(1, 5)) * (-1) ** int(rng.integers(0, 2))
                tree(cx * 8, cy * 8, 0)
        cu_qp, ctu_qp = cq.sim_cu_qps(sim, w, h, no_wpp, coeff, depth, qp_of_ctu, slice_qps)
        uncoded = 0
        for f in range(n):
            want_qp, ctus = cq.cu_qps_rule(w, h, no_wpp, depth[f].tolist(), cq.unit_coded(coeff[f], wc), qp_of_ctu[f].tolist(), int(slice_qps[f]))
            assert np.array_equal(np.array(want_qp, np.uint8).ravel(), cu_qp[f]), (w, h, f)
            for (cx, cy), (pred, delta) in ctus.items():
                word = int(ctu_qp[f][cy * wc + cx])
                assert (word & 255, word >> 8 & 255, word >> 16 & 1) == (pred, int(qp_of_ctu[f, cy, cx]), int(delta is not None)), (w, h, f, cx, cy)
                uncoded += delta is None
        assert uncoded > 0 or (w, h) == (64, 64)


def _refusals(lib, name):
    """(what is wrong, a CtuModels the library must refuse, words of its message)"""
    from kvazaar_amd.batch import CtuModels
    qp, ctus = cq.CLIPS[name][3], cq.grid(name)[0] * cq.grid(name)[1]
    out = []
    bad = cq.models(lib, name)
    bad.struct.struct_size += 4
    out.append(("struct_size", bad, "kvz_hip_ctu_models.struct_size"))
    bad = cq.models(lib, name)
    bad.struct.model_of_ctu = None
    out.append(("a NULL map", bad, "model index per CTU"))
    bad = cq.models(lib, name)
    bad.struct.pictures = None
    out.append(("a NULL table", bad, "needs a table"))
    bad = cq.models(lib, name)
    bad.index[ctus + 1] = bad.pictures.struct.n_models
    out.append(("a map index", bad, f"model_of_ctu[1][1] = {bad.pictures.struct.n_models}"))
    bad = cq.models(lib, name)
    bad.pictures.struct.struct_size -= 4
    out.append(("what picture_models_known refuses", bad, "kvz_hip_picture_models.struct_size"))
    bad = cq.models(lib, name)
    bad.pictures.models[1].no_wpp = 1
    out.append(("models that disagree in a switch", bad, "differs from model 0"))
    for switch in ("signhide", "rdoq", "search_nxn"):
        bad = cq.models(lib, name)
        for m in bad.pictures.models:
            setattr(m, switch, 1)
            m.coeff_cabac = 1
            m.search_32x32 = 1
        out.append((switch, bad, "rdoq / search_nxn / signhide"))
    out.append(("a span of 26", CtuModels(lib, [qp, qp], [[qp - 13] * ctus, [qp - 13] * (ctus - 1) + [qp + 13]], weights=cq.weights), "span more than 25"))
    out.append(("a slice QP 26 from a CTU QP", CtuModels(lib, [qp, qp + 14], [[qp] * ctus, [qp - 12] * ctus], weights=cq.weights), "span more than 25"))
    return out


def test_every_refusal_with_its_message(sim, lib, capfd):
    name = "3x3"
    w, h = cq.CLIPS[name][:2]
    check = sim.kvz_hostsim_ctu_models_check
    check.argtypes = [C.c_void_p] + [C.c_int] * 5
    good = cq.models(lib, name)
    assert check(C.addressof(good.struct), w, h, 2, 1, 0) == 0 and capfd.readouterr().err == ""
    for what, bad, words in _refusals(lib, name):
        assert check(C.addressof(bad.struct), w, h, 2, 1, 0) == -1, what
        assert words in capfd.readouterr().err, what
        assert cq.sim_pass(sim, bad, w, h, cq.clip_frames(name)) is None, what  # the pass asks the same function
        capfd.readouterr()
    assert check(C.addressof(good.struct), w, h, 2, 1, 1) == -1 and "the batch has scaling lists" in capfd.readouterr().err
    assert check(C.addressof(good.struct), w, h, 2, 0, 0) == -1 and "KVZ_HIP_SCHED=wave" in capfd.readouterr().err
    assert check(None, w, h, 2, 1, 0) == -1 and "kvz_hip_ctu_models.struct_size 0" in capfd.readouterr().err
    from kvazaar_amd.batch import CtuModels
    edge = CtuModels(lib, [27, 27], [[14] * 8 + [39], [27] * 9], weights=cq.weights)  # a span of exactly 25 runs
    assert check(C.addressof(edge.struct), w, h, 2, 1, 0) == 0


def test_the_abi(lib):
    from kvazaar_amd.batch import CtuModelsStruct
    text = open(os.path.join(cq.flatapi.ROOT, "include", "kvz_hip_types.h")).read()
    body = re.search(r"typedef struct kvz_hip_ctu_models \{(.*?)\} kvz_hip_ctu_models;", text, re.S).group(1)
    assert [re.sub(r"\s+", " ", f.split("/*")[0]).strip() for f in body.strip().split("\n")] == \
        ["uint32_t struct_size;", "const kvz_hip_picture_models *pictures;", "const uint16_t *model_of_ctu;"]
    assert [(n, getattr(CtuModelsStruct, n).offset) for n, _ in CtuModelsStruct._fields_] == [("struct_size", 0), ("pictures", 8), ("model_of_ctu", 16)] and C.sizeof(CtuModelsStruct) == 24
    header = open(os.path.join(cq.flatapi.ROOT, "include", "kvz_hip_batch.h")).read()
    for name in ("kvz_hip_intra_frames_ctu_models", "kvz_hip_batch_loop_filters_ctu_models", "kvz_hip_batch_entropy_code_ctu_models", "kvz_hip_batch_download_cu_qps"):
        assert hasattr(lib, name) and re.search(r"\b" + name + r"\(kvz_hip_batch \*b, ", header), name
    model = cc.hip_cost_model(lib, 27)
    assert model.struct_size == C.sizeof(type(model))  # kvz_hip_intra_cost_model keeps its size: the two cu_qp_delta contexts are not part of it


def test_the_build_list_has_its_own_choice_and_build_py_compiles_exactly_its_units(sim):
    import kvazaar_amd.build as build
    rows, mask = (C.c_int * (64 * 3))(), C.c_ulonglong(0)
    n = sim.kvz_hostsim_ctu_qp_builds(rows, C.byref(mask))
    listed = {tuple(rows[3 * i + 1:3 * i + 3]): rows[3 * i] for i in range(n)}
    assert listed == {(0, 0): 0, (1, 0): 1, (0, 1): 2, (1, 1): 3} and n == 4  # (CABAC, S32) -> unit: intra_ctu_ticket_kernel_ctuqp<CABAC, S32>
    for s32, any_cabac in itertools.product((0, 1), repeat=2):
        assert sim.kvz_hostsim_ctu_qp_build_choose(s32, any_cabac) == listed[any_cabac, s32]
    named = {name: defs for name, src, defs in build.UNITS if src == "kvz_ctu_qp_tu.hip"}
    assert sorted(named) == [f"kvz_ctuqp_tu{k}" for k in sorted(listed.values())] and mask.value == sum(1 << k for k in listed.values())
    assert not any(name.startswith("kvz_ctu_tu") for name in named)  # the units of kvz_ctu_builds.hpp stay that list's
    for name, defs in named.items():
        k = int(name[len("kvz_ctuqp_tu"):])
        assert f"-DKVZ_CTU_QP_KERNEL_TU={k}" in defs and f"-DKVZ_CTU_QP_UNITS_BUILT={mask.value}ull" in defs  # the header refuses another set of units when it compiles
