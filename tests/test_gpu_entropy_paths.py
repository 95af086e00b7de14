"""The entropy coder ON THE DEVICE on constructed decisions (-m gpu; the CPU half, with the census of what these pictures reach, is tests/test_entropy_paths.py): every
picture of tests/entropy_atlas.py through kvz_hip_dev_entropy_code_intra / kvz_hip_dev_entropy_code_inter, slice data and substream sizes byte for byte the oracle's.
The stage pictures are the ones that reach what runs on the device only: emulation prevention counted by position, the compaction kernel's 256 pieces with zero runs
that begin in an earlier piece, the offsets scan over more than 256 substreams.  Then the host-side paths at their other settings: the capacity retry, a chunk per
picture, the 8 / 16 / 32-lane forms of stage 3."""
import os
import subprocess
import sys

import pytest

import entropy_atlas as ea
import entropy_common as ec

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    import kvazaar_amd
    return kvazaar_amd.load_library()


@pytest.fixture(scope="module")
def intra_oracle(oracle):
    return {g[0]: ec.atlas_oracle_group(oracle, g) for g in ea.intra_groups() + ea.stage_groups()}


@pytest.fixture(scope="module")
def b_oracle(oracle):
    return {name: [ec.oracle_entropy_b(oracle, sw, w, h, p) for p in pictures] for name, w, h, sw, pictures in ea.b_groups()}


def differing(got, want):
    """the pictures of a group whose bytes or sizes differ: (picture, sizes got, sizes wanted, first differing byte)"""
    bad = []
    for k, (g, w) in enumerate(zip(got, want)):
        if g != w:
            first = next((i for i, (a, b) in enumerate(zip(g[0], w[0])) if a != b), min(len(g[0]), len(w[0])))
            bad.append((k, g[1], w[1], first))
    return bad + ([("pictures", len(got), len(want))] if len(got) != len(want) else [])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [g[0] for g in ea.intra_groups()])
def test_device_codes_the_intra_atlas(lib, intra_oracle, name):
    group = next(g for g in ea.intra_groups() if g[0] == name)
    assert not differing(ec.device_intra_group(lib, group), intra_oracle[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [g[0] for g in ea.b_groups()])
def test_device_codes_the_b_atlas(lib, b_oracle, name):
    group = next(g for g in ea.b_groups() if g[0] == name)
    assert not differing(ec.device_b_group(lib, group), b_oracle[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [g[0] for g in ea.stage_groups()])
def test_device_codes_the_stage_pictures(lib, intra_oracle, name):
    """"tall-272-substreams" is the launch with more than 256 substreams: their sizes and their places in the output pin the scan kernel's second block"""
    group = next(g for g in ea.stage_groups() if g[0] == name)
    assert not differing(ec.device_intra_group(lib, group), intra_oracle[name])


@pytest.mark.gpu
def test_intra_entry_point_refuses_before_it_queues(lib):
    """-1 for a NULL required pointer, a size that is no positive multiple of 8, a model of another struct_size, search_nxn without maps, half a set of SAO arrays"""
    import ctypes as C

    import numpy as np
    from kvazaar_amd.batch import cost_model
    from kvazaar_amd.dev import Dev
    dev = Dev(lib)
    f = lib.kvz_hip_dev_entropy_code_intra
    f.restype = C.c_long
    f.argtypes = [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p] * 6 + [C.c_size_t, C.c_void_p]
    d8, d4, dc = dev.put(np.zeros(64, np.uint8)), dev.put(np.zeros(256, np.uint8)), dev.put(np.zeros(6144, np.int16))
    out, sizes, merge, sao = np.zeros(4096, np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.uint8), np.zeros(15, np.int32)
    model = cost_model(lib, 22)

    def call(depth=d8, mode=d8, part=None, mode4=None, coeff=dc, w=64, h=64, m=model, luma=None, chroma=None, mg=None, o=out.ctypes.data, s=sizes.ctypes.data):
        return f(depth, mode, part, mode4, coeff, w, h, 1, C.addressof(m), None, luma, chroma, mg, o, out.nbytes, s)
    try:
        assert call() > 0  # (the arguments the refusals below change one of)
        assert call(depth=None) == -1 and call(mode=None) == -1 and call(coeff=None) == -1 and call(o=None) == -1 and call(s=None) == -1
        assert call(w=60) == -1 and call(h=0) == -1 and call(w=-64) == -1
        other = cost_model(lib, 22)
        other.struct_size -= 4
        assert call(m=other) == -1
        nxn = cost_model(lib, 22)
        nxn.search_nxn = 1
        assert call(m=nxn) == -1 and call(m=nxn, part=d8) == -1 and call(m=nxn, part=d8, mode4=d4) > 0
        assert call(luma=sao.ctypes.data) == -1 and call(luma=sao.ctypes.data, chroma=sao.ctypes.data, mg=merge.ctypes.data) > 0
    finally:
        dev.free(d8, d4, dc)


@pytest.fixture()
def coder_settings():
    """KVZ_HIP_ENTROPY_CAP / KVZ_HIP_ENTROPY_SCRATCH_MB are read on every call"""
    saved = {k: os.environ.get(k) for k in ("KVZ_HIP_ENTROPY_CAP", "KVZ_HIP_ENTROPY_SCRATCH_MB")}

    def put(**kw):
        for k, v in kw.items():
            os.environ[k] = str(v)
    yield put
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


# CAP 16: no CTU's bin list fits, every chunk runs again with the room its largest CTU needs.  CAP 16384 with one megabyte of scratch: 20 (12) CTUs of 16 384 records
# are 1.25 (0.75) MB, so a chunk holds one picture of the intra (B) group
@pytest.mark.gpu
@pytest.mark.parametrize("setting", [{"KVZ_HIP_ENTROPY_CAP": 16}, {"KVZ_HIP_ENTROPY_CAP": 16384, "KVZ_HIP_ENTROPY_SCRATCH_MB": 1}], ids=["retry", "chunk-per-picture"])
def test_device_capacity_retry_and_chunks_give_the_same_bytes(lib, intra_oracle, b_oracle, coder_settings, setting):
    intra = next(g for g in ea.intra_groups() if g[0] == "five-wide-cut-both-sao-nxn")
    b = next(g for g in ea.b_groups() if g[0] == "cut-both-poc3")
    coder_settings(**setting)
    assert not differing(ec.device_intra_group(lib, intra), intra_oracle[intra[0]])
    assert not differing(ec.device_b_group(lib, b), b_oracle[b[0]])


@pytest.mark.gpu
def test_device_lane_forms_of_stage_3():
    """KVZ_HIP_ENTROPY_LANES is read once per process: a fresh child per value, one after the other, each under its own time limit; the first child that fails or does
    not end cleanly ends the test, and no further child is started"""
    for lanes in (8, 16, 32):
        env = dict(os.environ, KVZ_HIP_ENTROPY_LANES=str(lanes))
        r = subprocess.run(["timeout", "-k", "10", "150", sys.executable, os.path.join(HERE, "entropy_lanes_child.py")], env=env, capture_output=True, text=True)
        assert r.returncode == 0, (lanes, r.returncode, r.stdout[-1500:], r.stderr[-1500:])
