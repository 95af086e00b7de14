"""Pictures under different cost models in ONE batch (kvz_hip_picture_models, the kvz_hip_*_models entry points), without a GPU: the device sources compiled for
the host (tests/hostsim/hostsim_models.cpp) walk a mixed batch picture by picture, finding every picture's model through the selection function the kernels use and
running ONE instantiation of the CTU program for the whole batch, as a launch does.  Every picture is an ordinary constant-QP picture, so every output has a reference
that exists already: the reference encoder's digests under tests/golden/, and the unchanged oracle run on that picture alone with that picture's model."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ctu_common as cc
import flatapi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as mg  # noqa: E402

RECON = json.load(open(os.path.join(HERE, "golden", "encoder_recon.json")))
ENTROPY = json.load(open(os.path.join(HERE, "golden", "entropy.json")))
NEW_SYMBOLS = ["kvz_hip_intra_frames_models", "kvz_hip_batch_loop_filters_models", "kvz_hip_batch_entropy_code_models", "kvz_hip_batch_entropy_code_then_models"]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


@pytest.fixture(scope="module")
def sim():
    """tests/hostsim/libkvz_hostsim_models.so: hostsim.cpp plus the twins of the _models entry points, rebuilt when a source is newer"""
    d, csrc = os.path.join(flatapi.ROOT, "tests", "hostsim"), os.path.join(flatapi.ROOT, "kvazaar_amd", "csrc")
    so = os.path.join(d, "libkvz_hostsim_models.so")
    srcs = [os.path.join(d, "hostsim_models.cpp"), os.path.join(d, "hostsim.cpp"), os.path.join(flatapi.ROOT, "include", "kvz_hip_types.h")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = os.path.join(d, f".libkvz_hostsim_models.{os.getpid()}.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp, os.path.join(d, "hostsim_models.cpp")])
        os.replace(tmp, so)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def hiplib():
    """libkvz_hip.so for its host-side functions only (the cost model of a QP): nothing here touches a device"""
    import kvazaar_amd
    return C.CDLL(kvazaar_amd.build_library())


def _weights(qp):
    return cc.coeff_weights(qp) if qp < 50 else 0  # kvazaar has no fast-estimate weights from QP 50 on (and never uses the estimate there)


def _table(hiplib, qps, **switches):
    from kvazaar_amd.batch import PictureModels
    return PictureModels(hiplib, qps, weights=_weights, **switches)


def _run_mixed(sim, pm, w, h, frames, nxn=False):
    """kvz_hostsim_intra_frames_models on the batch `frames` -> one output dict per picture"""
    n = len(frames)
    one = cc.outputs(w, h)
    big = {k: np.zeros(v.size * n, v.dtype) for k, v in one.items()}
    if nxn:
        big["part"], big["mode4"] = np.zeros((h // 8) * (w // 8) * n, np.uint8), np.zeros((h // 4) * (w // 4) * n, np.uint8)
    src = np.concatenate(frames)
    f = sim.kvz_hostsim_intra_frames_models
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8
    rc = f(C.addressof(pm.struct), w, h, n, src.ctypes.data, big["rec"].ctypes.data, big["coeff"].ctypes.data, big["depth"].ctypes.data, big["mode"].ctypes.data,
           big["cost"].ctypes.data, big["part"].ctypes.data if nxn else None, big["mode4"].ctypes.data if nxn else None)
    assert rc == 0
    return [{k: v.reshape(n, -1)[i].copy() for k, v in big.items()} for i in range(n)]


def test_mixed_batch_reproduces_the_reference_encoder_on_both_sides_of_fast_residual_cost(sim, hiplib):
    """[p0 @ 27, p0 @ 37, p1 @ 37, p1 @ 27] in one batch: QP 27 is priced by the fast estimate, QP 37 by the residual coder in counting mode (fast-residual-cost 28) --
    in ONE instantiation, the one with the CABAC model -- and every picture must be the reference encoder's"""
    w, h, n, seed, kind = 200, 136, 2, 3, "small"
    p = cc.yuv_frames(w, h, n, seed, kind)
    qps = [27, 37, 37, 27]
    pm = _table(hiplib, qps)
    assert [int(pm.model_of(i).coeff_cabac) for i in range(4)] == [0, 1, 1, 0]
    outs = _run_mixed(sim, pm, w, h, [p[0], p[0], p[1], p[1]])
    gold = {qp: RECON[mg.clip_key(w, h, n, seed, kind, qp, 0)] for qp in (27, 37)}
    cu = {qp: RECON[mg.clip_key(w, h, n, seed, kind, qp, 0) + "/cu"] for qp in (27, 37)}
    assert [_sha(o["rec"]) for o in outs] == [gold[27][0], gold[37][0], gold[37][1], gold[27][1]]
    assert [mg.cu_digest(o["depth"].reshape(h // 8, w // 8), o["mode"].reshape(h // 8, w // 8)) for o in outs] == [cu[27][0], cu[37][0], cu[37][1], cu[27][1]]


SWITCHES = {"ultrafast": {}, "search_32x32": {"search_32x32": 1}, "rdoq+search_nxn": {"search_32x32": 1, "coeff_cabac": 1, "rdoq": 1, "search_nxn": 1}}


@pytest.mark.parametrize("size", [(192, 136), (200, 136)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(SWITCHES))
def test_every_output_of_a_mixed_batch_equals_the_oracle_picture_by_picture(oracle, sim, hiplib, name, size):
    """random per-picture QPs 0..51: rec, coeff, depth, mode, cost (and the partition maps with search_nxn) of every picture of the mixed batch are byte for byte what
    the unchanged oracle computes for that picture alone under that picture's model"""
    w, h = size
    n = 6
    rng = np.random.default_rng(20260 + w + len(name))
    qps = [int(q) for q in rng.integers(0, 52, n)]
    if name == "ultrafast":
        qps[0], qps[1] = 27, 28  # both pricings in the batch whatever the draw
    clip = cc.yuv_frames(w, h, 2, 3, "small") + cc.yuv_frames(w, h, 4, 0, "adversarial")
    frames = [clip[i] for i in rng.permutation(len(clip))[:n]]
    pm = _table(hiplib, qps, **SWITCHES[name])
    nxn = "nxn" in name
    outs = _run_mixed(sim, pm, w, h, frames, nxn)
    bad = []
    for i, (f, o) in enumerate(zip(frames, outs)):
        model = pm.model_of(i)
        assert model.qp == qps[i]
        want = cc.run_oracle_nxn(oracle, model, w, h, f) if nxn else cc.run_oracle(oracle, model, w, h, f)
        diff = cc.compare(o, want)
        if diff:
            bad.append((i, qps[i], diff))
    assert not bad, bad


def test_slice_data_of_a_mixed_batch_equals_the_reference_encoders(oracle, sim, hiplib):
    """the four adversarial pictures at QP 12, then the same four at QP 37, coded as ONE batch of eight: every substream starts from its picture's own initial contexts"""
    w, h = 192, 136
    frames = cc.yuv_frames(w, h, 4, 0, "adversarial")
    qps = [12] * 4 + [37] * 4
    pm = _table(hiplib, qps)
    outs = [cc.run_oracle(oracle, pm.model_of(i), w, h, frames[i % 4]) for i in range(8)]
    hc = (h + 63) // 64
    depth, mode, coeff = (np.concatenate([o[k] for o in outs]) for k in ("depth", "mode", "coeff"))
    f = sim.kvz_hostsim_entropy_code_models
    f.restype = C.c_long
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    buf, sizes, most = np.zeros(8 * (w * h * 4 + 4096), np.uint8), np.zeros((8, hc), np.uint32), C.c_uint32(0)

    def run(cap):
        return f(C.addressof(pm.struct), w, h, 8, depth.ctypes.data, mode.ctypes.data, None, None, coeff.ctypes.data, None, None, cap, buf.ctypes.data, sizes.ctypes.data, C.byref(most))
    total = run(12288)
    if total == -1:  # a CTU's bin list did not fit (noise at QP 12): again with the room it needs, as kvz_hip_batch_entropy_code does
        total = run(most.value)
    assert total == int(sizes.sum())
    want = ENTROPY["noise-qp12"] + ENTROPY["noise-qp37"]
    at = 0
    for i in range(8):
        size = int(sizes[i].sum())
        assert [int(v) for v in sizes[i]] == want[i]["sizes"], i
        assert hashlib.sha256(bytes(buf[at:at + size])).hexdigest()[:24] == want[i]["sha"], i
        at += size


def test_tables_the_library_refuses(sim, hiplib, capfd):
    from kvazaar_amd.batch import PictureModels, PictureModelsStruct
    check = sim.kvz_hostsim_picture_models_check
    check.restype = C.c_int
    check.argtypes = [C.c_void_p, C.c_int, C.c_int]
    ok = _table(hiplib, [22, 32, 22, 40])
    assert ok.struct.n_models == 3 and list(ok.index) == [0, 1, 0, 2]  # deduplicated
    assert check(C.addressof(ok.struct), 4, 1) == 0

    def refused(pm, n=4, ticket=1):
        return check(C.addressof(pm.struct), n, ticket) == -1
    assert refused(ok, ticket=0)  # KVZ_HIP_SCHED=wave
    for field in ("adaptive", "no_wpp", "search_32x32", "rdoq", "search_nxn"):
        pm = _table(hiplib, [22, 32, 22, 40], coeff_cabac=1)
        setattr(pm.models[1], field, 0 if getattr(pm.models[1], field) else 1)
        assert refused(pm), field
    pm = _table(hiplib, [22, 32, 22, 40])
    pm.models[2].entropy_fbits[5] += 1.0  # the one price table
    assert refused(pm)
    pm = _table(hiplib, [22, 32, 22, 40])
    pm.index[3] = 3  # of 3 models
    assert refused(pm)
    assert not refused(pm, n=3)  # ... beyond the batch's pictures nothing is read
    pm = _table(hiplib, [22, 32, 22, 40])
    pm.struct.struct_size += 8
    assert refused(pm)
    pm = _table(hiplib, [22, 32, 22, 40])
    pm.models[1].struct_size -= 4
    assert refused(pm)
    pm = _table(hiplib, [22, 32, 22, 40])
    pm.struct.n_models = 0
    assert refused(pm)
    pm = _table(hiplib, [30, 40], rdoq=1, coeff_cabac=1, search_32x32=1)
    assert not refused(pm, n=2)
    pm.models[1].coeff_cabac = 0  # rdoq needs the CABAC model
    assert refused(pm, n=2)
    # models may differ in coeff_cabac without rdoq
    pm = _table(hiplib, [22, 32])
    assert [m.coeff_cabac for m in pm.models] == [0, 1] and not refused(pm, n=2)
    assert "kvz_hostsim_picture_models_check" in capfd.readouterr().err  # every refusal says why
    assert C.sizeof(PictureModelsStruct) == 24  # struct_size, n_models, two pointers
    # the intra and entropy twins refuse what the check refuses, and compute nothing
    bad = _table(hiplib, [22, 32])
    bad.index[1] = 7
    f = sim.kvz_hostsim_intra_frames_models
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8
    assert f(C.addressof(bad.struct), 64, 64, 2, *([None] * 8)) == -1
    with pytest.raises(ValueError):
        PictureModels(hiplib, [])
    with pytest.raises(TypeError):
        PictureModels(hiplib, [22], qp=3)


def test_library_exports_the_models_entry_points(hiplib):
    """in the manner of tests/test_capi.py: declared in the header, exported by the library"""
    text = open(os.path.join(flatapi.ROOT, "include", "kvz_hip_batch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(kvz_hip_[a-z0-9_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(hiplib, name), name
    types = open(os.path.join(flatapi.ROOT, "include", "kvz_hip_types.h")).read()
    assert "typedef struct kvz_hip_picture_models" in types
