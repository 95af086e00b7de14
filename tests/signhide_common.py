"""Helpers of the sign-data-hiding tests (kvz_hip_intra_cost_model::signhide, kvazaar's --signhide): the clips of tests/golden/signhide.json, the host simulation
with the sign-hiding instantiations of the CTU program (tests/hostsim/hostsim_signhide.cpp) and its ctypes calls.  Used by tests/test_signhide_sim.py,
tests/test_gpu_signhide.py and tests/golden/make_signhide_golden.py."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np

import ctu_common as cc
import flatapi

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "signhide.json")

# (name, width, height, frames, seed, kind, qp, preset, no_wpp): all-intra (-p 1) encodes with --signhide.  What each is there for:
CLIPS = [
    ("ultrafast-64x64-qp22", 64, 64, 2, 9, "small", 22, "ultrafast", 0),            # every CU is the 64x64 one: levels in the CTU's scratch block in HBM
    ("ultrafast-72x88-qp12", 72, 88, 2, 1, "small", 12, "ultrafast", 0),            # partial CTUs, 8x8 and 16x16 CUs, large levels
    ("ultrafast-200x136-qp27", 200, 136, 2, 3, "small", 27, "ultrafast", 0),        # depths 0-3 all present; the clip whose deblocked pictures are pinned too
    ("ultrafast-200x136-qp27-nowpp", 200, 136, 2, 3, "small", 27, "ultrafast", 1),  # ... and once as one substream per picture
    ("ultrafast-64x64-qp30", 64, 64, 2, 9, "small", 30, "ultrafast", 0),            # CABAC coefficient cost (QP >= 28)
    ("ultrafast-200x136-qp37", 200, 136, 2, 3, "small", 37, "ultrafast", 0),
    ("ultrafast-noise-qp32", 192, 136, 4, 0, "adversarial", 32, "ultrafast", 0),    # flat, noise (every group full), ramp, blocks
    ("fast-200x136-qp27", 200, 136, 2, 3, "small", 27, "fast", 0),                  # 32x32 CUs searched, depths 1-3
    ("fast-noise-qp22", 192, 136, 4, 0, "adversarial", 22, "fast", 0),
]
DEBLOCKED = "ultrafast-200x136-qp27"
# digests only: the pictures tools/bench_signhide.py times (the first eight of the 1080p bench clip), `ultrafast` QP 22
BENCH_CLIP = ("ultrafast-1920x1080-qp22", 1920, 1080, 8, 1, "large", 22, "ultrafast", 0)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def fixture():
    return json.load(open(FIXTURE))


def clip_frames(clip):
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    return cc.yuv_frames(w, h, n, seed, kind)


def switches(clip, signhide=1):
    """the cost-model switches of the clip's preset (tests/test_encoder_parity.py: `fast` = 32x32 CUs searched + the CABAC coefficient cost at every QP)"""
    s = {"signhide": signhide}
    if clip[7] == "fast":
        s.update(search_32x32=1, coeff_cabac=1)
    if clip[8]:
        s["no_wpp"] = 1
    return s


def weights(qp):
    return cc.coeff_weights(qp) if qp < 50 else 0


def table(lib, qps, **sw):
    """a PictureModels table with the reference's fast-estimate weights (signhide: a value, or one per picture)"""
    from kvazaar_amd.batch import PictureModels
    return PictureModels(lib, qps, weights=weights, **sw)


def load_sim():
    """tests/hostsim/libkvz_hostsim_signhide.so, built with the recipe of the other host simulations when it is missing or older than a source"""
    d, csrc = os.path.join(flatapi.ROOT, "tests", "hostsim"), os.path.join(flatapi.ROOT, "kvazaar_amd", "csrc")
    so = os.path.join(d, "libkvz_hostsim_signhide.so")
    srcs = [os.path.join(d, f) for f in ("hostsim_signhide.cpp", "hostsim_models.cpp", "hostsim.cpp")] + [os.path.join(flatapi.ROOT, "include", "kvz_hip_types.h")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = os.path.join(d, f".libkvz_hostsim_signhide.{os.getpid()}.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp, os.path.join(d, "hostsim_signhide.cpp")])
        os.replace(tmp, so)
    return C.CDLL(so)


def sim_pass(sim, pm, w, h, frames):
    """kvz_hostsim_signhide_intra_frames_models on the batch `frames` -> one output dict per picture (None: the table was refused)"""
    n = len(frames)
    one = cc.outputs(w, h)
    big = {k: np.zeros(v.size * n, v.dtype) for k, v in one.items()}
    src = np.concatenate(frames)
    f = sim.kvz_hostsim_signhide_intra_frames_models
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
    rc = f(C.addressof(pm.struct), w, h, n, src.ctypes.data, big["rec"].ctypes.data, big["coeff"].ctypes.data, big["depth"].ctypes.data, big["mode"].ctypes.data,
           big["cost"].ctypes.data)
    if rc != 0:
        return None
    return [{k: v.reshape(n, -1)[i].copy() for k, v in big.items()} for i in range(n)]


def sim_entropy(sim, pm, w, h, outs):
    """kvz_hostsim_signhide_entropy_code_models on the pass outputs `outs` -> [(slice data, substream sizes)] per picture"""
    n, hc = len(outs), (h + 63) // 64
    rows = 1 if pm.no_wpp else hc
    depth, mode, coeff = (np.concatenate([o[k] for o in outs]) for k in ("depth", "mode", "coeff"))
    f = sim.kvz_hostsim_signhide_entropy_code_models
    f.restype = C.c_long
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    buf, sizes, most = np.zeros(n * (w * h * 4 + 4096), np.uint8), np.zeros((n, rows), np.uint32), C.c_uint32(0)

    def run(cap):
        return f(C.addressof(pm.struct), w, h, n, depth.ctypes.data, mode.ctypes.data, coeff.ctypes.data, cap, buf.ctypes.data, sizes.ctypes.data, C.byref(most))
    total = run(12288)
    if total == -1:  # a CTU's bin list did not fit: again with the room it needs, as kvz_hip_batch_entropy_code does
        total = run(most.value)
    assert total >= 0 and total == int(sizes.sum()), total  # (-2: the counting run and the writing run disagree about a substream's size)
    out, at = [], 0
    for i in range(n):
        size = int(sizes[i].sum())
        out.append((bytes(buf[at:at + size]), [int(v) for v in sizes[i]]))
        at += size
    return out
