"""Helpers of the joint-pass tests (kvz_hip_batch_group: batches of different picture sizes in one launch of the all-intra CTU pass): the groups the tests run, the
truths they are compared with -- the reference encoder's digests under tests/golden/ and the unchanged oracle --, and the host simulation
(tests/hostsim/hostsim_joint.cpp) with its ctypes calls.  Used by tests/test_joint_pass_sim.py and tests/test_gpu_joint_pass.py."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

import ctu_common as cc
import flatapi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as mg  # noqa: E402

RECON = json.load(open(os.path.join(HERE, "golden", "encoder_recon.json")))
ENTROPY = json.load(open(os.path.join(HERE, "golden", "entropy.json")))
SIGNHIDE = json.load(open(os.path.join(HERE, "golden", "signhide.json")))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def weights(qp):
    return cc.coeff_weights(qp) if qp < 50 else 0


def table(lib, qps, **switches):
    from kvazaar_amd.batch import PictureModels
    return PictureModels(lib, qps, weights=weights, **switches)


class Spec:
    """one batch of a group: geometry, pictures, the QP of every picture, and where its truth comes from -- clip = (n, seed, kind, picture index of every batch
    picture): the reference encoder's fixture clip the pictures are taken from; None: the oracle"""

    def __init__(self, w, h, frames, qps, clip=None):
        self.w, self.h, self.frames, self.qps, self.clip = w, h, frames, list(qps), clip

    def key(self, qp, deblock=0, no_wpp=False):
        n, seed, kind, _ = self.clip
        return mg.clip_key(self.w, self.h, n, seed, kind, qp, deblock, no_wpp=no_wpp)

    def want(self, suffix="", deblock=0, no_wpp=False):
        """the fixture's digests of the batch's pictures"""
        return [RECON[self.key(q, deblock, no_wpp) + suffix][i] for q, i in zip(self.qps, self.clip[3])]


def clip_spec(w, h, n, seed, kind, qps, pictures=None):
    p = cc.yuv_frames(w, h, n, seed, kind)
    pictures = list(range(n)) if pictures is None else pictures
    return Spec(w, h, [p[i] for i in pictures], qps, (n, seed, kind, pictures))


def oracle_spec(w, h, n, seed, qp):
    return Spec(w, h, cc.yuv_frames(w, h, n, seed, "small"), [qp] * n)


def main_group(qp_200=(27, 37, 37, 27)):
    """64x64 x 2 at QP 22, 72x88 x 2 at QP 12, 200x136 x 4 at [27, 37, 37, 27] on pictures 0, 0, 1, 1 (the mixed-QP test's arrangement)"""
    return [clip_spec(64, 64, 2, 9, "small", [22, 22]), clip_spec(72, 88, 2, 1, "small", [12, 12]), clip_spec(200, 136, 2, 3, "small", list(qp_200), [0, 0, 1, 1])]


def small_specs():
    """a lone partial CTU, and a width that is a multiple of 16 but not of 32: sizes without a digest (the oracle is their truth)"""
    return [oracle_spec(8, 8, 1, 4, 27), oracle_spec(48, 40, 2, 6, 22)]


def cu_digest(o, w, h):
    return mg.cu_digest(o["depth"].reshape(h // 8, w // 8), o["mode"].reshape(h // 8, w // 8))


def oracle_model(oracle, qp, **switches):
    from test_encoder_parity import oracle_model as om
    m = om(oracle, qp)
    for k, v in switches.items():
        setattr(m, k, v)
    return m


# ---- the host simulation ----
def load_sim():
    """tests/hostsim/libkvz_hostsim_joint.so, built with the recipe of the other host simulations when it is missing or older than a source"""
    d, csrc = os.path.join(flatapi.ROOT, "tests", "hostsim"), os.path.join(flatapi.ROOT, "kvazaar_amd", "csrc")
    so = os.path.join(d, "libkvz_hostsim_joint.so")
    srcs = [os.path.join(d, f) for f in ("hostsim_joint.cpp", "hostsim_signhide.cpp", "hostsim_models.cpp", "hostsim.cpp")] + [os.path.join(flatapi.ROOT, "include", "kvz_hip_types.h")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = os.path.join(d, f".libkvz_hostsim_joint.{os.getpid()}.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp, os.path.join(d, "hostsim_joint.cpp")])
        os.replace(tmp, so)
    return C.CDLL(so)


def _ints(values):
    return (C.c_int * max(len(values), 1))(*values)


def sim_lists(sim, sizes):
    """sizes: (w, h, n) per batch -> (wpp items, raster items, picture words) of the group, as the library builds them"""
    total = sum(((w + 63) // 64) * ((h + 63) // 64) * n for w, h, n in sizes)
    wpp, raster, pictures = np.zeros(total, np.uint32), np.zeros(total, np.uint32), np.zeros(sum(n for _, _, n in sizes), np.uint32)
    f = sim.kvz_hostsim_joint_lists
    f.restype = C.c_long
    f.argtypes = [C.c_int] + [C.c_void_p] * 6
    got = f(len(sizes), _ints([s[0] for s in sizes]), _ints([s[1] for s in sizes]), _ints([s[2] for s in sizes]), wpp.ctypes.data, raster.ctypes.data, pictures.ctypes.data)
    assert got == total, (got, total)
    return wpp, raster, pictures


def sim_joint(sim, specs, tables, has_lists=None, failed=None, same_buffers=()):
    """kvz_hostsim_joint_intra_frames -> (return value, outputs [batch][picture]).  same_buffers: (i, k) pairs -- batch i is handed batch k's buffers (the same
    batch twice)"""
    n = len(specs)
    bigs = []
    for s in specs:
        one = cc.outputs(s.w, s.h)
        bigs.append({k: np.zeros(v.size * len(s.frames), v.dtype) for k, v in one.items()})
    for i, k in same_buffers:
        bigs[i] = bigs[k]
    srcs = [np.concatenate(s.frames) for s in specs]

    def ptrs(arrays):
        return (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrays])
    f = sim.kvz_hostsim_joint_intra_frames
    f.restype = C.c_int
    f.argtypes = [C.c_int] + [C.c_void_p] * 12
    rc = f(n, (C.c_void_p * max(n, 1))(*[C.addressof(t.struct) for t in tables]), _ints([s.w for s in specs]), _ints([s.h for s in specs]), _ints([len(s.frames) for s in specs]),
           ptrs(srcs), *[ptrs([b[k] for b in bigs]) for k in ("rec", "coeff", "depth", "mode", "cost")],
           _ints(has_lists) if has_lists else None, _ints(failed) if failed else None)
    outs = [[{k: v.reshape(len(s.frames), -1)[i].copy() for k, v in b.items()} for i in range(len(s.frames))] for s, b in zip(specs, bigs)]
    return rc, outs


def sim_entropy(sim, pm, w, h, outs):
    """kvz_hostsim_entropy_code_models on pass outputs -> [(slice data, substream sizes)] per picture"""
    n, hc = len(outs), (h + 63) // 64
    rows = 1 if pm.no_wpp else hc
    depth, mode, coeff = (np.concatenate([o[k] for o in outs]) for k in ("depth", "mode", "coeff"))
    f = sim.kvz_hostsim_entropy_code_models
    f.restype = C.c_long
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    buf, sizes, most = np.zeros(n * (w * h * 4 + 4096), np.uint8), np.zeros((n, rows), np.uint32), C.c_uint32(0)

    def run(cap):
        return f(C.addressof(pm.struct), w, h, n, depth.ctypes.data, mode.ctypes.data, None, None, coeff.ctypes.data, None, None, cap, buf.ctypes.data, sizes.ctypes.data, C.byref(most))
    total = run(12288)
    if total == -1:
        total = run(most.value)
    assert total == int(sizes.sum())
    out, at = [], 0
    for i in range(n):
        size = int(sizes[i].sum())
        out.append((bytes(buf[at:at + size]), [int(v) for v in sizes[i]]))
        at += size
    return out


def check_slice_data(got, want):
    """got: (bytes, sizes) per picture; want: the fixture's entries"""
    assert len(got) == len(want)
    for i, ((data, sizes), g) in enumerate(zip(got, want)):
        assert sizes == g["sizes"], i
        assert hashlib.sha256(data).hexdigest()[:24] == g["sha"], i
