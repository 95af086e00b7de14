"""Helpers of the scaling-list tests of the all-intra CTU pass (kvz_hip_batch_set_scaling_lists, kvazaar's --scaling-list): the clips of
tests/golden/scaling_lists.json, the host simulation with the LISTS instantiations of the CTU program (tests/hostsim/hostsim_scaling_lists.cpp) and its ctypes
calls.  Used by tests/test_scaling_lists_sim.py, tests/test_gpu_scaling_lists.py and tests/golden/make_scaling_lists_golden.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

import ctu_common as cc
import flatapi
import scaling_lists as sl
import signhide_common as sc

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "scaling_lists.json")
FLAT = 0xffff  # set_of_picture: the picture stays without lists

# (name, width, height, frames, seed, kind, qp, preset, no_wpp): all-intra (-p 1) encodes with --scaling-list default.  What each is there for:
CLIPS = [
    ("ultrafast-64x64-qp22", 64, 64, 2, 9, "small", 22, "ultrafast", 0),         # 32x32 and 16x16 transform units
    ("ultrafast-72x88-qp12", 72, 88, 2, 1, "small", 12, "ultrafast", 0),         # partial CTUs, large levels, chroma 4x4
    ("ultrafast-200x136-qp27", 200, 136, 2, 3, "small", 27, "ultrafast", 0),     # every depth; deblocked pictures and slice data pinned here
    ("fast-200x136-qp27", 200, 136, 2, 3, "small", 27, "fast", 0),               # searched 32x32 CUs
    ("ultrafast-noise-qp37", 192, 136, 4, 0, "adversarial", 37, "ultrafast", 0),  # CABAC cost; 4x4 and 8x8 on the clip-and-shift-left side of the dequantiser
    ("ultrafast-noise-qp44", 64, 64, 4, 0, "adversarial", 44, "ultrafast", 0),   # 16x16 at qp / 6 == shift
    ("ultrafast-noise-qp51", 64, 64, 4, 0, "adversarial", 51, "ultrafast", 0),   # 32x32 at qp / 6 == shift
]
PINNED = "ultrafast-200x136-qp27"
# pictures of the adversarial set that the default lists leave untouched at these QPs (flat picture: no levels at all; ramp and blocks: none where the list is not 16)
UNTOUCHED_OK = {"ultrafast-noise-qp37": (0,), "ultrafast-noise-qp44": (0, 2), "ultrafast-noise-qp51": (0, 2, 3)}
# digests only: the pictures tools/bench_scaling_lists.py times (the first eight of the 1080p bench clip), `ultrafast` QP 22
BENCH_CLIP = ("ultrafast-1920x1080-qp22", 1920, 1080, 8, 1, "large", 22, "ultrafast", 0)
# every transform size that occurs, on both sides of the dequantiser's branch (coverage())
CELLS = [f"{p}-{s}-{side}" for p, sizes in (("luma", (8, 16, 32)), ("chroma", (4, 8, 16))) for s in sizes for side in ("right", "left")]

sha = sc.sha


def fixture():
    return json.load(open(FIXTURE))


def clip_frames(clip):
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    return cc.yuv_frames(w, h, n, seed, kind)


def switches(clip):
    s = sc.switches(clip, 0)
    s.pop("signhide")
    return s


def table(lib, qps, **sw):
    return sc.table(lib, qps, **sw)


def lists(name):
    """a kvazaar_amd.batch.ScalingLists from the list set `name` of tests/scaling_lists.py ("default", "custom")"""
    from kvazaar_amd.batch import ScalingLists
    s = sl.get(name)
    return ScalingLists(s.coeff, s.dc)


# the all-intra switches of kvazaar's presets `ultrafast` .. `fast` (cfg.c: pu-depth-intra, fast-residual-cost)
PRESETS = {"ultrafast": {}, "superfast": {}, "veryfast": {}, "faster": dict(coeff_cabac=1), "fast": dict(coeff_cabac=1, search_32x32=1)}

MIXED = [(0, 22, 0), (1, 22, 2), (0, 27, FLAT), (1, 27, 0), (0, 37, 2), (1, 37, FLAT)]  # (picture of the 200x136 clip, QP, set: 0 default, 2 custom)


def mixed_batch(lib):
    """six 200x136 pictures at QPs 22, 27 and 37 under the sets [default, (unused), custom] or flat -> (frames, table, sets, set_of_picture)"""
    p = cc.yuv_frames(200, 136, 2, 3, "small")
    return [p[i] for i, _, _ in MIXED], table(lib, [qp for _, qp, _ in MIXED]), [lists("default"), lists("default"), lists("custom")], [s for _, _, s in MIXED]


def load_sim():
    """tests/hostsim/libkvz_hostsim_scaling_lists.so, built with the recipe of the other host simulations when it is missing or older than a source"""
    d, csrc = os.path.join(flatapi.ROOT, "tests", "hostsim"), os.path.join(flatapi.ROOT, "kvazaar_amd", "csrc")
    so = os.path.join(d, "libkvz_hostsim_scaling_lists.so")
    srcs = [os.path.join(d, f) for f in ("hostsim_scaling_lists.cpp", "hostsim_models.cpp", "hostsim.cpp")] + [os.path.join(flatapi.ROOT, "include", "kvz_hip_types.h")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = os.path.join(d, f".libkvz_hostsim_scaling_lists.{os.getpid()}.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp, os.path.join(d, "hostsim_scaling_lists.cpp")])
        os.replace(tmp, so)
    return C.CDLL(so)


def set_array(sets):
    from kvazaar_amd.batch import ScalingListsStruct
    return (ScalingListsStruct * max(len(sets), 1))(*[s.struct for s in sets])


def sim_pass(sim, pm, sets, set_of_picture, w, h, frames):
    """kvz_hostsim_lists_intra_frames_models on the batch `frames` with the ScalingLists `sets` (set_of_picture: an index per picture, FLAT, or None for set 0 everywhere)
    -> one output dict per picture (None: refused)"""
    n = len(frames)
    one = cc.outputs(w, h)
    big = {k: np.zeros(v.size * n, v.dtype) for k, v in one.items()}
    src = np.concatenate(frames)
    arr = set_array(sets)
    index = None if set_of_picture is None else (C.c_uint16 * n)(*[int(v) for v in set_of_picture])
    f = sim.kvz_hostsim_lists_intra_frames_models
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
    rc = f(C.addressof(pm.struct), C.addressof(arr) if sets else None, len(sets), C.addressof(index) if index is not None else None, w, h, n, src.ctypes.data,
           big["rec"].ctypes.data, big["coeff"].ctypes.data, big["depth"].ctypes.data, big["mode"].ctypes.data, big["cost"].ctypes.data)
    if rc != 0:
        return None
    return [{k: v.reshape(n, -1)[i].copy() for k, v in big.items()} for i in range(n)]


def sim_block(sim, which, lists_, log2w, c, qp, block):
    """kvz_hostsim_lists_quant / _dequant ("quant" / "dequant") of one row-major block of plane c under the ScalingLists `lists_` (None: the flat list)"""
    f = getattr(sim, "kvz_hostsim_lists_" + which)
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    src, out = np.ascontiguousarray(block, np.int16), np.zeros(block.size, np.int16)
    f(C.addressof(lists_.struct) if lists_ is not None else None, log2w, c, qp, src.ctypes.data, out.ctypes.data)
    return out


# ---- where a CTU's levels are (lcu_t z-order of the planes, kvz_hip_types.h KVZ_HIP_CTU_COEFFS) and the coverage table of the fixture
def _zorder(x4, y4):
    """z-order index of the 4x4 unit (x4, y4)"""
    z = 0
    for b in range(4):
        z |= ((x4 >> b) & 1) << (2 * b) | ((y4 >> b) & 1) << (2 * b + 1)
    return z


def coverage(outs, w, h, qp, set_name="default"):
    """From the pass's outputs of a clip at `qp`: the number of non-zero levels at positions whose list entry is not 16 (at 4x4, where the default list is flat: all
    of them), per plane kind, transform size and side of the dequantiser's branch ("right": rounded and shifted right, "left": clipped and shifted left) --
    {"luma-8-right": count, ...}.  A CU of depth d has one luma transform unit of min(64 >> d, 32) and chroma units of half that (4x4 for the 8x8 CU)."""
    s = sl.get(set_name)
    wc = (w + 63) // 64
    out = {}
    cqp = int(flatapi_chroma_qp(qp))
    for o in outs:
        depth = o["depth"].reshape(h // 8, w // 8)
        coeff = o["coeff"].reshape(-1, 6144)
        done = set()
        for y8 in range(h // 8):
            for x8 in range(w // 8):
                d = int(depth[y8, x8])
                cu = 64 >> d
                x0, y0 = (x8 * 8) // cu * cu, (y8 * 8) // cu * cu
                if (x0, y0) in done:
                    continue
                done.add((x0, y0))
                tu = min(cu, 32)
                for ty in range(y0, y0 + cu, tu):
                    for tx in range(x0, x0 + cu, tu):
                        ctu = coeff[(ty // 64) * wc + tx // 64]
                        for c in range(3):
                            size = tu if c == 0 else max(tu // 2, 4)
                            l2 = size.bit_length() - 1
                            lx, ly = (tx % 64) >> (1 if c else 0), (ty % 64) >> (1 if c else 0)
                            base = (0, 4096, 5120)[c] + _zorder(lx // 4, ly // 4) * 16
                            levels = ctu[base:base + size * size]
                            entries = s.tables(l2, c, 0)[1].astype(np.int64) // sl.INV_QUANT_SCALES[0]
                            counts = int(np.count_nonzero(levels[(entries != 16) | (l2 == 2)]))
                            q = qp if c == 0 else cqp
                            side = "right" if (20 - 14 - (15 - 8 - l2) + 4) > q // 6 else "left"
                            key = f"{'luma' if c == 0 else 'chroma'}-{size}-{side}"
                            out[key] = out.get(key, 0) + counts
    return out


def flatapi_chroma_qp(qp):
    """transform.c kvz_get_scaled_qp for chroma at 8 bit (kvz_g_chroma_scale)"""
    return qp if qp < 30 else (qp - 6 if qp >= 43 else (29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37)[qp - 30])
