"""Pictures with a QP and a POC of their own in ONE launch of the inter path (kvz_hip_inter_pictures, the kvz_hip_dev_*_pictures entry points), without a GPU: the
device sources compiled for the host (tests/hostsim/hostsim_inter_models.cpp) walk a mixed launch in the launch's ticket order with ONE program state, as a persistent
workgroup does -- consecutive CTUs belong to different pictures, QPs and POCs.  Every picture is an ordinary constant-QP picture, so its reference exists already:
the oracle's encode of its own sequence alone (inter_common.oracle_encode*, pinned to the reference encoder).  All comparisons are exact.

The loop filters of inter pictures have no host twin (hostsim.cpp offers the SAO decision of an all-intra model only), so kvz_hip_dev_loop_filters_inter_pictures is
covered on the device alone (tests/test_gpu_inter_mixed_qp.py); the slice data has one (kvz_hostsim_entropy_code_inter_pictures) and is covered here too."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import flatapi
import inter_common as ic
import inter_mixed_common as mx
from kvazaar_amd.inter import InterPictureParams, InterPicturesStruct

NEW_SYMBOLS = ["kvz_hip_dev_inter_ctu_pass_pictures", "kvz_hip_dev_loop_filters_inter_pictures", "kvz_hip_dev_entropy_code_inter_pictures"]


@pytest.fixture(scope="module")
def sim():
    """tests/hostsim/libkvz_hostsim_inter_models.so: hostsim.cpp plus the twins of the _pictures entry points, rebuilt when a source is newer"""
    d, csrc = os.path.join(flatapi.ROOT, "tests", "hostsim"), os.path.join(flatapi.ROOT, "kvazaar_amd", "csrc")
    so = os.path.join(d, "libkvz_hostsim_inter_models.so")
    srcs = [os.path.join(d, "hostsim_inter_models.cpp"), os.path.join(d, "hostsim.cpp"), os.path.join(flatapi.ROOT, "include", "kvz_hip_types.h"), os.path.join(flatapi.ROOT, "include", "kvz_hip_dev.h")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = os.path.join(d, f".libkvz_hostsim_inter_models.{os.getpid()}.so")
        # -Bsymbolic: the library holds a second copy of everything in libkvz_hostsim.so, which other tests load with RTLD_GLOBAL -- without it this copy's calls to
        # the program's inline functions would bind to that library's, which run on ITS workgroup-scope state (g_il / g_ic are file-static)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wl,-Bsymbolic", "-o", tmp, os.path.join(d, "hostsim_inter_models.cpp")])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.kvz_hostsim_mul24_violations.restype = C.c_ulonglong
    return lib


def test_veryfast_launch_of_five_sequences_at_three_gop_positions_equals_each_sequences_own_encode(sim):
    """ten pictures of sequences at --qp 17, 22, 27, 32, 37 (`veryfast`, loop filters, mv-constraint), POC 1, 2 and 3 side by side, walked in ticket order: picture QPs on
    both sides of fast-residual-cost 28 (the CABAC build's fast path beside its residual coder), poc == 1 pictures without temporal AMVP beside poc > 1 ones"""
    pics = mx.veryfast_pictures()
    qps, pocs = [p["qp"] for p in pics], [p["poc"] for p in pics]
    assert min(qps) < 28 <= max(qps) and {1, 2, 3} <= set(pocs)
    print("picture QPs", qps, "POCs", pocs)
    sim.kvz_hostsim_mul24_reset()
    rc, rec, cu, coeff = mx.hostsim_pass(sim, pics, mx.launch_params("veryfast"), InterPictureParams(qps, pocs))
    assert rc == 0
    mx.assert_pictures_equal_the_oracle(pics, rec, cu)
    assert int(sim.kvz_hostsim_mul24_violations()) == 0
    mx.assert_slice_data(pics, *mx.hostsim_slice_data(sim, pics, cu, coeff, mx.W, mx.H))  # the pass's levels, wherever a coded block flag makes them count


def test_faster_launch_with_the_qp_range_ends_equals_each_sequences_own_encode(sim):
    """`faster` (fast-residual-cost 0: every picture priced by the residual coder; quarter-sample search) with sequences at the ends of the range, --qp 0 and --qp 51,
    in the launch: their B pictures run at 2 and 3 (the GOP layer's offset; no B picture of a constant-QP sequence runs lower) and at 51"""
    w, h = 136, 72
    seqs = [mx.sequence(qp, preset="faster", seed=10 + i, w=w, h=h, n=3) for i, qp in enumerate((0, 51, 30))]
    pics = [mx.picture(seqs[0], 1), mx.picture(seqs[1], 2), mx.picture(seqs[2], 1), mx.picture(seqs[1], 1), mx.picture(seqs[0], 2)]
    qps, pocs = [p["qp"] for p in pics], [p["poc"] for p in pics]
    assert sorted(set(qps)) == [2, 3, 33, 51], qps
    sim.kvz_hostsim_mul24_reset()
    rc, rec, cu, coeff = mx.hostsim_pass(sim, pics, mx.launch_params("faster"), InterPictureParams(qps, pocs), w=w, h=h)
    assert rc == 0
    mx.assert_pictures_equal_the_oracle(pics, rec, cu)
    assert int(sim.kvz_hostsim_mul24_violations()) == 0
    mx.assert_slice_data(pics, *mx.hostsim_slice_data(sim, pics, cu, coeff, w, h))  # the pass's levels, wherever a coded block flag makes them count


def test_tiled_launch_with_two_qps(sim):
    """ref_width / tile_xy, no_tmvp, no_wpp with two QPs in one launch.  The oracle encodes whole frames with TMVP on, so the pictures are POC 1 of --no-wpp sequences:
    their reference is the I picture, whose records carry no motion, and no_tmvp changes nothing.  Pictures 0 and 1 are whole frames handed over as the one tile of
    their frame (origin through tile_xy): expected = the oracle's picture.  Pictures 2 and 3 are 128x64 tiles at (64, 64) and (128, 8) of the same frames: motion
    leaves the tile, which no whole-frame encode states, so their expected outputs are the single-QP twin's (kvz_hostsim_inter_tile, pinned to the reference
    encoder's tiled streams by tests/test_dist_cpu.py) on each tile alone"""
    w, h = 264, 136
    seqs = [mx.sequence(qp, seed=20 + i, w=w, h=h, n=2, no_wpp=True, mv_constraint=False, parts=False) for i, qp in enumerate((22, 32))]
    full = [mx.picture(s, 1) for s in seqs]
    assert full[0]["qp"] < 28 <= full[1]["qp"]
    prm = mx.launch_params("veryfast", no_wpp=1, mv_constraint=0, ref_width=w, ref_height=h, no_tmvp=1)
    ref, ref_cu = mx.stacked(full, "ref"), np.concatenate([np.ascontiguousarray(p["ref_cu"]).reshape(-1) for p in full])
    rc, rec, cu, _ = mx.hostsim_pass(sim, full, prm, InterPictureParams([p["qp"] for p in full], [1, 1]), w=w, h=h, tile_xy=[[0, 0], [0, 0]], n_references=2, ref=ref, ref_cu=ref_cu)
    assert rc == 0
    mx.assert_pictures_equal_the_oracle(full, rec, cu)
    # real tiles: picture p predicts from frame p % 2
    import tile_common as tc
    tw, th, origins = 128, 64, [(64, 64), (128, 8)]
    alone = tc.hostsim_tile_pass(sim)
    sim.kvz_hostsim_inter_tile.restype = None
    sim.kvz_hostsim_inter_tile.argtypes = [C.c_int] * 4 + [C.c_uint64, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 5 + [C.c_int] * 5
    tiles = []
    for p, (tx, ty) in zip(full, origins):
        src = tc.tile_sub(p["src"], tx, ty, tw, th, w, h)
        want_rec, want_cu = alone(tw, th, p["qp"], 1, src, np.ascontiguousarray(p["ref"]), np.ascontiguousarray(p["ref_cu"]), w, h, tx, ty)
        tiles.append(dict(src=src, rec=want_rec, cu=want_cu, qp=p["qp"], poc=1))
    rc, rec, cu, _ = mx.hostsim_pass(sim, tiles, prm, InterPictureParams([t["qp"] for t in tiles], [1, 1]), w=tw, h=th, tile_xy=origins, n_references=2, ref=ref, ref_cu=ref_cu)
    assert rc == 0
    mx.assert_pictures_equal_the_oracle(tiles, rec, cu)


def test_slice_data_of_a_mixed_launch_equals_each_sequences_own(sim):
    """the entropy coder over the ten pictures of the veryfast launch in one job: a row of B-slice context states per distinct QP, a POC per picture (the temporal MV
    predictor exists from POC 2 on); inputs are the oracle's records, levels and SAO decisions, the bytes must be those of the sequence's own bitstream"""
    pics = mx.veryfast_pictures()
    cu = np.stack([np.ascontiguousarray(p["seq"]["parts"]["cu"][p["k"]]) for p in pics])
    coeff = np.stack([p["coeff"] for p in pics])
    mx.assert_slice_data(pics, *mx.hostsim_slice_data(sim, pics, cu, coeff))


def _check(sim, qps, pocs, n, struct_size=None, null=None):
    t = InterPictureParams(qps, pocs)
    if struct_size is not None:
        t.struct.struct_size = struct_size
    if null:
        setattr(t.struct, null, None)
    f = sim.kvz_hostsim_inter_pictures_check
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int]
    return f(t.ptr, n)


def test_refusals(sim, capfd):
    """the rules of kvz_inter_pictures.hpp, the text kvz_hip_dev_*_pictures check with before they queue anything: return code and message"""
    assert _check(sim, [22, 30], [1, 2], 2) == 0
    assert _check(sim, [0, 51], [1, 1 << 20], 2) == 0
    capfd.readouterr()
    for kw, args, message in ((dict(struct_size=C.sizeof(InterPicturesStruct) + 8), ([22, 30], [1, 2], 2), "struct_size"),
                              (dict(struct_size=0), ([22, 30], [1, 2], 2), "struct_size"),
                              ({}, ([22, 30], [1, 2], 3), "n_pictures 2 is not the call's 3"),
                              (dict(null="qp"), ([22, 30], [1, 2], 2), "qp is NULL"),
                              (dict(null="poc"), ([22, 30], [1, 2], 2), "poc is NULL"),
                              ({}, ([22, 52], [1, 2], 2), "picture 1 has QP 52 outside 0..51"),
                              ({}, ([-1, 30], [1, 2], 2), "picture 0 has QP -1 outside 0..51"),
                              ({}, ([22, 30], [1, 0], 2), "picture 1 has POC 0 below 1")):
        assert _check(sim, *args, **kw) == -1, (kw, args)
        err = capfd.readouterr().err
        assert message in err and "kvz_hostsim_inter_pictures_check" in err, (message, err)
    g = sim.kvz_hostsim_inter_picture_qps_check
    g.restype, g.argtypes = C.c_int, [C.c_void_p, C.c_int]
    ok = np.array([0, 51, 28], np.int32)
    assert g(ok.ctypes.data, 3) == 0
    capfd.readouterr()
    assert g(None, 3) == -1 and "QP array is NULL" in capfd.readouterr().err
    bad = np.array([0, 60, 28], np.int32)
    assert g(bad.ctypes.data, 3) == -1 and "picture 1 has QP 60" in capfd.readouterr().err
    # the pass's twin refuses through the same text and computes nothing
    pics = [mx.picture(mx.sequence(22, seed=1), 1)]
    rc, rec, cu, _ = mx.hostsim_pass(sim, pics, mx.launch_params("veryfast"), InterPictureParams([22, 22], [1, 1]))
    assert rc == -1 and not rec.any() and "n_pictures 2 is not the call's 1" in capfd.readouterr().err


def test_headers_declare_the_new_entry_points_and_the_struct():
    dev = open(os.path.join(flatapi.ROOT, "include", "kvz_hip_dev.h")).read()
    types = open(os.path.join(flatapi.ROOT, "include", "kvz_hip_types.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|long)\s+" + name + r"\(", dev), name
    m = re.search(r"typedef struct kvz_hip_inter_pictures \{(.*?)\} kvz_hip_inter_pictures;", types, re.S)
    assert m
    fields = re.findall(r"^\s*(?:const )?(\w+)\s+\*?(\w+);", m.group(1), re.M)
    assert fields == [("uint32_t", "struct_size"), ("int32_t", "n_pictures"), ("int32_t", "qp"), ("int32_t", "poc")], fields
    assert C.sizeof(InterPicturesStruct) == 24  # the binding's struct is the header's


def test_library_exports_the_new_entry_points():
    import kvazaar_amd
    out = subprocess.check_output(["nm", "-D", "--defined-only", kvazaar_amd.build_library()], text=True)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bT " + name + r"$", out, re.M), name
