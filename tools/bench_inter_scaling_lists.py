#!/usr/bin/env python3
"""What per-coefficient scaling lists (kvz_hip_dev_inter_ctu_pass_lists, kvazaar's --scaling-list default) cost in the inter CTU pass.

BASELINE config 4's picture as bench.py's inter leg runs it: 3840x2160 `--preset veryfast --gop lp-g4d3t1 -q 22` (kvazaar_amd.synth, seed 2), the first B picture
(picture QP 25) of `--sequences` independent sequences in one launch, every sequence the same clip.  The same resident pictures in three legs:
  flat        no lists (n_sets == 0: the `_fast` kernel of every launch without them), from the I picture encoded without lists
  default     every picture under the default lists (the `_lists_fast` kernel), from the I picture encoded under them (HipBatch.set_scaling_lists)
  flat_again  the lists cleared
Times are device times from the HIP events the library records around the launch (kvz_hip_dev_inter_kernel_ms), warm-up launches first.  The timed launches are
verified: the CU decisions of the flat legs against the reference encoder's (tests/golden/inter_recon.json), the CU decisions and -- after the loop filters -- the
final picture of the `default` leg against the reference encoder run with --scaling-list default (tests/golden/inter_scaling_lists.json); the first and the last
sequence of a launch must agree.  A library without the entry point (an older build, timed for comparison through KVZ_HIP_LIB) runs the flat legs only.
Prints one JSON line; exit status 1 when a verification fails.  Usage: python tools/bench_inter_scaling_lists.py [--sequences 384] [--steps 3] [--warmup 1]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLIP = "baseline-c4-2160p"


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def i_picture(lib, w, h, frame, qp, lists):
    """the I picture through the all-intra pass and its loop filters on the device -> the final picture"""
    from kvazaar_amd.batch import HipBatch, ScalingLists, cost_model
    b = HipBatch(lib, w, h, 1)
    try:
        b.upload(0, frame)
        if lists:
            b.set_scaling_lists([ScalingLists.default(lib)])
        model = cost_model(lib, qp)
        b.launch(model)
        b.loop_filters(model, deblock=True, sao=True)
        return b.download(0)["rec"]
    finally:
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=384)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import kvazaar_amd
    from kvazaar_amd import inter, synth
    from kvazaar_amd.batch import ScalingLists
    lib = kvazaar_amd.load_library()
    has_lists = hasattr(lib, "kvz_hip_dev_inter_ctu_pass_lists")
    lib.kvz_hip_dev_inter_kernel_ms.restype = C.c_float
    w, h, n, qp = 3840, 2160, args.sequences, 22
    pictures = [np.concatenate([p.reshape(-1) for p in planes]) for planes in synth.frames(w, h, 2, 2, "large")]
    qps = [inter.lowdelay_picture_qp(qp, k) for k in range(2)]
    flat_gold = json.load(open(os.path.join(ROOT, "tests", "golden", "inter_recon.json")))[CLIP]
    refs = {False: i_picture(lib, w, h, pictures[0], qps[0], False)}
    ok = {"i_picture_flat": sha(refs[False]) == flat_gold["rec"][0]}
    if has_lists:
        gold = json.load(open(os.path.join(ROOT, "tests", "golden", "inter_scaling_lists.json")))[CLIP]
        refs[True] = i_picture(lib, w, h, pictures[0], qps[0], True)
        ok["i_picture_default"] = sha(refs[True]) == gold["rec"][0]
    ip = inter.InterPictures(lib, w, h, n)
    cu0 = inter.intra_picture_cu_info(w, h)
    prm = inter.veryfast_params(qps[1], 1)
    # both reference sets resident before the clock starts: a leg swaps the pointer
    d_ref = {False: ip.d_ref}
    for i in range(n):
        ip.upload(i, pictures[1], refs[False], cu0)
    if has_lists:
        d_ref[True] = ip.dev.empty(n * ip.fs)
        for i in range(n):
            lib.kvz_hip_dev_upload(d_ref[True] + i * ip.fs, refs[True].ctypes.data, ip.fs)
    cases = {}
    for name in ("flat", "default", "flat_again") if has_lists else ("flat", "flat_again"):
        lists = name == "default"
        ip.d_ref = d_ref[lists]
        if has_lists:
            ip.set_scaling_lists([ScalingLists.default(lib)] if lists else [])
        pass_ms = []
        for k in range(args.warmup + args.steps):
            ip.run(prm)
            if k >= args.warmup:
                pass_ms.append(round(float(lib.kvz_hip_dev_inter_kernel_ms()), 3))
        cases[name] = {"pass_device_ms": pass_ms}
        (_, cu_first), (_, cu_last) = ip.download(0), ip.download(n - 1)
        want = gold if lists else flat_gold
        ok[name + "_cu_decisions"] = inter.cu_digest(cu_first) == want["cu"][1] and np.array_equal(cu_first, cu_last)
        if lists:
            ip.loop_filters(prm)
            ok["default_final_picture"] = sha(ip.download(0)[0]) == gold["rec"][1] and np.array_equal(ip.download(0)[0], ip.download(n - 1)[0])
    med = {k: float(np.median(v["pass_device_ms"])) for k, v in cases.items()}
    out = {"metric": "inter_scaling_lists_cost", "sequences": n, "width": w, "height": h, "qp": qp, "picture_qp": qps[1], "ctus": n * ip.ctus, "steps": args.steps, "has_lists": has_lists,
           "cases": cases, "median_pass_ms": med, "pass_ctus_per_s": {k: n * ip.ctus / (v * 1e-3) for k, v in med.items()}, "flat_again_over_flat": med["flat_again"] / med["flat"],
           "verify": {k: bool(v) for k, v in ok.items()}, "verified": bool(all(ok.values()))}
    if has_lists:
        out["pass_default_over_flat"] = med["default"] / med["flat"]
    print(json.dumps(out))
    ip.d_ref = d_ref[False]
    if has_lists:
        ip.dev.free(d_ref[True])
    ip.close()
    return 0 if out["verified"] else 1


if __name__ == "__main__":
    sys.exit(main())
