#!/usr/bin/env python3
"""What a P picture (kvazaar's --no-bipred: kvz_hip_dev_inter_ctu_pass_slices with KVZ_HIP_SLICE_P) costs beside the B picture of the same input, on BASELINE config
4's picture: the first inter picture (`--preset veryfast --gop lp-g4d3t1 -q 22`: picture QP 25, POC 1) of --sequences resident 3840x2160 sequences
(tools/bench_inter_joint.py's workload).

--slices     the pass as P and as B on the same resident pictures in the same process, and the entropy coder alone (after the slice type's loop filters) on the P
             and on the B outputs of that launch; P as a ratio to B.
--baseline   the default B launch through kvz_hip_dev_inter_ctu_pass; with --parent-lib PATH (a library built from the parent commit) the same launch on that
             library before and after, each in a child process with KVZ_HIP_LIB=PATH; this library's median is held against the range of the parent's own launches.
Pass times are device times from the HIP events the library records around its launch (kvz_hip_dev_inter_kernel_ms); coder times are the host's clock around the
call, which returns with the slice data downloaded.  --warmup launches, then --steps timed ones (at least five), their median and spread.  The B launch's decisions
are verified against tests/golden/inter_recon.json; the P launch has no encoder-level truth at this size (tests/test_gpu_inter_p.py holds it against the reference
encoder on small clips): first and last sequence must agree, every inter record must move by list 0 alone, and the decisions must differ from B's.
Prints one JSON line; --out FILE merges it into that file.
Usage: python tools/bench_inter_p.py [--slices] [--baseline [--parent-lib PATH]] [--out profiles/inter_p_slices_cost.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_inter_joint as bj  # noqa: E402  (the workload: i_picture(), stats(), decisions())

W, H, SEED, CLIP = bj.SIZES[2]


def params():
    from kvazaar_amd import inter
    return inter.veryfast_params(inter.lowdelay_picture_qp(bj.QP, 1), 1)


def resident_with_levels(lib, n):
    """bj.resident with the levels' buffer the entropy coder reads"""
    from kvazaar_amd import inter, synth
    pictures = [np.concatenate([p.reshape(-1) for p in planes]) for planes in synth.frames(W, H, 2, SEED, "large")]
    ref = bj.i_picture(lib, W, H, pictures[0], inter.lowdelay_picture_qp(bj.QP, 0))
    ip = inter.InterPictures(lib, W, H, n, with_levels=True)
    cu0 = inter.intra_picture_cu_info(W, H)
    for i in range(n):
        ip.upload(i, pictures[1], ref, cu0)
    return ip


def timed_pass(lib, ip, prm, args, slice_type):
    ms = []
    for k in range(args.warmup + args.steps):
        if slice_type is None:
            ip.run(prm)
        else:
            ip.run(prm, slice_type=slice_type)
        if k >= args.warmup:
            ms.append(float(lib.kvz_hip_dev_inter_kernel_ms()))
    digest, same = bj.decisions(ip)
    return dict(bj.stats(ms), sequences=ip.n, first_equals_last=bool(same)), digest


def timed_coder(ip, prm, args, slice_type):
    """the slice type's loop filters once (the coder writes their SAO decisions), then the coder alone"""
    ip.loop_filters(prm, slice_type=slice_type)
    ip.sync()
    ms, size = [], 0
    for k in range(args.warmup + args.steps):
        t = time.perf_counter()
        data, _ = ip.entropy_code(prm, slice_type=slice_type)
        if k >= args.warmup:
            ms.append((time.perf_counter() - t) * 1e3)
        size = len(data)
    return dict(bj.stats(ms), slice_data_bytes=int(size))


def run_slices(lib, args, gold):
    ip = resident_with_levels(lib, args.sequences)
    prm = params()
    out = {}
    b, digest_b = timed_pass(lib, ip, prm, args, None)
    b["verified"] = bool(b["first_equals_last"] and digest_b == gold[CLIP]["cu"][1])
    out["pass_b"] = b
    out["coder_b"] = timed_coder(ip, prm, args, "B")
    p, digest_p = timed_pass(lib, ip, prm, args, "P")
    cu = ip.download(0)[1]
    p["list0_only"] = bool((cu["mv_dir"][cu["type"] == 2] == 1).all())
    p["differs_from_b"] = bool(digest_p != digest_b)
    out["pass_p"] = p
    out["coder_p"] = timed_coder(ip, prm, args, "P")
    out["pass_p_over_b"] = p["median_ms"] / b["median_ms"]
    out["coder_p_over_b"] = out["coder_p"]["median_ms"] / out["coder_b"]["median_ms"]
    ip.close()
    return out


def run_baseline(lib, args, gold):
    ip = bj.resident(lib, W, H, SEED, args.sequences)
    r, digest = timed_pass(lib, ip, params(), args, None)
    r["verified"] = bool(r["first_equals_last"] and digest == gold[CLIP]["cu"][1])
    ip.close()
    return r


def child(args, lib_path):
    """this tool's default B launch on another library, in a child process of its own"""
    env = dict(os.environ, KVZ_HIP_LIB=os.path.abspath(lib_path))
    cmd = [sys.executable, os.path.abspath(__file__), "--baseline-only", "--steps", str(args.steps), "--warmup", str(args.warmup), "--sequences", str(args.sequences)]
    return json.loads(subprocess.check_output(cmd, env=env, text=True).strip().splitlines()[-1])["baseline_only"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", action="store_true")
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--baseline-only", action="store_true", help="(child of --parent-lib) the default B launch on the library under KVZ_HIP_LIB")
    ap.add_argument("--parent-lib")
    ap.add_argument("--sequences", type=int, default=96)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.steps < 5:
        ap.error("medians of at least five timed launches")
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "inter_recon.json")))
    out = {"metric": "inter_p_slices_cost", "qp": bj.QP, "steps": args.steps, "warmup": args.warmup}
    # (children first and last, this process's device work between them: one process on the device at a time)
    before = child(args, args.parent_lib) if args.baseline and args.parent_lib else None
    if args.slices or args.baseline or args.baseline_only:
        import kvazaar_amd
        lib = kvazaar_amd.load_library()
        lib.kvz_hip_dev_inter_kernel_ms.restype = C.c_float
        if args.baseline_only:
            out["baseline_only"] = run_baseline(lib, args, gold)
        if args.slices:
            out["slices"] = run_slices(lib, args, gold)
        if args.baseline:
            base = {"this": run_baseline(lib, args, gold)}
            if before is not None:
                after = child(args, args.parent_lib)
                launches = before["launches_ms"] + after["launches_ms"]
                base["parent"] = {"before": before, "after": after, "range_ms": [min(launches), max(launches)], "verified": before["verified"] and after["verified"]}
                base["this_range_ms"] = [base["this"]["min_ms"], base["this"]["max_ms"]]
                base["this_median_inside_the_parents_range"] = bool(min(launches) <= base["this"]["median_ms"] <= max(launches))
            out["baseline"] = base
    print(json.dumps(out))
    if args.out:
        merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
        merged.update(out)
        json.dump(merged, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
