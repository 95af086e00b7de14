#!/usr/bin/env python3
"""What the choice of integer motion search (kvz_hip_inter_params me_algorithm / me_early_termination: kvazaar's --me, --me-early-termination) costs in the inter CTU
pass, on BASELINE config 4's picture: the first B picture (`--preset veryfast --gop lp-g4d3t1 -q 22`: picture QP 25, POC 1) of --sequences resident 3840x2160
sequences (tools/bench_inter_joint.py's workload).

--options    the pass under dia, tz, full8, full16, full32 (full64 on --sequences-full64 sequences), each with --me-early-termination on and off, as a ratio to the
             default search (hexbs, sensitive) at the same number of sequences in the same process.
--window-lib PATH   the full searches with --me-early-termination off on --sequences-windows sequences, on this library and, in a child process, on that one (a
             build whose windows go through probe_group in groups of eight, -DKVZ_ICTU_ME_WINDOW_BY_PROBES while that form existed).
--baseline   three zero members through kvz_hip_dev_inter_ctu_pass; with --parent-lib PATH (a library built from the parent commit) the same launch on that
             library before and after, each in a child process with KVZ_HIP_LIB=PATH and the parent's shorter kvz_hip_inter_params; this library's median is held
             against the range of the parent's own launches.
--reference  (no GPU) the reference encoder's own wall time for the same options on the same two pictures, on the host CPUs: each option's encode minus the
             encode of the I picture alone, as a ratio to hexbs.
Times are device times from the HIP events the library records around its launch (kvz_hip_dev_inter_kernel_ms): --warmup launches, then --steps timed ones (at
least five), their median and spread.  The default search's decisions are verified against tests/golden/inter_recon.json; the others have no encoder-level truth at
this size (tests/test_gpu_inter_me.py holds them against the reference encoder on small clips): first and last sequence must agree.
Prints one JSON line; --out FILE merges it into that file.
Usage: python tools/bench_inter_me.py [--options] [--baseline [--parent-lib PATH]] [--window-lib PATH] [--reference] [--out profiles/inter_me_cost.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_inter_joint as bj  # noqa: E402  (the workload: resident(), stats(), decisions())

W, H, SEED, CLIP = bj.SIZES[2]
ALGORITHMS = ("dia", "tz", "full8", "full16", "full32", "full64")
FULL = ("full8", "full16", "full32")


def params(me="hexbs", term="sensitive", parent_struct=False):
    from kvazaar_amd import inter
    prm = inter.veryfast_params(inter.lowdelay_picture_qp(bj.QP, 1), 1)
    for k, v in inter.me_search_fields(me=me, me_early_termination=term).items():
        setattr(prm, k, v)
    if parent_struct:
        prm.struct_size = C.sizeof(inter.InterParams) - 12  # the parent's struct: this one without its last three members
    return prm


def timed(lib, ip, prm, args):
    ms = []
    for k in range(args.warmup + args.steps):
        ip.run(prm)
        if k >= args.warmup:
            ms.append(float(lib.kvz_hip_dev_inter_kernel_ms()))
    digest, same = bj.decisions(ip)
    return dict(bj.stats(ms), sequences=ip.n, first_equals_last=bool(same)), digest


def run_options(lib, args, gold, names, terms=("on", "off"), full64=True):
    out = {}
    for n, algos in ((args.sequences, [a for a in names if a != "full64"]), (args.sequences_full64, ["full64"] if full64 and "full64" in names else [])):
        if not algos:
            continue
        ip = bj.resident(lib, W, H, SEED, n)
        base, digest = timed(lib, ip, params(), args)
        base["verified"] = bool(base["first_equals_last"] and digest == gold[CLIP]["cu"][1])
        out[f"hexbs@{n}"] = base
        for a in algos:
            for t in terms:
                r, _ = timed(lib, ip, params(a, t), args)
                r["over_hexbs"] = r["median_ms"] / base["median_ms"]
                out[f"{a}/{t}"] = r
                print(a, t, round(r["median_ms"], 2), "ms", round(r["over_hexbs"], 2), "x", file=sys.stderr, flush=True)
        ip.close()
    return out


def run_baseline(lib, args, gold, parent_struct):
    ip = bj.resident(lib, W, H, SEED, args.sequences)
    r, digest = timed(lib, ip, params(parent_struct=parent_struct), args)
    r["verified"] = bool(r["first_equals_last"] and digest == gold[CLIP]["cu"][1])
    ip.close()
    return r


def child(args, lib_path, mode, sequences=None):
    """this tool on another library, in a child process of its own: mode is the leg's flag"""
    env = dict(os.environ, KVZ_HIP_LIB=os.path.abspath(lib_path))
    cmd = [sys.executable, os.path.abspath(__file__), mode, "--steps", str(args.steps), "--warmup", str(args.warmup), "--sequences", str(sequences or args.sequences)]
    return json.loads(subprocess.check_output(cmd, env=env, text=True).strip().splitlines()[-1])


def run_reference(args):
    """wall time of oracle/_ref/kvazaar_ref on the two pictures under every option, minus the I picture's encode"""
    from kvazaar_amd import synth
    exe = os.path.join(ROOT, "oracle", "_ref", "kvazaar_ref")
    frames = [np.concatenate([p.reshape(-1) for p in planes]) for planes in synth.frames(W, H, 2, SEED, "large")]
    out = {}
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "in.yuv")
        open(src, "wb").write(b"".join(f.tobytes() for f in frames))

        def encode(n, extra):
            cmd = [exe, "-i", src, "--input-res", f"{W}x{H}", "--preset", "veryfast", "--gop", "lp-g4d3t1", "-q", str(bj.QP), "-n", str(n), "-o", os.path.join(d, "out.hevc"),
                   "--threads", str(args.reference_threads), "--owf", "0"] + list(extra)
            t = time.perf_counter()
            subprocess.run(cmd, check=True, capture_output=True)
            return time.perf_counter() - t

        intra = min(encode(1, ()) for _ in range(2))
        base = min(encode(2, ()) for _ in range(2)) - intra
        out["hexbs"] = {"b_picture_s": base}
        for a in ALGORITHMS:
            for t in ("on", "off"):
                s = encode(2, ("--me", a, "--me-early-termination", t)) - intra
                out[f"{a}/{t}"] = {"b_picture_s": s, "over_hexbs": s / base}
                print("reference", a, t, round(s, 2), "s", round(s / base, 2), "x", file=sys.stderr, flush=True)
    return {"threads": args.reference_threads, "i_picture_s": intra, "options": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--options", action="store_true")
    ap.add_argument("--full-only", action="store_true", help="(child of --window-lib) the full searches with --me-early-termination off only")
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--parent-struct", action="store_true", help="(child of --parent-lib) the library under KVZ_HIP_LIB takes the parent's kvz_hip_inter_params")
    ap.add_argument("--parent-lib")
    ap.add_argument("--window-lib")
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--reference-threads", type=int, default=8)
    ap.add_argument("--sequences", type=int, default=96)
    ap.add_argument("--sequences-full64", type=int, default=24)
    ap.add_argument("--sequences-windows", type=int, default=48)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.steps < 5:
        ap.error("medians of at least five timed launches")
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "inter_recon.json")))
    out = {"metric": "inter_me_cost", "qp": bj.QP, "steps": args.steps, "warmup": args.warmup}
    if args.reference:
        out["reference_encoder"] = run_reference(args)
    gpu = args.options or args.baseline or args.full_only or args.parent_struct or args.window_lib
    # (children first and last, this process's device work between them: one process on the device at a time)
    before = child(args, args.parent_lib, "--parent-struct")["baseline_parent_struct"] if args.baseline and args.parent_lib else None
    windows = child(args, args.window_lib, "--full-only", args.sequences_windows)["full_only"] if args.window_lib else None
    if gpu:
        import kvazaar_amd
        lib = kvazaar_amd.load_library()
        lib.kvz_hip_dev_inter_kernel_ms.restype = C.c_float
        if args.parent_struct:
            out["baseline_parent_struct"] = run_baseline(lib, args, gold, True)
        if args.full_only:
            out["full_only"] = run_options(lib, args, gold, FULL, terms=("off",), full64=False)
        if args.options:
            out["options"] = run_options(lib, args, gold, ALGORITHMS)
        if windows is not None:  # the two forms of the full search's windows at the same number of sequences
            all_sequences, args.sequences = args.sequences, args.sequences_windows
            sweep = run_options(lib, args, gold, FULL, terms=("off",), full64=False)
            args.sequences = all_sequences
            out["windows"] = {"sequences": args.sequences_windows, "by_probe_group": windows, "by_sweep": sweep,
                              "sweep_over_probe_group": {a: sweep[f"{a}/off"]["median_ms"] / windows[f"{a}/off"]["median_ms"] for a in FULL}}
        if args.baseline:
            base = {"this": run_baseline(lib, args, gold, False)}
            if before is not None:
                after = child(args, args.parent_lib, "--parent-struct")["baseline_parent_struct"]
                launches = before["launches_ms"] + after["launches_ms"]
                base["parent"] = {"before": before, "after": after, "range_ms": [min(launches), max(launches)], "verified": before["verified"] and after["verified"]}
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
