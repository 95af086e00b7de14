#!/usr/bin/env python3
"""What reference lists cost a P picture (kvazaar's --no-bipred --ref N: kvz_hip_dev_inter_ctu_pass_refs / _entropy_code_inter_refs) beside the single-reference P
picture of the same input, on BASELINE config 4's pictures: --sequences resident 3840x2160 `veryfast` sequences (tools/bench_inter_joint.py's workload, -q 22 under
the low-delay GOP's picture QPs), encoded on the device up to the measured picture -- I picture, then P pictures whose finished pictures move into the resident pool
(InterPictures.advance_pool).

--refs       POC 2, the first picture with two pictures to refer to: the single-reference P pass (kvz_hip_dev_inter_ctu_pass_slices from POC 1), the REFS build with
             the list [1] and with the list [1, 0] (--ref 2); POC 3: the REFS build with [2], [2, 1] and [2, 1, 0] (--ref 3 under --gop 0).  The entropy coder alone
             (after the loop filters) on the outputs of the single-reference P launch, of the --ref 2 launch and of the --ref 3 launch.  Ratios to the
             single-reference launch of the same picture.
--baseline   the default B launch (kvz_hip_dev_inter_ctu_pass) and the single-reference P launch (kvz_hip_dev_inter_ctu_pass_slices) of tools/bench_inter_p.py;
             with --parent-lib PATH (a library built from the parent commit) the same launches on that library before and after, each in a child process with
             KVZ_HIP_LIB=PATH; this library's medians are held against the range of the parent's own launches.
--reference  (no GPU) the reference encoder's own wall time for --ref 1, 2 and 3 on the same four pictures with --no-bipred --gop 0, on the host CPUs, minus the I
             picture's encode: for orientation only.
Pass times are device times from the HIP events the library records around its launch (kvz_hip_dev_inter_kernel_ms); coder times are the host's clock around the
call.  --warmup launches, then --steps timed ones (at least five), their median and spread.  There is no encoder-level truth at this size
(tests/test_gpu_inter_refs.py holds the path against the reference encoder on small clips): first and last sequence must agree, the REFS build with a list of one
must decide what the single-reference P build decides, and a longer list must decide otherwise.
Prints one JSON line; --out FILE merges it into that file.
Usage: python tools/bench_inter_refs.py [--refs] [--baseline [--parent-lib PATH]] [--reference] [--out profiles/inter_refs_cost.json]"""
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

import bench_inter_joint as bj  # noqa: E402  (the workload: i_picture(), stats(), decisions())
import bench_inter_p as bp  # noqa: E402  (the default B launch and the timed loops)

W, H, SEED, CLIP = bj.SIZES[2]
I_SLOT = 1  # the pool's slots: POC 1 goes to slot 0 -- where the single-reference entry points look for "the reference picture" --, the I picture to slot 1, POC 2 to slot 2


def sources():
    from kvazaar_amd import synth
    return [np.concatenate([p.reshape(-1) for p in planes]) for planes in synth.frames(W, H, 4, SEED, "large")]


def prm_of(poc):
    from kvazaar_amd import inter
    return inter.veryfast_params(inter.lowdelay_picture_qp(bj.QP, poc), poc)


def table(ip, poc, slots, slot_poc, ref_pocs_of):
    """every sequence's picture `poc` with the list of the pool slots `slots`"""
    from kvazaar_amd import inter
    frame_pocs, frame_refs = [], []
    for s in range(ip.pool):
        for i in range(ip.n):
            frame_pocs.append(slot_poc.get(s, -1 - s))
            frame_refs.append(ref_pocs_of.get(slot_poc.get(s), []))
    lists = [[ip.pool_frame(s, i) for s in slots] for i in range(ip.n)]
    refs = inter.InterReferences(frame_pocs, frame_refs, [len(slots)] * ip.n, lists)
    return inter.InterPictureParams([prm_of(poc).qp] * ip.n, [poc] * ip.n, references=refs)


def timed(lib, ip, args, launch):
    ms = []
    for k in range(args.warmup + args.steps):
        launch()
        if k >= args.warmup:
            ms.append(float(lib.kvz_hip_dev_inter_kernel_ms()))
    digest, same = bj.decisions(ip)
    print("pass", [round(v, 1) for v in ms], "ms", file=sys.stderr, flush=True)
    return dict(bj.stats(ms), sequences=ip.n, first_equals_last=bool(same)), digest


def timed_coder(ip, args, filters, code):
    filters()
    ip.sync()
    ms, size = [], 0
    for k in range(args.warmup + args.steps):
        t = time.perf_counter()
        data, _ = code()
        if k >= args.warmup:
            ms.append((time.perf_counter() - t) * 1e3)
        size = len(data)
    print("coder", [round(v, 1) for v in ms], "ms", file=sys.stderr, flush=True)
    return dict(bj.stats(ms), slice_data_bytes=int(size))


def run_refs(lib, args):
    from kvazaar_amd import inter
    src = sources()
    n = args.sequences
    final0 = bj.i_picture(lib, W, H, src[0], inter.lowdelay_picture_qp(bj.QP, 0))
    ip = inter.InterPictures(lib, W, H, n, with_levels=True, pool=3)
    cu0 = inter.intra_picture_cu_info(W, H)
    for i in range(n):
        ip.upload_pool(I_SLOT, i, final0, cu0)
        ip.upload_source(i, src[1])
    slot_poc, ref_pocs_of = {I_SLOT: 0}, {0: []}
    out = {}
    # POC 1, untimed: the one picture there is to refer to
    t1 = table(ip, 1, [I_SLOT], slot_poc, ref_pocs_of)
    ip.run(prm_of(1), pictures=t1, slice_type="P")
    ip.loop_filters(prm_of(1), pictures=t1, slice_type="P")
    ip.advance_pool(0)
    slot_poc[0], ref_pocs_of[1] = 1, [0]
    # POC 2
    for i in range(n):
        ip.upload_source(i, src[2])
    prm = prm_of(2)
    one, two = table(ip, 2, [0], slot_poc, ref_pocs_of), table(ip, 2, [0, I_SLOT], slot_poc, ref_pocs_of)
    p, digest_p = timed(lib, ip, args, lambda: ip.run(prm, slice_type="P"))
    out["poc2_pass_p"] = p
    out["poc2_coder_p"] = timed_coder(ip, args, lambda: ip.loop_filters(prm, slice_type="P"), lambda: ip.entropy_code(prm, slice_type="P"))
    r1, digest_1 = timed(lib, ip, args, lambda: ip.run(prm, pictures=one, slice_type="P"))
    r1["decides_what_the_p_build_decides"] = bool(digest_1 == digest_p)
    out["poc2_pass_refs_list_of_1"] = r1
    r2, digest_2 = timed(lib, ip, args, lambda: ip.run(prm, pictures=two, slice_type="P"))
    cu = ip.download(0)[1]
    r2["differs_from_list_of_1"] = bool(digest_2 != digest_1)
    r2["cus_4x4_units_with_ref_idx_1"] = int(((cu["type"] == 2) & (cu["mv_ref"][..., 0] == 1)).sum())
    out["poc2_pass_refs_list_of_2"] = r2
    out["poc2_coder_refs_list_of_2"] = timed_coder(ip, args, lambda: ip.loop_filters(prm, pictures=two, slice_type="P"), lambda: ip.entropy_code(prm, pictures=two, slice_type="P"))
    out["poc2_pass_ref2_over_p"] = r2["median_ms"] / p["median_ms"]
    out["poc2_pass_refs_build_over_p_build_at_one_reference"] = r1["median_ms"] / p["median_ms"]
    out["poc2_coder_ref2_over_p"] = out["poc2_coder_refs_list_of_2"]["median_ms"] / out["poc2_coder_p"]["median_ms"]
    ip.advance_pool(2)  # (the --ref 2 picture after its loop filters)
    slot_poc[2], ref_pocs_of[2] = 2, [1, 0]
    # POC 3
    for i in range(n):
        ip.upload_source(i, src[3])
    prm = prm_of(3)
    results = {}
    for name, slots in (("1", [2]), ("2", [2, 0]), ("3", [2, 0, I_SLOT])):
        t = table(ip, 3, slots, slot_poc, ref_pocs_of)
        results[name], _ = timed(lib, ip, args, lambda: ip.run(prm, pictures=t, slice_type="P"))
        out[f"poc3_pass_refs_list_of_{name}"] = results[name]
        if name != "2":
            out[f"poc3_coder_refs_list_of_{name}"] = timed_coder(ip, args, lambda: ip.loop_filters(prm, pictures=t, slice_type="P"), lambda: ip.entropy_code(prm, pictures=t, slice_type="P"))
    cu = ip.download(0)[1]
    out["poc3_pass_refs_list_of_3"]["cus_4x4_units_with_ref_idx_2"] = int(((cu["type"] == 2) & (cu["mv_ref"][..., 0] == 2)).sum())
    out["poc3_pass_ref2_over_one_reference"] = results["2"]["median_ms"] / results["1"]["median_ms"]
    out["poc3_pass_ref3_over_one_reference"] = results["3"]["median_ms"] / results["1"]["median_ms"]
    out["poc3_coder_ref3_over_one_reference"] = out["poc3_coder_refs_list_of_3"]["median_ms"] / out["poc3_coder_refs_list_of_1"]["median_ms"]
    ip.close()
    return out


def run_baseline(lib, args, gold):
    ip = bj.resident(lib, W, H, SEED, args.sequences)
    b, digest = bp.timed_pass(lib, ip, bp.params(), args, None)
    b["verified"] = bool(b["first_equals_last"] and digest == gold[CLIP]["cu"][1])
    p, _ = bp.timed_pass(lib, ip, bp.params(), args, "P")
    ip.close()
    return {"b": b, "p": p}


def child(args, lib_path):
    """this tool's baseline launches on another library, in a child process of its own"""
    env = dict(os.environ, KVZ_HIP_LIB=os.path.abspath(lib_path))
    cmd = [sys.executable, os.path.abspath(__file__), "--baseline-only", "--steps", str(args.steps), "--warmup", str(args.warmup), "--sequences", str(args.sequences)]
    return json.loads(subprocess.check_output(cmd, env=env, text=True).strip().splitlines()[-1])["baseline_only"]


def run_reference(args):
    """wall time of oracle/_ref/kvazaar_ref on the four pictures with --no-bipred --gop 0 under --ref 1, 2 and 3, minus the I picture's encode"""
    exe = os.path.join(ROOT, "oracle", "_ref", "kvazaar_ref")
    frames = sources()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "in.yuv")
        open(src, "wb").write(b"".join(f.tobytes() for f in frames))

        def encode(n, extra):
            cmd = [exe, "-i", src, "--input-res", f"{W}x{H}", "--preset", "veryfast", "--gop", "0", "-q", str(bj.QP), "-n", str(n), "-o", os.path.join(d, "out.hevc"),
                   "--threads", str(args.reference_threads), "--owf", "0", "--no-bipred"] + list(extra)
            t = time.perf_counter()
            subprocess.run(cmd, check=True, capture_output=True)
            return time.perf_counter() - t

        intra = min(encode(1, ()) for _ in range(2))
        for ref in (1, 2, 3):
            out[f"ref{ref}"] = {"three_p_pictures_s": min(encode(4, ("--ref", str(ref))) for _ in range(2)) - intra}
            out[f"ref{ref}"]["over_ref1"] = out[f"ref{ref}"]["three_p_pictures_s"] / out["ref1"]["three_p_pictures_s"]
            print("reference --ref", ref, out[f"ref{ref}"], file=sys.stderr, flush=True)
    return {"threads": args.reference_threads, "i_picture_s": intra, "options": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", action="store_true")
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--baseline-only", action="store_true", help="(child of --parent-lib) the baseline launches on the library under KVZ_HIP_LIB")
    ap.add_argument("--parent-lib")
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--reference-threads", type=int, default=8)
    ap.add_argument("--sequences", type=int, default=96)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.steps < 5:
        ap.error("medians of at least five timed launches")
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "inter_recon.json")))
    out = {"metric": "inter_refs_cost", "qp": bj.QP, "steps": args.steps, "warmup": args.warmup}
    if args.reference:
        out["reference_encoder"] = run_reference(args)
    # (children first and last, this process's device work between them: one process on the device at a time)
    before = child(args, args.parent_lib) if args.baseline and args.parent_lib else None
    if args.refs or args.baseline or args.baseline_only:
        import kvazaar_amd
        lib = kvazaar_amd.load_library()
        lib.kvz_hip_dev_inter_kernel_ms.restype = C.c_float
        if args.baseline_only:
            out["baseline_only"] = run_baseline(lib, args, gold)
        if args.refs:
            out["refs"] = run_refs(lib, args)
        if args.baseline:
            base = {"this": run_baseline(lib, args, gold)}
            if before is not None:
                after = child(args, args.parent_lib)
                base["parent"] = {"before": before, "after": after}
                for kind in ("b", "p"):
                    launches = before[kind]["launches_ms"] + after[kind]["launches_ms"]
                    base[f"parent_{kind}_range_ms"] = [min(launches), max(launches)]
                    base[f"this_{kind}_range_ms"] = [base["this"][kind]["min_ms"], base["this"][kind]["max_ms"]]
                    base[f"this_{kind}_median_inside_the_parents_range"] = bool(min(launches) <= base["this"][kind]["median_ms"] <= max(launches))
            out["baseline"] = base
    print(json.dumps(out))
    if args.out:
        merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
        merged.update(out)
        json.dump(merged, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
