#!/usr/bin/env python3
"""What joining the inter CTU passes of B pictures of different sizes into ONE launch (kvz_hip_dev_inter_ctu_pass_groups, kvazaar_amd.inter.InterGroup) buys, and
that the launches of one size cost what they cost before.

--mix: the first B picture (`--preset veryfast --gop lp-g4d3t1 -q 22`: picture QP 25, POC 1, as BASELINE config 4) of 1920x1080, 832x480 and 3840x2160 sequences
(kvazaar_amd.synth `large` clips, seeds 1, 5, 2; every sequence of a size the same clip, predicted from its I picture through the all-intra pass), in two legs:
  solo    the three sizes' own launches one after the other through kvz_hip_dev_inter_ctu_pass_pictures (the sum of the three device times)
  joint   one launch of the three groups
  --mix thin   24 + 48 + 6 sequences: alone, each size exposes a fraction of the device's workgroup slots' worth of anti-diagonals
  --mix full   192 + 384 + 48: the device is full either way
--baseline: BASELINE config 4's picture (96 resident 3840x2160 sequences) through the unchanged entry point kvz_hip_dev_inter_ctu_pass; with --parent-lib PATH (a
library built from the parent commit) the same measurement is run on that library before and after, each in a child process with KVZ_HIP_LIB=PATH (the method of
tools/bench_inter_scaling_lists.py), and the medians of this library's launches are held against the range of the parent's own launches of the same session.
Times are device times from the HIP events the library records around its launch (kvz_hip_dev_inter_kernel_ms): warm-up launches first, then --steps timed
launches (at least five), their median and their spread (min, max).  Every timed leg is verified: the CU decisions of the 1080p and 2160p pictures against the
reference encoder's (tests/golden/inter_recon.json), the 832x480 ones joint against solo, first and last sequence of every size against each other.
Prints one JSON line; --out FILE merges it into that file under its keys; exit status 1 when a verification fails.
Usage: python tools/bench_inter_joint.py [--mix thin] [--mix full] [--baseline [--parent-lib PATH]] [--steps 5] [--warmup 1] [--out profiles/inter_joint_pass.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(1920, 1080, 1, "survey-1080p"), (832, 480, 5, None), (3840, 2160, 2, "baseline-c4-2160p")]  # width, height, synth seed, the golden clip of the size
MIXES = {"thin": (24, 48, 6), "full": (192, 384, 48)}
QP = 22


def i_picture(lib, w, h, frame, qp):
    """the I picture through the all-intra pass and its loop filters on the device -> the final picture"""
    from kvazaar_amd.batch import HipBatch, cost_model
    b = HipBatch(lib, w, h, 1)
    try:
        b.upload(0, frame)
        model = cost_model(lib, qp)
        b.launch(model)
        b.loop_filters(model, deblock=True, sao=True)
        return b.download(0)["rec"]
    finally:
        b.close()


def resident(lib, w, h, seed, n):
    """picture 1 of n copies of the size's sequence, resident: source, the I picture as reference, its CU info"""
    from kvazaar_amd import inter, synth
    pictures = [np.concatenate([p.reshape(-1) for p in planes]) for planes in synth.frames(w, h, 2, seed, "large")]
    ref = i_picture(lib, w, h, pictures[0], inter.lowdelay_picture_qp(QP, 0))
    ip = inter.InterPictures(lib, w, h, n)
    cu0 = inter.intra_picture_cu_info(w, h)
    for i in range(n):
        ip.upload(i, pictures[1], ref, cu0)
    return ip


def stats(ms):
    return {"launches_ms": [round(v, 3) for v in ms], "median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def decisions(ip):
    from kvazaar_amd import inter
    (_, first), (_, last) = ip.download(0), ip.download(ip.n - 1)
    return inter.cu_digest(first), bool(np.array_equal(first, last))


def run_mix(lib, name, args, gold):
    from kvazaar_amd import inter
    members = [resident(lib, w, h, seed, n) for (w, h, seed, _), n in zip(SIZES, MIXES[name])]
    picture_qp = inter.lowdelay_picture_qp(QP, 1)
    prm = inter.veryfast_params(picture_qp, 1)
    tables = [inter.InterPictureParams([picture_qp] * m.n, [1] * m.n) for m in members]
    group = inter.InterGroup(lib, members)
    solo, solo_parts, joint, ok = [], [], [], {}
    for k in range(args.warmup + args.steps):
        parts = []
        for m, t in zip(members, tables):
            m.run(prm, pictures=t)  # kvz_hip_dev_inter_ctu_pass_pictures
            parts.append(float(lib.kvz_hip_dev_inter_kernel_ms()))
        if k >= args.warmup:
            solo.append(sum(parts))
            solo_parts.append([round(v, 3) for v in parts])
    solo_cu = [decisions(m) for m in members]
    for m in members:  # the joint leg must write every picture again
        zeros = np.zeros(m.n * m.cells * inter.CU_DTYPE.itemsize, np.uint8)
        lib.kvz_hip_dev_upload(m.d_cu, zeros.ctypes.data, zeros.nbytes)
    for k in range(args.warmup + args.steps):
        if group.run(prm, tables) != 0:
            raise RuntimeError("the joint launch failed")
        if k >= args.warmup:
            joint.append(float(lib.kvz_hip_dev_inter_kernel_ms()))
    joint_cu = [decisions(m) for m in members]
    for (w, h, _, clip), s, j in zip(SIZES, solo_cu, joint_cu):
        ok[f"{w}x{h}"] = s[1] and j[1] and s[0] == j[0] and (clip is None or s[0] == gold[clip]["cu"][1])
    ctus = [m.ctus * m.n for m in members]
    group.close()
    for m in members:
        m.close()
    out = {"sequences": list(MIXES[name]), "ctus": ctus, "picture_qp": picture_qp, "solo": stats(solo), "solo_launches_ms": solo_parts, "joint": stats(joint)}
    out["joint_over_solo"] = out["joint"]["median_ms"] / out["solo"]["median_ms"]
    out["ctus_per_s"] = {k: sum(ctus) / (out[k]["median_ms"] * 1e-3) for k in ("solo", "joint")}
    out["verify"], out["verified"] = ok, all(ok.values())
    return out


def run_baseline(lib, args, gold):
    """BASELINE config 4's picture through kvz_hip_dev_inter_ctu_pass, the entry point every launch of one size goes through"""
    from kvazaar_amd import inter
    w, h, seed, clip = SIZES[2]
    ip = resident(lib, w, h, seed, args.sequences)
    prm = inter.veryfast_params(inter.lowdelay_picture_qp(QP, 1), 1)
    ms = []
    for k in range(args.warmup + args.steps):
        ip.run(prm)
        if k >= args.warmup:
            ms.append(float(lib.kvz_hip_dev_inter_kernel_ms()))
    digest, same = decisions(ip)
    out = dict(stats(ms), sequences=args.sequences, ctus=ip.ctus * ip.n, verified=bool(same and digest == gold[clip]["cu"][1]))
    ip.close()
    return out


def parent_baseline(args):
    """the same measurement on the parent's library, in a child process of its own"""
    env = dict(os.environ, KVZ_HIP_LIB=os.path.abspath(args.parent_lib))
    line = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--baseline", "--steps", str(args.steps), "--warmup", str(args.warmup), "--sequences", str(args.sequences)],
                                   env=env, text=True).strip().splitlines()[-1]
    return json.loads(line)["baseline"]["this"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mix", action="append", choices=list(MIXES), default=[])
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--sequences", type=int, default=96)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.steps < 5:
        ap.error("medians of at least five timed launches")
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "inter_recon.json")))
    out = {"metric": "inter_joint_pass", "qp": QP, "steps": args.steps, "warmup": args.warmup}
    before = parent_baseline(args) if args.baseline and args.parent_lib else None  # (before this process opens the device: one process at a time)
    import kvazaar_amd
    lib = kvazaar_amd.load_library()
    lib.kvz_hip_dev_inter_kernel_ms.restype = C.c_float
    if args.mix:
        out["mixes"] = {name: run_mix(lib, name, args, gold) for name in args.mix}
    if args.baseline:
        base = {"this": run_baseline(lib, args, gold)}
        if before is not None:
            after = parent_baseline(args)
            launches = before["launches_ms"] + after["launches_ms"]
            base["parent"] = {"before": before, "after": after, "range_ms": [min(launches), max(launches)], "verified": before["verified"] and after["verified"]}
            base["this_median_inside_the_parents_range"] = bool(min(launches) <= base["this"]["median_ms"] <= max(launches))
        out["baseline"] = base
    ok = all(m["verified"] for m in out.get("mixes", {}).values()) and all(v.get("verified", True) for v in out.get("baseline", {}).values() if isinstance(v, dict))
    out["verified"] = bool(ok)
    print(json.dumps(out))
    if args.out:
        merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
        for k, v in out.items():
            if isinstance(v, dict) and isinstance(merged.get(k), dict):
                merged[k].update(v)
            elif k == "verified":
                merged[k] = bool(merged.get(k, True) and v)
            else:
                merged[k] = v
        json.dump(merged, open(args.out, "w"), indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
