#!/usr/bin/env python3
"""What per-coefficient scaling lists (kvz_hip_batch_set_scaling_lists, kvazaar's --scaling-list default) cost in the all-intra CTU pass.

1 536 resident 1080p pictures (bench.py's clip and batch size: kvazaar_amd.synth, seed 1, eight distinct frames cycled), `ultrafast` QP 22, the same batch in three
legs: `flat` (no lists: the fast-estimate instantiation of every batch without them), `default` (every picture under the default lists: the LISTS instantiation) and
`flat_again` (the lists cleared).  Times are device times from the HIP events the library records on the batch's own stream around its launch
(kvz_hip_batch_last_kernel_ms), warm-up launches first.  The timed launches are verified: the first eight pictures of the `default` leg against the reference
encoder's --scaling-list default reconstructions (tests/golden/scaling_lists.json), those of the flat legs against tests/golden/encoder_recon.json.
A library without the entry point (an older build, timed for comparison through KVZ_HIP_LIB) runs the flat legs only.
Prints one JSON line; exit status 1 when a verification fails.  Usage: python tools/bench_scaling_lists.py [--frames 1536] [--steps 3] [--warmup 1] [--qp 22]"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1536)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--qp", type=int, default=22)
    args = ap.parse_args()
    import kvazaar_amd
    from kvazaar_amd import synth
    from kvazaar_amd.batch import HipBatch, ScalingLists, cost_model
    lib = kvazaar_amd.load_library()
    has_lists = hasattr(lib, "kvz_hip_batch_set_scaling_lists")
    w, h, n = args.width, args.height, args.frames
    clip = [np.concatenate([p.reshape(-1) for p in planes]) for planes in synth.frames(w, h, args.distinct, 1, "large")]
    batch = HipBatch(lib, w, h, n)
    for i in range(n):
        batch.upload(i, clip[i % len(clip)])
    model = cost_model(lib, args.qp)
    cases, digests = {}, {}
    for name in ("flat", "default", "flat_again") if has_lists else ("flat", "flat_again"):
        if has_lists:
            batch.set_scaling_lists([ScalingLists.default(lib)] if name == "default" else [])
        pass_ms = []
        for k in range(args.warmup + args.steps):
            if batch.launch(model) < 0:
                raise RuntimeError("launch refused")
            batch.sync()
            if k >= args.warmup:
                pass_ms.append(round(float(batch.kernel_ms()), 3))
        cases[name] = {"pass_device_ms": pass_ms}
        digests[name] = [sha(batch.download(i)["rec"]) for i in range(min(n, len(clip)))]
    ok = None
    if (w, h, args.qp, args.distinct) == (1920, 1080, 22, 8):  # the pictures the fixtures hold
        recon = json.load(open(os.path.join(ROOT, "tests", "golden", "encoder_recon.json")))["1920x1080/n8/seed1/large/qp22/nodeblock"]
        k = min(n, 8)
        ok = digests["flat"] == recon[:k] and digests["flat_again"] == recon[:k]
        if has_lists:
            gold = json.load(open(os.path.join(ROOT, "tests", "golden", "scaling_lists.json")))["ultrafast-1920x1080-qp22"]["rec"]
            ok = ok and digests["default"] == gold[:k]
    ctus = batch.ctus_per_frame * n
    med = {k: float(np.median(v["pass_device_ms"])) for k, v in cases.items()}
    out = {"metric": "scaling_lists_cost", "frames": n, "width": w, "height": h, "qp": args.qp, "ctus": ctus, "steps": args.steps, "has_lists": has_lists, "cases": cases,
           "median_pass_ms": med, "pass_fps": {k: n / (v * 1e-3) for k, v in med.items()}, "flat_again_over_flat": med["flat_again"] / med["flat"], "verified": ok}
    if has_lists:
        out["pass_default_over_flat"] = med["default"] / med["flat"]
    print(json.dumps(out))
    batch.close()
    return 0 if ok in (None, True) else 1


if __name__ == "__main__":
    sys.exit(main())
