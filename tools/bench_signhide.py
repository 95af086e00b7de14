#!/usr/bin/env python3
"""What sign data hiding (kvz_hip_intra_cost_model::signhide, kvazaar's --signhide) costs in the all-intra CTU pass and in the entropy coder.

1 536 resident 1080p pictures (bench.py's clip and batch size: kvazaar_amd.synth, seed 1, eight distinct frames cycled), `ultrafast` QP 22, the same batch under the
model without the switch (kvz_hip_intra_frames -> the fast-estimate instantiation) and with it (-> the sign-hiding instantiation).  Times of the pass are device times
from the HIP events the library records on the batch's own stream around its launch (kvz_hip_batch_last_kernel_ms), warm-up launches first; the entropy coder alone
(kvz_hip_batch_entropy_code on the levels the pass just left) is timed by the host's clock over the call, which ends with the slice data on the host.  The timed
launches are verified: the first eight pictures of the last launch with the switch against the reference encoder's --signhide reconstructions
(tests/golden/signhide.json), those without it against tests/golden/encoder_recon.json.
Prints one JSON line; exit status 1 when a verification fails.  Usage: python tools/bench_signhide.py [--frames 1536] [--steps 3] [--warmup 1] [--qp 22]"""
import argparse
import hashlib
import json
import os
import sys
import time

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
    from kvazaar_amd.batch import HipBatch, cost_model
    lib = kvazaar_amd.load_library()
    w, h, n = args.width, args.height, args.frames
    clip = [np.concatenate([p.reshape(-1) for p in planes]) for planes in synth.frames(w, h, args.distinct, 1, "large")]
    batch = HipBatch(lib, w, h, n)
    for i in range(n):
        batch.upload(i, clip[i % len(clip)])
    plain, hidden = cost_model(lib, args.qp), cost_model(lib, args.qp)
    hidden.signhide = 1
    cases = {}
    digests = {}
    for name, model in (("plain", plain), ("signhide", hidden), ("plain_again", plain)):
        pass_ms, coder_ms, nbytes = [], [], 0
        for k in range(args.warmup + args.steps):
            if batch.launch(model) < 0:
                raise RuntimeError("launch refused")
            batch.sync()
            ms = batch.kernel_ms()
            t0 = time.perf_counter()
            data, sizes = batch.entropy_code(model)
            t1 = time.perf_counter()
            nbytes = len(data)
            if k >= args.warmup:
                pass_ms.append(round(float(ms), 3))
                coder_ms.append(round((t1 - t0) * 1e3, 3))
        cases[name] = {"pass_device_ms": pass_ms, "coder_wall_ms": coder_ms, "slice_bytes": nbytes}
        digests[name] = [sha(batch.download(i)["rec"]) for i in range(min(n, len(clip)))]
    ok = None
    if (w, h, args.qp, args.distinct) == (1920, 1080, 22, 8):  # the pictures the fixtures hold
        gold = json.load(open(os.path.join(ROOT, "tests", "golden", "signhide.json")))["ultrafast-1920x1080-qp22"]["rec"]
        recon = json.load(open(os.path.join(ROOT, "tests", "golden", "encoder_recon.json")))["1920x1080/n8/seed1/large/qp22/nodeblock"]
        k = min(n, 8)
        ok = digests["signhide"] == gold[:k] and digests["plain"] == recon[:k] and digests["plain_again"] == recon[:k]
    ctus = batch.ctus_per_frame * n
    med = {k: {"pass_ms": float(np.median(v["pass_device_ms"])), "coder_ms": float(np.median(v["coder_wall_ms"]))} for k, v in cases.items()}
    rate = {k: ctus / (v["pass_ms"] * 1e-3) for k, v in med.items()}
    print(json.dumps({"metric": "signhide_cost", "frames": n, "width": w, "height": h, "qp": args.qp, "ctus": ctus, "steps": args.steps, "cases": cases, "median": med,
                      "pass_ctus_per_s": rate, "pass_fps": {k: n / (v["pass_ms"] * 1e-3) for k, v in med.items()},
                      "pass_signhide_over_plain": med["signhide"]["pass_ms"] / med["plain"]["pass_ms"],
                      "coder_signhide_over_plain": med["signhide"]["coder_ms"] / med["plain"]["coder_ms"],
                      "slice_bytes_signhide_over_plain": cases["signhide"]["slice_bytes"] / cases["plain"]["slice_bytes"], "verified": ok}))
    batch.close()
    return 0 if ok in (None, True) else 1


if __name__ == "__main__":
    sys.exit(main())
