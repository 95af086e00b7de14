#!/usr/bin/env python3
"""What pictures at two QPs cost in ONE launch of the all-intra CTU pass (kvz_hip_intra_frames_models) against what a caller could do before: one launch per QP.

1 536 resident 1080p pictures (bench.py's clip: kvazaar_amd.synth, seed 1, eight distinct frames cycled), four timed cases:
  uniform_qp22 / uniform_qp32   the whole batch under one model (kvz_hip_intra_frames)
  mixed                         even pictures at QP 22, odd ones at QP 32, one launch (kvz_hip_intra_frames_models)
  two_launches                  the same halves as two 768-picture batches launched back to back, each on its stream: `overlapped` = nothing orders them (the second
                                moves into the workgroup slots the first one frees), `serial` = the second ordered behind the first (kvz_hip_batch_order_after)
Times are device times from the HIP events the library records on a batch's own stream around its launch (kvz_hip_batch_last_kernel_ms); for the two overlapped launches
the later-ending one's (it is queued microseconds behind the other and ends last), with the host's wall clock over launch + sync of every case beside it.
Prints one JSON line.  Usage: python tools/bench_mixed_qp.py [--frames 1536] [--steps 3] [--warmup 1] [--qps 22 32]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1536)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--qps", type=int, nargs=2, default=[22, 32])
    args = ap.parse_args()
    import kvazaar_amd
    from kvazaar_amd import synth
    from kvazaar_amd.batch import HipBatch, PictureModels, cost_model
    lib = kvazaar_amd.load_library()
    w, h, n, half = args.width, args.height, args.frames, args.frames // 2
    assert n == 2 * half
    qa, qb = args.qps
    clip = [np.concatenate([p.reshape(-1) for p in planes]) for planes in synth.frames(w, h, args.distinct, 1, "large")]
    whole, first, second = HipBatch(lib, w, h, n), HipBatch(lib, w, h, half), HipBatch(lib, w, h, half)
    # picture i of the whole batch is clip picture i % distinct; the mixed launch runs the even ones at qa and the odd ones at qb, and the two half batches hold exactly
    # those pictures
    for i in range(n):
        whole.upload(i, clip[i % len(clip)])
        (first if i % 2 == 0 else second).upload(i // 2, clip[i % len(clip)])
    ma, mb = cost_model(lib, qa), cost_model(lib, qb)
    mixed = PictureModels(lib, [qa if i % 2 == 0 else qb for i in range(n)])

    def timed(run):
        """-> (device ms per step, wall ms per step)"""
        dev, wall = [], []
        for k in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            ms = run()
            t1 = time.perf_counter()
            if k >= args.warmup:
                dev.append(round(float(ms), 3))
                wall.append(round((t1 - t0) * 1e3, 3))
        return dev, wall

    def one(batch, model):
        def run():
            if batch.launch(model) < 0:
                raise RuntimeError("launch refused")
            batch.sync()
            return batch.kernel_ms()
        return run

    def two(serial):
        def run():
            if serial:
                second.order_after(first)
            first.launch(ma)
            if serial:
                second.order_after(first)
            second.launch(mb)
            first.sync()
            second.sync()
            return first.kernel_ms() + second.kernel_ms() if serial else max(first.kernel_ms(), second.kernel_ms())
        return run

    cases = {}
    for name, run in ((f"uniform_qp{qa}", one(whole, ma)), (f"uniform_qp{qb}", one(whole, mb)), ("mixed", one(whole, mixed)),
                      ("two_launches_overlapped", two(False)), ("two_launches_serial", two(True)), ("mixed_again", one(whole, mixed))):
        dev, wall = timed(run)
        cases[name] = {"device_ms": dev, "wall_ms": wall}
    # the mixed launch computed what the half launches computed: picture hashes of the last runs
    mixed_sums = whole.checksums()
    same = bool(np.array_equal(mixed_sums[0::2], first.checksums()) and np.array_equal(mixed_sums[1::2], second.checksums()))
    med = {k: float(np.median(v["device_ms"])) for k, v in cases.items()}
    ctus = whole.ctus_per_frame * n
    best_two = min(med["two_launches_overlapped"], med["two_launches_serial"])
    uniform_mean = 0.5 * (med[f"uniform_qp{qa}"] + med[f"uniform_qp{qb}"])
    print(json.dumps({"metric": "mixed_qp_launch_ms", "frames": n, "width": w, "height": h, "qps": [qa, qb], "ctus": ctus, "steps": args.steps, "cases": cases,
                      "median_ms": med, "mixed_ctus_per_s": ctus / (med["mixed"] * 1e-3),
                      "mixed_over_two_launches": med["mixed"] / best_two, "mixed_over_mean_of_uniform": med["mixed"] / uniform_mean,
                      "two_launches_spread": (max(cases["two_launches_overlapped"]["device_ms"]) - min(cases["two_launches_overlapped"]["device_ms"])) / med["two_launches_overlapped"],
                      "mixed_equals_half_launches": same}))
    for b in (whole, first, second):
        b.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
