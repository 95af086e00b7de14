#!/usr/bin/env python3
"""What B pictures at two QPs cost in ONE launch of the inter CTU pass (kvz_hip_dev_inter_ctu_pass_pictures) against what a caller could do before: one launch per QP.

`--sequences` resident 3840x2160 sequences (`--preset veryfast`, bench.py's clip: kvazaar_amd.synth; every sequence the same I picture and first B picture), timed cases:
  uniform_qp<a> / uniform_qp<b>  the whole launch at one QP (kvz_hip_dev_inter_ctu_pass)
  mixed                          even sequences at QP a, odd ones at QP b, one launch (kvz_hip_dev_inter_ctu_pass_pictures)
  two_launches_serial            the same halves as two half-size launches, one after the other on one thread
  two_launches_threads           ... side by side from two host threads, each on half of the workgroup slots (kvz_hip_dev_inter_set_share(2))
Device times are the HIP events the library records around a launch (kvz_hip_dev_inter_kernel_ms; serial: their sum, threads: the longer one), with the host's wall
clock over every case beside them -- for the two threads the wall clock is the figure that counts.
Prints one JSON line.  Usage: python tools/bench_inter_mixed_qp.py [--sequences 96] [--steps 3] [--warmup 1] [--qps 25 32]"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=96)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--qps", type=int, nargs=2, default=[25, 32], help="picture QPs of the two halves (25: --qp 22 at GOP layer 3, priced by the fast estimate; 32: by the residual coder)")
    args = ap.parse_args()
    import kvazaar_amd
    from kvazaar_amd import inter, synth
    from kvazaar_amd.batch import HipBatch, cost_model
    lib = kvazaar_amd.load_library()
    lib.kvz_hip_dev_inter_kernel_ms.restype = C.c_float
    w, h, n, half = args.width, args.height, args.sequences, args.sequences // 2
    assert n == 2 * half
    qa, qb = args.qps
    clip = [np.concatenate([p.reshape(-1) for p in planes]) for planes in synth.frames(w, h, 2, 1, "large")]
    # the reference of every sequence: the I picture through the batched intra pass and its loop filters
    mi = cost_model(lib, 21)
    bi = HipBatch(lib, w, h, 1)
    bi.upload(0, clip[0])
    bi.launch(mi)
    bi.loop_filters(mi, deblock=True, sao=True)
    rec0 = bi.download(0)["rec"]
    bi.close()
    cu0 = inter.intra_picture_cu_info(w, h)
    whole, first, second = inter.InterPictures(lib, w, h, n), inter.InterPictures(lib, w, h, half), inter.InterPictures(lib, w, h, half)
    for ip in (whole, first, second):
        for i in range(ip.n):
            ip.upload(i, clip[1], rec0, cu0)
    pa, pb = inter.veryfast_params(qa, 1), inter.veryfast_params(qb, 1)
    table = inter.InterPictureParams([qa if i % 2 == 0 else qb for i in range(n)], [1] * n)
    pool = ThreadPoolExecutor(max_workers=2)

    def kernel_ms():
        return float(lib.kvz_hip_dev_inter_kernel_ms())

    def one(ip, prm, pictures=None):
        def run():
            ip.run(prm, pictures=pictures)
            return kernel_ms()
        return run

    def serial():
        first.run(pa)
        ms = kernel_ms()
        second.run(pb)
        return ms + kernel_ms()

    def threads():
        def part(ip, prm):
            lib.kvz_hip_dev_inter_set_share(2)  # per calling thread: the pool's threads stay alive
            ip.run(prm)
            return kernel_ms()
        return max(f.result() for f in [pool.submit(part, first, pa), pool.submit(part, second, pb)])

    def timed(run):
        dev, wall = [], []
        for k in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            ms = run()
            t1 = time.perf_counter()
            if k >= args.warmup:
                dev.append(round(ms, 3))
                wall.append(round((t1 - t0) * 1e3, 3))
        return dev, wall

    cases = {}
    for name, run in ((f"uniform_qp{qa}", one(whole, pa)), (f"uniform_qp{qb}", one(whole, pb)), ("mixed", one(whole, pb, table)), ("two_launches_serial", serial),
                      ("two_launches_threads", threads), ("mixed_again", one(whole, pb, table))):
        dev, wall = timed(run)
        cases[name] = {"device_ms": dev, "wall_ms": wall}
    # the mixed launch computed what the half launches computed
    same = True
    for i in (0, 1, n - 2, n - 1):
        rec, cu = whole.download(i)
        rec2, cu2 = (first if i % 2 == 0 else second).download(i // 2)
        same = same and bool(np.array_equal(rec, rec2) and cu.tobytes() == cu2.tobytes())
    med = {k: float(np.median(v["device_ms"])) for k, v in cases.items()}
    wall = {k: float(np.median(v["wall_ms"])) for k, v in cases.items()}
    ctus = whole.ctus * n
    print(json.dumps({"metric": "inter_mixed_qp_launch_ms", "sequences": n, "width": w, "height": h, "qps": [qa, qb], "ctus": ctus, "steps": args.steps, "cases": cases,
                      "median_device_ms": med, "median_wall_ms": wall, "mixed_ctus_per_s": ctus / (med["mixed"] * 1e-3),
                      "mixed_over_serial_pair": med["mixed"] / med["two_launches_serial"], "mixed_wall_over_threads_wall": wall["mixed"] / wall["two_launches_threads"],
                      "mixed_over_mean_of_uniform": med["mixed"] / (0.5 * (med[f"uniform_qp{qa}"] + med[f"uniform_qp{qb}"])), "mixed_equals_half_launches": same}))
    for ip in (whole, first, second):
        ip.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
