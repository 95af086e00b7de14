#!/usr/bin/env python3
"""What a cost model per CTU costs (kvz_hip_intra_frames_ctu_models and the loop filters behind it), and that the launches that existed before cost what they cost.

1 536 resident 1080p pictures (bench.py's clip: kvazaar_amd.synth, seed 1, eight distinct frames cycled), `ultrafast`, QP 22, medians of five launches:
  (a) uniform / models             kvz_hip_intra_frames and kvz_hip_intra_frames_models (one model at 22), their loop filters (deblocking + SAO) and their coder -- on
                                   this build, and with --parent-lib <libkvz_hip.so of the parent commit> on that build too, in the same session.  The criterion: this
                                   build's median lies inside the parent's own min .. max of its launches.
  (b) ctu_models_uniform           the same pictures under a map that repeats 22 for every CTU, per stage, as ratios to `models`
  (c) ctu_models_map               a map of 22 +- 6 in 2x2-CTU blocks.  Slower by CONTENT: the CTUs at 16 carry more coefficients than the CTUs at 28 save
  (d) cu_qp_step_ms                the CU-QP step alone (kvz_hip_batch_last_cu_qp_ms)
The coder of a map codes one delta per CTU that has a coefficient beside what the coder of `models` codes.  The pass is device time from the batch's own events (kvz_hip_batch_last_kernel_ms); the loop filters and the coder are the host's wall clock over call + sync.
Every library is measured in a child process of its own.  Prints one JSON line.
Usage: python tools/bench_ctu_qp.py [--parent-lib PATH] [--frames 1536] [--steps 5] [--warmup 1] > profiles/ctu_qp_cost.json"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(args):
    import kvazaar_amd
    from kvazaar_amd import synth
    from kvazaar_amd.batch import HipBatch, PictureModels, cost_model
    lib = kvazaar_amd.load_library()
    w, h, n, qp = args.width, args.height, args.frames, args.qp
    clip = [np.concatenate([p.reshape(-1) for p in planes]) for planes in synth.frames(w, h, args.distinct, 1, "large")]
    b = HipBatch(lib, w, h, n)
    for i in range(n):
        b.upload(i, clip[i % len(clip)])
    wc, hc = (w + 63) // 64, (h + 63) // 64
    cases = {"uniform": cost_model(lib, qp), "models": PictureModels(lib, [qp] * n)}
    if hasattr(lib, "kvz_hip_intra_frames_ctu_models"):  # (the parent's library has none)
        from kvazaar_amd.batch import CtuModels
        blocks = [qp + (6 if (x // 2 + y // 2) % 2 else -6) for y in range(hc) for x in range(wc)]
        cases["ctu_models_uniform"] = CtuModels(lib, [qp] * n, [[qp] * (wc * hc)] * n)
        cases["ctu_models_map"] = CtuModels(lib, [qp] * n, [blocks] * n)
        lib.kvz_hip_batch_last_cu_qp_ms.restype = ctypes.c_float
        lib.kvz_hip_batch_last_cu_qp_ms.argtypes = [ctypes.c_void_p]
    out = {}
    for name, model in cases.items():
        stages = {"pass_ms": [], "loop_filters_ms": [], "coder_ms": [], "cu_qp_step_ms": []}
        for k in range(args.warmup + args.steps):
            if b.launch(model) < 0:
                raise RuntimeError("launch refused")
            b.sync()
            t0 = time.perf_counter()
            b.loop_filters(model, deblock=True, sao=True)
            t1 = time.perf_counter()
            b.entropy_code(model, sao=True)
            coder = (time.perf_counter() - t1) * 1e3
            if k >= args.warmup:
                stages["pass_ms"].append(round(float(b.kernel_ms()), 3))
                stages["loop_filters_ms"].append(round((t1 - t0) * 1e3, 3))
                stages["coder_ms"].append(round(coder, 3))
                if name.startswith("ctu_models"):
                    stages["cu_qp_step_ms"].append(round(float(lib.kvz_hip_batch_last_cu_qp_ms(b.handle)), 3))
        out[name] = {k: v for k, v in stages.items() if v}
        out[name]["checksum"] = int(b.checksums().astype(np.uint64).sum())
    b.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1536)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--qp", type=int, default=22)
    ap.add_argument("--parent-lib")
    ap.add_argument("--measure", action="store_true", help="(internal) measure the library of this process")
    args = ap.parse_args()
    if args.measure:
        measure(args)
        return 0

    def child(lib_path):
        env = dict(os.environ)
        if lib_path:
            env["KVZ_HIP_LIB"] = lib_path
        cmd = [sys.executable, os.path.abspath(__file__), "--measure"] + [f"--{k}={getattr(args, k)}" for k in ("frames", "width", "height", "distinct", "steps", "warmup", "qp")]
        return json.loads(subprocess.run(cmd, env=env, check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1])

    builds = {"this": child(None)}
    if args.parent_lib:
        builds["parent"] = child(args.parent_lib)
        builds["this_again"] = child(None)  # the session's drift, beside the comparison
    med = {b: {c: {s: float(np.median(v)) for s, v in stages.items() if s != "checksum"} for c, stages in cases.items()} for b, cases in builds.items()}
    result = {"metric": "ctu_qp_cost", "frames": args.frames, "width": args.width, "height": args.height, "qp": args.qp, "steps": args.steps, "builds": builds, "median_ms": med}
    this = med["this"]
    if "ctu_models_uniform" in this:
        result["b_uniform_map_over_models"] = {s: this["ctu_models_uniform"][s] / this["models"][s] for s in ("pass_ms", "loop_filters_ms", "coder_ms")}
        result["c_map_over_models"] = {s: this["ctu_models_map"][s] / this["models"][s] for s in ("pass_ms", "loop_filters_ms", "coder_ms")}
        result["c_note"] = "the map of 22 +- 6 is slower by content: its CTUs at 16 carry more coefficients than its CTUs at 28 save"
        result["d_cu_qp_step_ms"] = this["ctu_models_uniform"]["cu_qp_step_ms"]
        result["uniform_map_equals_uniform"] = builds["this"]["ctu_models_uniform"]["checksum"] == builds["this"]["uniform"]["checksum"]  # (picture hashes after the loop filters)
    if "parent" in builds:
        inside = {}
        for c in ("uniform", "models"):
            for s, v in builds["parent"][c].items():
                if s != "checksum":
                    inside[f"{c}.{s}"] = {"this_median": this[c][s], "parent_min": min(v), "parent_max": max(v), "inside": min(v) <= this[c][s] <= max(v)}
        result["a_this_median_inside_parent_range"] = inside
        result["same_pictures_as_parent"] = all(builds["this"][c]["checksum"] == builds["parent"][c]["checksum"] for c in ("uniform", "models"))
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
