"""bench.py's two-batch chain_full pattern (pictures uploaded inside the timed region) with and without kvz_hip_batch_sse_async behind every deblocking.
One JSON line on stdout.  KVZ_HIP_LIB selects the library (the parent commit's build has no SSE: --variants plain)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def chain(pair, model, qp, reps, src_ptr, sse_ptrs):
    for b in pair:
        b.sync()
    for b in pair:
        b.entropy_defer_download(True)
    t = time.perf_counter()
    turns = reps * len(pair)
    cur = pair[0]
    cur.launch(model)
    cur.deblock(qp, wait=False)
    if sse_ptrs:
        cur.sse_async(sse_ptrs[id(cur)])
    for i in range(turns):
        nxt = pair[(i + 1) % len(pair)]
        more = i + 1 < turns
        if i + len(pair) < turns:
            cur.upload_all_async(src_ptr)
        cur.entropy_code(model, then=(nxt, model) if more else None)
        if more:
            nxt.deblock(qp, wait=False)
            if sse_ptrs:
                nxt.sse_async(sse_ptrs[id(nxt)])
        cur = nxt
    for b in pair:
        b.sync()
    s = time.perf_counter() - t
    for b in pair:
        b.entropy_defer_download(False)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="plain,sse")
    ap.add_argument("--tag", default="")
    ap.add_argument("--frames", type=int, default=1536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--attempts", type=int, default=3)
    args = ap.parse_args()
    import bench
    import kvazaar_amd
    from kvazaar_amd.batch import HipBatch, cost_model, pinned_bytes
    lib = kvazaar_amd.load_library()
    w, h, qp, n = 1920, 1080, 22, args.frames
    model = cost_model(lib, qp)
    distinct = bench.synth_frames(w, h, 8, bench.clip_seed(w, h))
    fb = w * h * 3 // 2
    pair = []
    for _ in range(2):
        b = HipBatch(lib, w, h, n)
        for i in range(n):
            b.upload(i, distinct[i % len(distinct)])
        pair.append(b)
    src_ptr, src_view = pinned_bytes(lib, n * fb)
    for i in range(n):
        src_view[i * fb:(i + 1) * fb] = distinct[i % len(distinct)]
    variants = args.variants.split(",")
    sse_ptrs, sse_views = {}, {}
    if "sse" in variants:
        for b in pair:
            sse_ptrs[id(b)], sse_views[id(b)] = pinned_bytes(lib, n * 24)
    for b in pair:  # first use: the coder's scratch allocations
        b.launch(model)
        b.deblock(qp, wait=False)
        b.entropy_code(model)
    chain(pair, model, qp, 1, src_ptr, None)  # warm-up of the pattern (pinned pages)
    out = {"tag": args.tag, "lib": os.environ.get("KVZ_HIP_LIB", "default"), "frames_per_batch": n, "batches_timed": 2 * args.reps, "ms_per_batch": {v: [] for v in variants}}
    for _ in range(args.attempts):
        for v in variants:  # alternating
            try:
                s = chain(pair, model, qp, args.reps, src_ptr, sse_ptrs if v == "sse" else None)
                out["ms_per_batch"][v].append(round(s / (2 * args.reps) * 1e3, 2))
            except Exception as e:
                out["ms_per_batch"][v].append(repr(e))
                for b in pair:
                    b.reset()
    if "sse" in variants:
        got = [np.frombuffer(sse_views[id(b)], np.uint64).reshape(n, 3) for b in pair]
        out["sse_copies_consistent"] = bool(all(np.array_equal(g[i], g[i % len(distinct)]) for g in got for i in range(n)) and np.array_equal(got[0], got[1]))
        out["sse_picture0"] = [int(v) for v in got[0][0]]
        try:
            gold = json.load(open(os.path.join(ROOT, "tests", "golden", "psnr.json")))["ultrafast-1920x1080-qp22"]["0"]["sse"]
            out["sse_picture0_equals_fixture"] = out["sse_picture0"] == gold
        except Exception as e:
            out["sse_picture0_equals_fixture"] = repr(e)
    print(json.dumps(out), flush=True)
    for b in pair:
        b.close()


if __name__ == "__main__":
    main()
