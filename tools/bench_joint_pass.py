#!/usr/bin/env python3
"""What joining the CTU passes of batches of different picture sizes into ONE launch (kvz_hip_batch_group) buys, and what the per-ticket record fetch costs.

Mixes of 1920x1080, 832x480 and 3840x2160 pictures (kvazaar_amd.synth `large` clips, seeds 1, 5, 2: the pictures tests/golden/encoder_recon.json holds digests of at
`ultrafast` QP 22; the distinct frames cycled over each batch), each in three legs:
  solo          the three batches' own passes one after the other (kvz_hip_intra_frames_models; the sum of the three device times)
  side_by_side  the three passes launched back to back on their own streams, each on its share of the workgroup slots in proportion to its CTU count
                (kvz_hip_batch_set_device_share); host wall-clock from the first launch to the last sync, and the longest of the three device times
  joint         one launch of the group (kvz_hip_batch_group_last_kernel_ms)
  --mix full    512 x 1080p + 1 024 x 832x480 + 96 x 2160p        --mix thin    48 + 96 + 12: alone, each exposes a fraction of the device's slots' worth of diagonals
--record-fetch: a group of two 768-picture 1080p batches against ONE 1 536-picture batch (kvz_hip_intra_frames), launches alternating; the ratio of the medians
beside the single batch's own run-to-run range.
Device times are from the HIP events the library records around its launches, warm-up launches first, medians of --steps timed launches.  Every timed leg is verified:
the first pictures of every batch against the fixture's digests.  Prints one JSON line; exit status 1 when a verification fails.
Usage: python tools/bench_joint_pass.py [--mix full|thin] [--record-fetch] [--steps 3] [--warmup 1]"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(1920, 1080, 8, 1, "1920x1080/n8/seed1/large/qp22/nodeblock"), (832, 480, 1, 5, "832x480/n1/seed5/large/qp22/nodeblock"),
         (3840, 2160, 4, 2, "3840x2160/n4/seed2/large/qp22/nodeblock")]
MIXES = {"full": (512, 1024, 96), "thin": (48, 96, 12)}
QP = 22


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def make_batch(lib, w, h, n, distinct, seed):
    from kvazaar_amd import synth
    from kvazaar_amd.batch import HipBatch
    clip = [np.concatenate([p.reshape(-1) for p in planes]) for planes in synth.frames(w, h, distinct, seed, "large")]
    b = HipBatch(lib, w, h, n)
    for i in range(n):
        b.upload(i, clip[i % distinct])
    return b


def verified(batch, distinct, key, recon):
    k = min(batch.n, distinct)
    return [sha(batch.download(i)["rec"]) for i in range(k)] == recon[key][:k]


def shares(ctus, slots=8):
    """slots per CU in proportion to the CTU counts, at least one each, largest remainders first"""
    exact = [slots * c / sum(ctus) for c in ctus]
    got = [max(1, int(e)) for e in exact]
    for i in sorted(range(len(ctus)), key=lambda i: exact[i] - int(exact[i]), reverse=True):
        if sum(got) < slots:
            got[i] += 1
    return got


def run_mix(lib, name, args, recon):
    from kvazaar_amd.batch import BatchGroup, PictureModels
    batches = [make_batch(lib, w, h, n, d, seed) for (w, h, d, seed, _), n in zip(SIZES, MIXES[name])]
    tables = [PictureModels(lib, [QP] * b.n) for b in batches]
    ctus = [b.ctus_per_frame * b.n for b in batches]
    group = BatchGroup(lib, batches)
    legs, ok = {"solo": [], "side_by_side": [], "side_by_side_wall": [], "joint": [], "joint_wall": []}, True

    def check():
        return all(verified(b, s[2], s[4], recon) for b, s in zip(batches, SIZES))
    for k in range(args.warmup + args.steps):
        ms = 0.0
        for b, t in zip(batches, tables):
            b.run(t)
            ms += float(b.kernel_ms())
        if k >= args.warmup:
            legs["solo"].append(round(ms, 3))
    ok = ok and check()
    part = shares(ctus)
    for b, p in zip(batches, part):
        b.set_device_share(p, 8)
    for k in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        for b, t in zip(batches, tables):
            if b.launch(t) < 0:
                raise RuntimeError("launch refused")
        for b in batches:
            b.sync()
        wall = (time.perf_counter() - t0) * 1e3
        if k >= args.warmup:
            legs["side_by_side"].append(round(max(float(b.kernel_ms()) for b in batches), 3))
            legs["side_by_side_wall"].append(round(wall, 3))
    ok = ok and check()
    for b in batches:
        b.set_device_share(1, 1)
    for k in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        group.run(tables)
        wall = (time.perf_counter() - t0) * 1e3
        if k >= args.warmup:
            legs["joint"].append(round(group.kernel_ms(), 3))
            legs["joint_wall"].append(round(wall, 3))
    ok = ok and check()
    group.close()
    for b in batches:
        b.close()
    med = {k: float(np.median(v)) for k, v in legs.items()}
    total = sum(ctus)
    return {"pictures": list(MIXES[name]), "ctus": ctus, "slot_shares_of_8": part, "legs_ms": legs, "median_ms": med,
            "ctus_per_s": {k: total / (med[k] * 1e-3) for k in ("solo", "side_by_side", "side_by_side_wall", "joint")},
            "joint_over_solo": med["joint"] / med["solo"], "joint_over_side_by_side": med["joint"] / med["side_by_side"],
            "joint_over_side_by_side_wall": med["joint"] / med["side_by_side_wall"], "verified": ok}


def run_record_fetch(lib, args, recon):
    from kvazaar_amd.batch import BatchGroup, PictureModels, cost_model
    w, h, d, seed, key = SIZES[0]
    single = make_batch(lib, w, h, 1536, d, seed)
    halves = [make_batch(lib, w, h, 768, d, seed) for _ in range(2)]
    group = BatchGroup(lib, halves)
    model, tables = cost_model(lib, QP), [PictureModels(lib, [QP] * 768) for _ in range(2)]
    one, two = [], []
    for k in range(args.warmup + args.steps):  # alternating
        single.run(model)
        group.run(tables)
        if k >= args.warmup:
            one.append(round(float(single.kernel_ms()), 3))
            two.append(round(group.kernel_ms(), 3))
    ok = verified(single, d, key, recon) and all(verified(b, d, key, recon) for b in halves)
    group.close()
    for b in halves + [single]:
        b.close()
    return {"single_1536_ms": one, "group_2x768_ms": two, "single_range_ms": [min(one), max(one)], "group_over_single": float(np.median(two)) / float(np.median(one)), "verified": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mix", action="append", choices=list(MIXES), default=[])
    ap.add_argument("--record-fetch", action="store_true")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import kvazaar_amd
    lib = kvazaar_amd.load_library()
    recon = json.load(open(os.path.join(ROOT, "tests", "golden", "encoder_recon.json")))
    out = {"metric": "joint_pass", "qp": QP, "steps": args.steps, "warmup": args.warmup, "mixes": {}}
    for name in args.mix or ([] if args.record_fetch else ["thin"]):
        out["mixes"][name] = run_mix(lib, name, args, recon)
    if args.record_fetch:
        out["record_fetch"] = run_record_fetch(lib, args, recon)
    ok = all(m["verified"] for m in out["mixes"].values()) and out.get("record_fetch", {}).get("verified", True)
    out["verified"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
