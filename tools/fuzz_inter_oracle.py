#!/usr/bin/env python3
"""Fuzz of the sequence oracle (oracle/kvz_oracle_inter.inc) against the REFERENCE ENCODER itself (oracle/_ref/kvazaar_ref with the ref_cudump.c interposer; only where
the reference was compiled, i.e. not on the GPU box).  The rounds are drawn by tests/inter_common.py draw_fuzz_case, the distribution the device meets in
tests/test_gpu_inter_fuzz.py: picture sizes from 8x8 to 264x264 in steps of 8 (a third of them below one CTU in a dimension), --qp 0..51, the presets ultrafast /
superfast / veryfast / faster, --subme and --fast-residual-cost overrides, low-delay GOPs of 2, 3, 4 and 8 pictures, loop filters on / off, the overlapped-picture
motion restriction (--owf 2) on / off, --no-wpp, and six kinds of content: the textured clip with moving objects, per-sample 0 / 255, 0 / 255 in 4x4 blocks, uniform
noise, flat pictures and a full-range smooth texture, each under a whole- or sub-sample pan.  The oracle's final pictures must be the encoder's --debug output
every CU decision (type, depth, skip / merge, merge index, vectors, MVP indices, intra mode) the encoder's, and the slice data of every picture (the oracle's
entropy coder) the bytes behind the encoder's slice headers.  usage: tools/fuzz_inter_oracle.py [rounds] [seed]"""
import os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import flatapi, inter_common as ic, entropy_common as ec

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 12
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
oracle = flatapi.load_oracle()
bad = 0
for r in range(rounds):
    c = ic.draw_fuzz_case(rng, max_frames=5)
    w, h, qp, no_wpp, ov = c["w"], c["h"], c["qp"], c["no_wpp"], c["overrides"]
    extra = []  # options that differ from the preset's: --subme (0..4), --fast-residual-cost
    if "fme_level" in ov:
        extra += ["--subme", str(ov["fme_level"])]
    if "fast_residual_cost" in ov:
        extra += ["--fast-residual-cost", str(ov["fast_residual_cost"])]
    frames = ic.fuzz_frames(c)
    kw = ic.fuzz_oracle_kwargs(c)
    rs, rf, cu, qps = ic.oracle_encode(oracle, w, h, frames, qp, **kw)
    with tempfile.TemporaryDirectory() as d:
        rrec, rcu = ic.reference_encode(w, h, frames, qp, d, preset=c["preset"], deblock=bool(c["deblock"]), sao=bool(c["sao"]), owf=c["ref_owf"], gop="lp-g%dd%dt1" % c["gop"], extra=extra + (["--no-wpp"] if no_wpp else []))
        payloads = ec.slice_payloads(open(os.path.join(d, "out.hevc"), "rb").read())
    diff = ic.first_difference(cu, rcu)
    ok = diff is None and np.array_equal(rf, rrec)
    # ... and the slice data the oracle's entropy coder writes for every picture (kvz_oracle_entropy.inc) must be the tail of the encoder's slice NAL payloads
    bits = ic.oracle_encode_bits(oracle, w, h, frames, qp, **kw)
    for payload, (data, sizes) in zip(payloads, bits):
        ok = ok and payload[len(payload) - sum(sizes):] == data and ec.header_ends_with_entry_points(payload[:len(payload) - sum(sizes)], sizes, not no_wpp)
    b = cu[1:]
    print("round %d: %s ref owf %d (pictures %s): intra %d inter %d -> %s" % (r, ic.describe_fuzz_case(c), c["ref_owf"], list(map(int, qps)), int((b["type"] == 1).sum()), int((b["type"] == 2).sum()),
                                                                              "equal" if ok else "DIFFERENT %s" % (diff,)), flush=True)
    bad += not ok
print("%d of %d rounds differ" % (bad, rounds))
sys.exit(1 if bad else 0)
