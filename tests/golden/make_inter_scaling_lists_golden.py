#!/usr/bin/env python3
"""Generates tests/golden/inter_scaling_lists.json from the reference encoder (oracle/_ref/kvazaar_ref, compiled by `make -C oracle ref`) run on low-delay
sequences (--gop lp-g4d3t1) with --scaling-list default:

    python tests/golden/make_inter_scaling_lists_golden.py [--no-bench] [clip names]

Per clip of tests/inter_lists_common.py CLIPS and per picture the fixture records what the encoder wrote while running:
  rec      sha256 prefix of the --debug reconstruction (the final picture, after the loop filters)
  cu       digest of the CU decisions behind it (oracle/ref_cudump.c records, kvazaar_amd.inter.cu_digest)
  entropy  (one clip) per B picture the sha256 prefix of the slice data -- the bytes are taken from the REFERENCE bitstream -- and the substream sizes
and, as digests only, the 3840x2160 B picture tools/bench_inter_scaling_lists.py verifies its timed launches against (--no-bench keeps the ones the file has).
Asserted here: every B picture DIFFERS from its encode without the lists; the host-simulated chain (tests/inter_lists_common.py sim_chain: the LISTS simulation of the
all-intra pass, the oracle's loop filters, tests/hostsim/hostsim_inter_lists.cpp, the B-slice coder simulation) reproduces all of it; and the coverage table --
non-zero levels at positions whose list entry is not 16, per CU kind, plane, transform size and side of the dequantiser's branch, counted from the simulation's
levels -- has no empty cell over the clips."""
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import entropy_common as ec  # noqa: E402
import flatapi  # noqa: E402
import inter_common as ic  # noqa: E402
import inter_lists_common as ilc  # noqa: E402
import scaling_lists_common as slc  # noqa: E402

LISTS = ("--scaling-list", "default")


def reference(clip, workdir, extra):
    name, w, h, n, qp, preset, dbk, sao, owf, _ = clip
    rec, cu = ic.reference_encode(w, h, ic.case_frames(clip), qp, workdir, preset=preset, deblock=bool(dbk), sao=bool(sao), owf=owf, extra=extra)
    return rec, cu, ec.slice_payloads(open(os.path.join(workdir, "out.hevc"), "rb").read())


def clip_entry(clip, sim, intra_sim, oracle, lib, workdir):
    from kvazaar_amd import inter
    name, w, h, n, qp, preset, dbk, sao, owf, _ = clip
    rec, cu, payloads = reference(clip, workdir, LISTS)
    plain = reference(clip, workdir, ())[0]
    changed = [int((a != b).sum()) for a, b in zip(rec, plain)]
    assert all(c > 0 for c in changed[1:]), (name, "a B picture the lists leave untouched", changed)
    entry = {"rec": [ilc.sha(r) for r in rec], "cu": [inter.cu_digest(c) for c in cu], "samples_changed_by_the_lists": changed}
    ilc.mul24_violations(sim, reset=True)
    chain = ilc.sim_chain(sim, intra_sim, oracle, lib, clip, "default", slice_data=name == ilc.PINNED)
    assert ilc.mul24_violations(sim) == 0, (name, "a 24-bit multiply with an operand out of range")
    for k in range(n):
        assert ilc.sha(chain["final"][k]) == entry["rec"][k], (name, k, "the simulated chain does not reproduce the reference's picture")
        if k > 0:
            assert ic.first_difference(chain["cu"][k][None], cu[k][None]) is None and inter.cu_digest(chain["cu"][k]) == entry["cu"][k], (name, k, "CU decisions")
    entry["coverage"] = ilc.coverage(chain["cu"][1:], chain["coeff"][1:], w, h, chain["qps"][1:])
    entry["qps"] = chain["qps"]
    if name == ilc.PINNED:
        pictures = [None]
        for k in range(1, n):
            data, sizes = chain["slices"][k]
            total = sum(sizes)
            ref_data, header = payloads[k][len(payloads[k]) - total:], payloads[k][:len(payloads[k]) - total]
            assert ec.header_ends_with_entry_points(header, sizes, True), (name, k, "the slice header's entry points are not these substream sizes")
            assert ref_data == data, (name, k, "the B-slice coder simulation does not reproduce the reference's slice data")
            pictures.append({"sha": ilc.sha(np.frombuffer(ref_data, np.uint8)), "sizes": sizes})
        entry["entropy"] = pictures
    print(name, chain["qps"], changed, entry["coverage"], flush=True)
    return entry


def bench_entry(workdir):
    """picture 1 of BASELINE config 4's sequence, before and after its loop filters are not separable in the reference: the final picture and the CU decisions"""
    from kvazaar_amd import inter
    case = [c for c in ic.CASES if c[0] == ilc.BENCH_CLIP][0]
    name, w, h, n, qp, preset, dbk, sao, owf, _ = case
    frames = ic.case_frames(case)[:2]
    rec, cu = ic.reference_encode(w, h, frames, qp, workdir, preset=preset, deblock=bool(dbk), sao=bool(sao), owf=owf, extra=LISTS)
    return {"rec": [ilc.sha(r) for r in rec], "cu": [inter.cu_digest(c) for c in cu]}


def main():
    import kvazaar_amd
    lib = C.CDLL(kvazaar_amd.build_library())  # host-side functions only: the cost model of a QP
    sim, intra_sim, oracle = ilc.load_sim(), slc.load_sim(), flatapi.load_oracle()
    names = [a for a in sys.argv[1:] if not a.startswith("--")]
    old = ilc.fixture() if os.path.exists(ilc.FIXTURE) else {}
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for clip in ilc.CLIPS:
            out[clip[0]] = clip_entry(clip, sim, intra_sim, oracle, lib, d) if not names or clip[0] in names else old[clip[0]]
        total = {cell: sum(out[c[0]]["coverage"].get(cell, 0) for c in ilc.CLIPS) for cell in ilc.CELLS}
        assert all(v > 0 for v in total.values()), total
        out["coverage"] = total
        if "--no-bench" in sys.argv:
            if ilc.BENCH_CLIP in old:
                out[ilc.BENCH_CLIP] = old[ilc.BENCH_CLIP]
        else:
            out[ilc.BENCH_CLIP] = bench_entry(d)
    json.dump(out, open(ilc.FIXTURE, "w"), indent=0, sort_keys=True)
    print("wrote inter_scaling_lists.json:", len(out), "entries; coverage", total)


if __name__ == "__main__":
    main()
