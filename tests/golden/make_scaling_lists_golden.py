#!/usr/bin/env python3
"""Generates tests/golden/scaling_lists.json from the reference encoder (oracle/_ref/kvazaar_ref, compiled by `make -C oracle ref`) run with --scaling-list default:

    python tests/golden/make_scaling_lists_golden.py [--no-bench]

Per clip of tests/scaling_lists_common.py CLIPS and per picture the fixture records what the encoder wrote while running:
  rec      sha256 prefix of the --debug reconstruction before the loop filters (--no-deblock, --sao off)
  cu       digest of the CU depth / intra mode maps behind it (oracle/ref_cudump.c), and `depths`, the CU depths that occur in the clip
  deblock  (one clip) the digest after deblocking
  entropy  (the same clip) sha256 prefix of the slice data -- the bytes are taken from the REFERENCE bitstream -- and the substream sizes
and, as digests only, the eight 1080p pictures tools/bench_scaling_lists.py verifies its timed launches against (--no-bench keeps the ones the file has).
Asserted here: the host simulation (tests/hostsim/hostsim_scaling_lists.cpp) reproduces all of it; every picture DIFFERS from its encode without the lists, except
the pictures scaling_lists_common.UNTOUCHED_OK names (no levels where the default list is not 16); and the coverage table -- non-zero levels at positions whose list
entry is not 16, per plane, transform size and side of the dequantiser's branch, counted from the simulation's levels -- has no empty cell over the clips."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ctypes as C  # noqa: E402

import deblock_common as dc  # noqa: E402
import entropy_common as ec  # noqa: E402
import flatapi  # noqa: E402
import make_golden as mg  # noqa: E402
import scaling_lists_common as slc  # noqa: E402
import signhide_common as sc  # noqa: E402

LISTS = ("--scaling-list", "default")


def clip_entry(clip, sim, coder_sim, oracle, lib, workdir):
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    frames = slc.clip_frames(clip)
    maps = []
    recs = mg.reference_encoder_recon(w, h, frames, qp, 0, workdir, maps, bool(no_wpp), None, False, False, preset, extra=LISTS)
    plain = mg.reference_encoder_recon(w, h, frames, qp, 0, workdir, None, bool(no_wpp), None, False, False, preset)
    changed = [int((a != b).sum()) for a, b in zip(recs, plain)]
    assert all(c > 0 for i, c in enumerate(changed) if i not in slc.UNTOUCHED_OK.get(name, ())), (name, changed)
    entry = {"rec": [slc.sha(r) for r in recs], "cu": [mg.cu_digest(d, m) for d, m in maps], "depths": sorted({int(v) for d, _ in maps for v in np.unique(d)}),
             "samples_changed_by_the_lists": changed}
    pm = slc.table(lib, [qp] * n, **slc.switches(clip))
    outs = slc.sim_pass(sim, pm, [slc.lists("default")], None, w, h, frames)
    assert [slc.sha(o["rec"]) for o in outs] == entry["rec"], (name, "the host simulation does not reproduce the reference's reconstruction")
    assert [mg.cu_digest(o["depth"].reshape(h // 8, w // 8), o["mode"].reshape(h // 8, w // 8)) for o in outs] == entry["cu"], (name, "CU maps")
    entry["coverage"] = slc.coverage(outs, w, h, qp)
    if name == slc.PINNED:
        entry["deblock"] = [slc.sha(r) for r in mg.reference_encoder_recon(w, h, frames, qp, 1, workdir, None, bool(no_wpp), None, False, False, preset, extra=LISTS)]
        deb = [dc.run_cpu(oracle.lib.kvz_oracle_deblock_frame, w, h, qp, 0, 0, o["rec"], o["depth"].reshape(h // 8, w // 8)) for o in outs]
        assert [slc.sha(d) for d in deb] == entry["deblock"], (name, "deblocking of the simulation's pictures")
        options = list(LISTS) + (["--no-wpp"] if no_wpp else []) + (["--sao", "off"] if preset != "ultrafast" else [])
        payloads = ec.reference_slice_payloads(os.path.join(flatapi.ROOT, "oracle", "_ref", "kvazaar_ref"), (name, w, h, n, seed, kind, qp, preset, options), workdir)
        pictures = []
        for payload, (data, sizes) in zip(payloads, sc.sim_entropy(coder_sim, pm, w, h, outs)):
            total = sum(sizes)
            ref_data, header = payload[len(payload) - total:], payload[:len(payload) - total]
            assert ec.header_ends_with_entry_points(header, sizes, not no_wpp), (name, "the slice header's entry points are not these substream sizes")
            assert ref_data == data, (name, "the host simulation's coder does not reproduce the reference's slice data")
            pictures.append({"sha": slc.sha(np.frombuffer(ref_data, np.uint8)), "sizes": sizes})
        entry["entropy"] = pictures
    print(name, entry["depths"], changed, entry["coverage"], flush=True)
    return entry


def bench_entry(workdir):
    name, w, h, n, seed, kind, qp, preset, no_wpp = slc.BENCH_CLIP
    recs = mg.reference_encoder_recon(w, h, slc.clip_frames(slc.BENCH_CLIP), qp, 0, workdir, None, False, None, False, False, preset, extra=LISTS)
    return {"rec": [slc.sha(r) for r in recs]}


def main():
    import kvazaar_amd
    lib = C.CDLL(kvazaar_amd.build_library())  # host-side functions only: the cost model of a QP
    sim, coder_sim, oracle = slc.load_sim(), sc.load_sim(), flatapi.load_oracle()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for clip in slc.CLIPS:
            out[clip[0]] = clip_entry(clip, sim, coder_sim, oracle, lib, d)
        total = {cell: sum(out[c[0]]["coverage"].get(cell, 0) for c in slc.CLIPS) for cell in slc.CELLS}
        assert all(v > 0 for v in total.values()), total
        out["coverage"] = total
        if "--no-bench" in sys.argv:
            old = slc.fixture() if os.path.exists(slc.FIXTURE) else {}
            if slc.BENCH_CLIP[0] in old:
                out[slc.BENCH_CLIP[0]] = old[slc.BENCH_CLIP[0]]
        else:
            out[slc.BENCH_CLIP[0]] = bench_entry(d)
    json.dump(out, open(slc.FIXTURE, "w"), indent=0, sort_keys=True)
    print("wrote scaling_lists.json:", len(out), "entries; coverage", total)


if __name__ == "__main__":
    main()
