#!/usr/bin/env python3
"""Generates tests/golden/signhide.json from the reference encoder (oracle/_ref/kvazaar_ref, compiled by `make -C oracle ref`) run with --signhide:

    python tests/golden/make_signhide_golden.py [--no-bench]

Per clip of tests/signhide_common.py CLIPS and per picture the fixture records what the encoder wrote while running:
  rec      sha256 prefix of the --debug reconstruction before the loop filters (--no-deblock, --sao off)
  cu       digest of the CU depth / intra mode maps behind it (oracle/ref_cudump.c), and `depths`, the CU depths that occur in the clip
  deblock  (one clip) the digest after deblocking
  entropy  sha256 prefix of the slice data -- the bytes are taken from the REFERENCE bitstream -- and the substream sizes
and, as digests only, the eight 1080p pictures tools/bench_signhide.py verifies its timed launch against (--no-bench keeps the ones the file has: two minutes of
the reference encoder).  Where the slice header ends follows from the substream sizes, which come from the host simulation's coder
(tests/hostsim/hostsim_signhide.cpp) and which the header's own entry points must confirm; the simulation's bytes must equal the reference's -- both asserted here,
as tests/golden/make_golden.py does with the oracle's coder.  Every picture must also DIFFER from its reconstruction without --signhide (the flat picture of the
adversarial set excepted): a fixture that the switch does not change would pin nothing."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ctypes as C  # noqa: E402

import entropy_common as ec  # noqa: E402
import flatapi  # noqa: E402
import make_golden as mg  # noqa: E402
import signhide_common as sc  # noqa: E402


def clip_entry(clip, sim, lib, workdir):
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    frames = sc.clip_frames(clip)
    maps = []
    recs = mg.reference_encoder_recon(w, h, frames, qp, 0, workdir, maps, bool(no_wpp), None, False, False, preset, extra=("--signhide",))
    plain = mg.reference_encoder_recon(w, h, frames, qp, 0, workdir, None, bool(no_wpp), None, False, False, preset)
    changed = [int((a != b).sum()) for a, b in zip(recs, plain)]
    assert all(c > 0 for i, c in enumerate(changed) if not (kind == "adversarial" and i == 0)), (name, changed)
    entry = {"rec": [sc.sha(r) for r in recs], "cu": [mg.cu_digest(d, m) for d, m in maps], "depths": sorted({int(v) for d, _ in maps for v in np.unique(d)}),
             "samples_changed_by_the_switch": changed}
    if name == sc.DEBLOCKED:
        entry["deblock"] = [sc.sha(r) for r in mg.reference_encoder_recon(w, h, frames, qp, 1, workdir, None, bool(no_wpp), None, False, False, preset, extra=("--signhide",))]
    options = ["--signhide"] + (["--no-wpp"] if no_wpp else []) + (["--sao", "off"] if preset != "ultrafast" else [])
    payloads = ec.reference_slice_payloads(os.path.join(flatapi.ROOT, "oracle", "_ref", "kvazaar_ref"), (name, w, h, n, seed, kind, qp, preset, options), workdir)
    pm = sc.table(lib, [qp] * n, **sc.switches(clip))
    outs = sc.sim_pass(sim, pm, w, h, frames)
    assert [sc.sha(o["rec"]) for o in outs] == entry["rec"], (name, "the host simulation does not reproduce the reference's reconstruction")
    pictures = []
    for payload, (data, sizes) in zip(payloads, sc.sim_entropy(sim, pm, w, h, outs)):
        total = sum(sizes)
        ref_data, header = payload[len(payload) - total:], payload[:len(payload) - total]
        assert ec.header_ends_with_entry_points(header, sizes, not no_wpp), (name, "the slice header's entry points are not these substream sizes")
        assert ref_data == data, (name, "the host simulation's coder does not reproduce the reference's slice data")
        pictures.append({"sha": sc.sha(np.frombuffer(ref_data, np.uint8)), "sizes": sizes})
    entry["entropy"] = pictures
    print(name, entry["depths"], changed, [sum(p["sizes"]) for p in pictures], flush=True)
    return entry


def bench_entry(workdir):
    name, w, h, n, seed, kind, qp, preset, no_wpp = sc.BENCH_CLIP
    recs = mg.reference_encoder_recon(w, h, sc.clip_frames(sc.BENCH_CLIP), qp, 0, workdir, None, False, None, False, False, preset, extra=("--signhide",))
    return {"rec": [sc.sha(r) for r in recs]}


def main():
    import kvazaar_amd
    lib = C.CDLL(kvazaar_amd.build_library())  # host-side functions only: the cost model of a QP
    sim = sc.load_sim()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for clip in sc.CLIPS:
            out[clip[0]] = clip_entry(clip, sim, lib, d)
        if "--no-bench" in sys.argv:
            out[sc.BENCH_CLIP[0]] = sc.fixture()[sc.BENCH_CLIP[0]]
        else:
            out[sc.BENCH_CLIP[0]] = bench_entry(d)
    json.dump(out, open(sc.FIXTURE, "w"), indent=0, sort_keys=True)
    print("wrote signhide.json:", len(out), "clips")


if __name__ == "__main__":
    main()
