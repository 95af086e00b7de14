#!/usr/bin/env python3
"""Generates tests/golden/inter_me.json from the reference encoder (oracle/_ref/kvazaar_ref, compiled by `make -C oracle _ref/kvazaar_ref`) run on low-delay
sequences (--gop lp-g4d3t1) with --me / --me-steps / --me-early-termination:

    python tests/golden/make_inter_me_golden.py

Per case (a clip of tests/inter_me_common.py CLIPS under one of its options) and per picture the fixture records what the encoder wrote while running:
  rec     sha256 prefix of the --debug reconstruction (the final picture, after the loop filters)
  slices  per B picture the sha256 prefix of the slice data -- the bytes are taken from the REFERENCE bitstream -- and the substream sizes; the slice data pins every
          CU decision, vector and level
No library is preloaded into any process: the reference runs as it is built.
Asserted here: the host-simulated chain (tests/inter_me_common.py sim_chain) reproduces all of it with no 24-bit multiply out of range; every option differs from
the hexbs encode on at least one clip; `on` differs from `sensitive`, `off` from both; and the simulation's counters show that the searches met every branch
REQUIRED names.  Also recorded, without a threshold: bitstream bytes and luma PSNR of every case."""
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
import inter_me_common as mec  # noqa: E402
import scaling_lists_common as slc  # noqa: E402

# counters of the simulation that must be non-zero over the set (tests/inter_me_common.py me_events)
REQUIRED = ("tz_from_zero", "star_two_rounds", "tz_distance_16", "full_extra_run", "full_extra_skipped", "merge_window_covered", "mv_refused", "leaves_left", "leaves_right",
            "leaves_top", "leaves_bottom", "dia_step_limit", "hex_step_limit")


def reference(clip, workdir, extra):
    name, w, h, n, qp, preset, dbk, sao, owf, _ = clip
    rec, _ = ic.reference_encode(w, h, ic.case_frames(clip), qp, workdir, preset=preset, deblock=bool(dbk), sao=bool(sao), owf=owf, cu=False, extra=extra)
    stream = open(os.path.join(workdir, "out.hevc"), "rb").read()
    return rec, ec.slice_payloads(stream), len(stream)


def psnr_y(frames, rec, w, h):
    mse = np.mean([np.mean((f[:w * h].astype(np.float64) - r[:w * h].astype(np.float64)) ** 2) for f, r in zip(frames, rec)])
    return round(float(10 * np.log10(255.0 ** 2 / mse)), 3)


def case_entry(clip, option, sim, intra_sim, oracle, lib, workdir, events):
    name, w, h, n, qp, preset, dbk, sao, owf, _ = clip
    rec, payloads, stream_bytes = reference(clip, workdir, mec.OPTIONS[option][0])
    entry = {"rec": [ilc.sha(r) for r in rec], "bytes": stream_bytes, "psnr_y": psnr_y(ic.case_frames(clip), rec, w, h)}
    ilc.mul24_violations(sim, reset=True)
    mec.me_events(sim, reset=True)
    chain = mec.sim_chain(sim, intra_sim, oracle, lib, clip, option)
    assert ilc.mul24_violations(sim) == 0, (name, option, "a 24-bit multiply with an operand out of range")
    for k, v in mec.me_events(sim, reset=True).items():
        events[k] = events.get(k, 0) + v
    slices = [None]
    for k in range(n):
        assert ilc.sha(chain["final"][k]) == entry["rec"][k], (name, option, k, "the simulated chain does not reproduce the reference's picture")
        if k > 0:
            data, sizes = chain["slices"][k]
            total = sum(sizes)
            ref_data, header = payloads[k][len(payloads[k]) - total:], payloads[k][:len(payloads[k]) - total]
            assert ec.header_ends_with_entry_points(header, sizes, True), (name, option, k, "the slice header's entry points are not these substream sizes")
            assert ref_data == data, (name, option, k, "the B-slice coder simulation does not reproduce the reference's slice data")
            slices.append({"sha": ilc.sha(np.frombuffer(ref_data, np.uint8)), "sizes": sizes})
    entry["slices"], entry["qps"] = slices, chain["qps"]
    print(name, option, chain["qps"], entry["bytes"], entry["psnr_y"], flush=True)
    return entry


def main():
    import kvazaar_amd
    lib = C.CDLL(kvazaar_amd.build_library())  # host-side functions only: the cost model of a QP
    sim, intra_sim, oracle = mec.load_sim(), slc.load_sim(), flatapi.load_oracle()
    out, events = {}, {}
    with tempfile.TemporaryDirectory() as d:
        for clip, options in mec.CLIPS:
            for option in options:
                out[mec.key(clip[0], option)] = case_entry(clip, option, sim, intra_sim, oracle, lib, d, events)
    # 1. every option changes something somewhere; the termination settings differ from each other
    for option in mec.ALL:
        if option != "hexbs":
            assert any(out[mec.key(c[0], option)]["rec"] != out[mec.key(c[0], "hexbs")]["rec"] for c, opts in mec.CLIPS if option in opts), (option, "never differs from hexbs")
    pan11 = {o: out[mec.key("pan11", o)]["rec"] for o in mec.ALL}
    assert pan11["et-on"] != pan11["hexbs"] and pan11["et-off"] != pan11["hexbs"] and pan11["et-off"] != pan11["et-on"]
    assert len({tuple(v) for v in pan11.values()}) == len(pan11), "two options of pan11 encode alike"
    # 2. the branches the searches met
    missing = [k for k in REQUIRED if not events.get(k)]
    assert not missing, ("no clip reaches", missing, events)
    out["events"] = events
    out["compression"] = {k: {"bytes": v["bytes"], "psnr_y": v["psnr_y"]} for k, v in out.items() if "bytes" in v}
    json.dump(out, open(mec.FIXTURE, "w"), indent=0, sort_keys=True)
    print("wrote inter_me.json:", len(out), "entries; events", events)


if __name__ == "__main__":
    main()
