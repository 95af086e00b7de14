#!/usr/bin/env python3
"""Generates tests/golden/inter_p.json from the reference encoder (oracle/_ref/kvazaar_ref, compiled by `make -C oracle _ref/kvazaar_ref`) run with --no-bipred on
the clips of tests/inter_p_common.py CLIPS (--gop lp-g4d3t1, one with --gop 0): the IPPP stream, whose inter pictures are P slices.

    python tests/golden/make_inter_p_golden.py

Per case and per picture the fixture records what the encoder wrote while running:
  rec     sha256 prefix of the --debug reconstruction (the final picture, after the loop filters)
  slices  per P picture the sha256 prefix of the slice data -- the bytes are taken from the REFERENCE bitstream -- and the substream sizes; the slice data pins every
          CU decision, vector and level
  qps     the picture QPs
No library is preloaded into any process: the reference runs as it is built.
Asserted here, on the reference alone: every inter slice header of a case says slice_type P (the first payload byte of its NAL unit begins 1 1 010:
first_slice_segment_in_pic_flag, slice_pic_parameter_set_id 0, slice_type 1), and the pictures differ from the B encode of the same clip (the same command
without --no-bipred).  Asserted with the simulated chain (tests/inter_p_common.py sim_chain): it reproduces every picture and every slice byte with no 24-bit
multiply out of range, no CU record of a P picture carries an mv_dir other than 1, and every event of the census occurs at least 16 times over the set.
Also recorded, without a threshold: bitstream bytes and luma PSNR of every case beside the B encode's."""
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
import inter_p_common as pc  # noqa: E402
import scaling_lists_common as slc  # noqa: E402


def reference(clip, gop, workdir, extra):
    name, w, h, n, qp, preset, dbk, sao, owf, _ = clip
    rec, _ = ic.reference_encode(w, h, ic.case_frames(clip), qp, workdir, preset=preset, deblock=bool(dbk), sao=bool(sao), owf=owf, gop=gop, cu=False, extra=extra)
    stream = open(os.path.join(workdir, "out.hevc"), "rb").read()
    return rec, ec.slice_payloads(stream), len(stream)


def psnr_y(frames, rec, w, h):
    mse = np.mean([np.mean((f[:w * h].astype(np.float64) - r[:w * h].astype(np.float64)) ** 2) for f, r in zip(frames, rec)])
    return round(float(10 * np.log10(255.0 ** 2 / mse)), 3) if mse > 0 else 999.99


def case_entry(clip, gop, sim, intra_sim, oracle, lib, workdir, counts):
    name, w, h, n, qp, preset, dbk, sao, owf, _ = clip
    frames = ic.case_frames(clip)
    rec, payloads, stream_bytes = reference(clip, gop, workdir, ("--no-bipred",))
    for k in range(1, n):
        assert payloads[k][0] >> 3 == 0b11010, (name, k, "the slice header does not say slice_type P", format(payloads[k][0], "08b"))
    rec_b, payloads_b, stream_bytes_b = reference(clip, gop, workdir, ())
    for k in range(1, n):
        assert payloads_b[k][0] >> 5 == 0b111, (name, k, "the encode without --no-bipred is not of B slices (1 1 1: slice_type 0)")
    assert any(ilc.sha(rec[k]) != ilc.sha(rec_b[k]) for k in range(1, n)), (name, "the P encode's pictures are the B encode's")
    entry = {"rec": [ilc.sha(r) for r in rec], "bytes": stream_bytes, "psnr_y": psnr_y(frames, rec, w, h),
             "b_encode": {"bytes": stream_bytes_b, "psnr_y": psnr_y(frames, rec_b, w, h)}, "gop": gop}
    ilc.mul24_violations(sim, reset=True)
    chain = pc.sim_chain(sim, intra_sim, oracle, lib, clip, gop, pc.P, counts)
    assert ilc.mul24_violations(sim) == 0, (name, "a 24-bit multiply with an operand out of range")
    slices = [None]
    for k in range(n):
        assert ilc.sha(chain["final"][k]) == entry["rec"][k], (name, k, "the simulated chain does not reproduce the reference's picture")
        if k > 0:
            data, sizes = chain["slices"][k]
            total = sum(sizes)
            ref_data, header = payloads[k][len(payloads[k]) - total:], payloads[k][:len(payloads[k]) - total]
            assert ec.header_ends_with_entry_points(header, sizes, True), (name, k, "the slice header's entry points are not these substream sizes")
            assert ref_data == data, (name, k, "the P-slice coder simulation does not reproduce the reference's slice data")
            slices.append({"sha": ilc.sha(np.frombuffer(ref_data, np.uint8)), "sizes": sizes})
    entry["slices"], entry["qps"] = slices, chain["qps"]
    print(name, gop, chain["qps"], "P", entry["bytes"], entry["psnr_y"], "B", entry["b_encode"], flush=True)
    return entry


def main():
    import kvazaar_amd
    lib = C.CDLL(kvazaar_amd.build_library())  # host-side functions only: the cost model of a QP
    sim, intra_sim, oracle = pc.load_sim(), slc.load_sim(), flatapi.load_oracle()
    out, counts = {}, {}
    with tempfile.TemporaryDirectory() as d:
        for clip, gop in pc.CLIPS:
            out[clip[0]] = case_entry(clip, gop, sim, intra_sim, oracle, lib, d, counts)
    print("census", counts)
    assert counts["mv_dir_not_1"] == 0 and counts["merge_list_unknown"] == 0, counts
    short = {k: counts[k] for k in pc.CENSUS_REQUIRED if counts[k] < pc.CENSUS_MIN}
    assert not short, ("the set reaches fewer than", pc.CENSUS_MIN, "of", short)
    out["census"] = counts
    json.dump(out, open(pc.FIXTURE, "w"), indent=0, sort_keys=True)
    print("wrote inter_p.json:", len(out), "entries")


if __name__ == "__main__":
    main()
