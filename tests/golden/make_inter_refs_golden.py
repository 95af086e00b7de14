#!/usr/bin/env python3
"""Generates tests/golden/inter_refs.json from the reference encoder (oracle/_ref/kvazaar_ref, compiled by `make -C oracle _ref/kvazaar_ref`) run with --no-bipred
--ref N on the cases of tests/inter_refs_common.py CASES: the IPPP stream whose P pictures have reference lists of up to four pictures.

    python tests/golden/make_inter_refs_golden.py

Per case and per picture the fixture records what the encoder wrote while running:
  rec     sha256 prefix of the --debug reconstruction (the final picture, after the loop filters)
  slices  per P picture the sha256 prefix of the slice data -- the bytes are taken from the REFERENCE bitstream -- and the substream sizes; the slice data pins every
          CU decision, reference index, vector and level
  qps     the picture QPs;  lists  the POCs of every picture's list (kvazaar_amd.inter.reference_pocs: what the chain predicted from)
No library is preloaded into any process: the reference runs as it is built.
Asserted here, on the reference alone: every case's encode differs from the same command with --ref 1 -- picture 1, which has one picture to refer to, does not;
from picture 2 on the slice data differs in every case and the pictures differ in every case but the two of 24x16 samples (tiny-qp51, tiny-qp0), whose three CUs are
reconstructed alike under both commands while their syntax carries ref_idx_l0: "pictures_differ_from_ref1" records which --, and every inter slice header begins 1 1 010
(first_slice_segment_in_pic_flag, slice_pic_parameter_set_id 0, slice_type P) and, under --gop lp-g4d3t1 and --gop 0, goes on with the three high bits of
slice_pic_order_cnt_lsb -- 11010000 for picture 1, 11010001 for pictures 2 and 3, and so on.  Asserted with the simulated chain (tests/inter_refs_common.py sim_chain): it reproduces every picture and every slice
byte with no 24-bit multiply out of range, no record carries a reference index outside its picture's list, and every event of the census occurs at least as
often over the set as tests/inter_refs_common.py CENSUS_MIN asks."""
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
import inter_refs_common as rc  # noqa: E402
import scaling_lists_common as slc  # noqa: E402


def reference(clip, gop, workdir, ref):
    name, w, h, n, qp, preset, dbk, sao, owf, _ = clip
    rec, _ = ic.reference_encode(w, h, rc.case_frames(clip), qp, workdir, preset=preset, deblock=bool(dbk), sao=bool(sao), owf=owf, gop=gop, cu=False, extra=("--no-bipred", "--ref", str(ref)))
    stream = open(os.path.join(workdir, "out.hevc"), "rb").read()
    return rec, ec.slice_payloads(stream), len(stream)


def case_entry(case, sim, intra_sim, oracle, lib, workdir, counts):
    key, clip, gop, ref = case
    name, w, h, n, qp, preset, dbk, sao, owf, _ = clip
    rec, payloads, stream_bytes = reference(clip, gop, workdir, ref)
    for k in range(1, n):
        assert payloads[k][0] >> 3 == 0b11010, (key, k, "the slice header does not say slice_type P", format(payloads[k][0], "08b"))
        if gop != "lp-g8d4t1":  # (the three bits behind the slice type are the high bits of slice_pic_order_cnt_lsb, whose width follows the GOP)
            assert payloads[k][0] & 7 == (k >> 1) & 7, (key, k, "the slice header's first byte is not the one observed", format(payloads[k][0], "08b"))
    rec_1, payloads_1, stream_bytes_1 = reference(clip, gop, workdir, 1)
    assert ilc.sha(rec[1]) == ilc.sha(rec_1[1]) and payloads[1] == payloads_1[1], (key, "picture 1 has one picture to refer to under both commands")
    assert any(payloads[k] != payloads_1[k] for k in range(2, n)), (key, "the encode's slices are those of --ref 1")
    pictures_differ = any(ilc.sha(rec[k]) != ilc.sha(rec_1[k]) for k in range(2, n))
    assert pictures_differ or w * h <= 24 * 16, (key, "the encode's pictures are those of --ref 1")
    entry = {"rec": [ilc.sha(r) for r in rec], "bytes": stream_bytes, "ref1_encode": {"bytes": stream_bytes_1}, "gop": gop, "ref": ref, "pictures_differ_from_ref1": pictures_differ}
    ilc.mul24_violations(sim, reset=True)
    chain = rc.sim_chain(sim, intra_sim, oracle, lib, case, counts)
    assert ilc.mul24_violations(sim) == 0, (key, "a 24-bit multiply with an operand out of range")
    slices = [None]
    for k in range(n):
        assert ilc.sha(chain["final"][k]) == entry["rec"][k], (key, k, "the simulated chain does not reproduce the reference's picture")
        if k > 0:
            data, sizes = chain["slices"][k]
            total = sum(sizes)
            ref_data, header = payloads[k][len(payloads[k]) - total:], payloads[k][:len(payloads[k]) - total]
            assert ec.header_ends_with_entry_points(header, sizes, True), (key, k, "the slice header's entry points are not these substream sizes")
            assert ref_data == data, (key, k, "the coder simulation does not reproduce the reference's slice data")
            slices.append({"sha": ilc.sha(np.frombuffer(ref_data, np.uint8)), "sizes": sizes})
    entry["slices"], entry["qps"], entry["lists"] = slices, chain["qps"], chain["lists"]
    print(key, gop, "--ref", ref, chain["qps"], chain["lists"], entry["bytes"], "--ref 1:", stream_bytes_1, flush=True)
    return entry


def main():
    import kvazaar_amd
    lib = C.CDLL(kvazaar_amd.build_library())  # host-side functions only: the cost model of a QP
    sim, intra_sim, oracle = rc.load_sim(), slc.load_sim(), flatapi.load_oracle()
    out, counts = {}, {}
    with tempfile.TemporaryDirectory() as d:
        for case in rc.CASES:
            out[case[0]] = case_entry(case, sim, intra_sim, oracle, lib, d, counts)
    print("census", counts)
    assert counts["ref_idx_outside_list"] == 0, counts
    short = {k: counts[k] for k, least in rc.CENSUS_MIN.items() if counts[k] < least}
    assert not short, ("the set reaches too few of", short, rc.CENSUS_MIN)
    out["census"] = counts
    json.dump(out, open(rc.FIXTURE, "w"), indent=0, sort_keys=True)
    print("wrote inter_refs.json:", len(out), "entries")


if __name__ == "__main__":
    main()
