#!/usr/bin/env python3
"""Generates tests/golden/ctu_qp.json from the reference encoder (oracle/_ref/kvazaar_ref, compiled by `make -C oracle ref`) run with --roi, a text map per picture
on the CTU grid (cu_qp_delta with one quantisation group per CTU):

    python tests/golden/make_ctu_qp_golden.py

Per clip of tests/ctu_qp_common.py CLIPS and per picture the fixture records what the encoder wrote while running:
  rec      sha256 prefix of the --debug reconstruction before the loop filters (--no-deblock, --sao off)
  cu       digest of the CU depth / intra mode maps behind it (oracle/ref_cudump.c)
  deblock  the digest after deblocking
  sao      the digest after deblocking + SAO (--sao full)
  entropy  sha256 prefix of the slice data -- the bytes are taken from the REFERENCE bitstream -- and the substream sizes; for one clip also under an all-zero map
and, from the host simulation (tests/hostsim/hostsim_ctu_qp.cpp), the digests of the plane of CU QPs and of the CTU words, and the census of what the clip
exercises.  Asserted here before anything is written: the simulation reproduces rec and cu; the deblocking filter with a QP per edge (ctu_qp_common.deblock_cu_qps,
over tests/deblock_reference.py) applied to the simulation's picture under the simulation's CU QPs reproduces deblock -- which holds the CU QPs to the reference
too; the plain-Python rule of the CU QPs gives the simulation's; every picture differs from its encode without the map; the census is complete; an all-zero map gives
the plain encode's reconstruction; the simulation's SAO decision with every CTU under its own lambda (kvz_hostsim_sao_decide_ctu on the pictures deblock_cu_qps gives,
reconstructed by the oracle's SAO filter) reproduces sao."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ctypes as C  # noqa: E402

import ctu_qp_common as cq  # noqa: E402
import entropy_common as ec  # noqa: E402
import make_golden as mg  # noqa: E402


def slice_data(name, sim, cm, outs, workdir, zero):
    """[{sha, sizes}] per picture: the slice data taken from the REFERENCE bitstream.  Where the slice header ends follows from the substream sizes, which come from the
    host simulation's coder and which the header's own entry points must confirm; the simulation's bytes must equal the reference's"""
    w, h, no_wpp = cq.CLIPS[name][0], cq.CLIPS[name][1], cq.CLIPS[name][5]
    pictures = []
    for payload, (data, sizes) in zip(cq.reference_slice_payloads(name, workdir, zero), cq.sim_entropy(sim, cm, w, h, outs)):
        total = sum(sizes)
        ref_data, header = payload[len(payload) - total:], payload[:len(payload) - total]
        assert ec.header_ends_with_entry_points(header, sizes, not no_wpp), (name, "the slice header's entry points are not these substream sizes")
        assert ref_data == data, (name, "the host simulation's coder does not reproduce the reference's slice data")
        pictures.append({"sha": cq.sha(np.frombuffer(ref_data, np.uint8)), "sizes": sizes})
    return pictures


def clip_entry(name, sim, lib, oracle, workdir):
    w, h, seed, qp, preset, no_wpp, layouts, deltas = cq.CLIPS[name]
    frames = cq.clip_frames(name)
    roi = ("--roi", cq.roi_file(os.path.join(workdir, "roi.txt"), name))
    maps = []
    recs = mg.reference_encoder_recon(w, h, frames, qp, 0, workdir, maps, bool(no_wpp), None, False, False, preset, extra=roi)
    plain = mg.reference_encoder_recon(w, h, frames, qp, 0, workdir, None, bool(no_wpp), None, False, False, preset)
    assert all((a != b).any() for a, b in zip(recs, plain)), (name, "a picture the map does not change pins nothing")
    outs = cq.sim_pass(sim, cq.models(lib, name), w, h, frames)
    assert [cq.sha(o["rec"]) for o in outs] == [cq.sha(r) for r in recs], (name, "the host simulation does not reproduce the reference's reconstruction")
    assert [mg.cu_digest(o["depth"].reshape(h // 8, w // 8), o["mode"].reshape(h // 8, w // 8)) for o in outs] == [mg.cu_digest(d, m) for d, m in maps], (name, "CU maps")
    for i, o in enumerate(outs):
        cu_qp, ctus = cq.rule_of_outputs(w, h, no_wpp, o, cq.ctu_qps(name)[i], qp)
        assert np.array_equal(np.array(cu_qp, np.uint8).ravel(), o["cu_qp"]), (name, i, "the rule of the CU QPs")
    dbk = mg.reference_encoder_recon(w, h, frames, qp, 1, workdir, None, bool(no_wpp), None, False, False, preset, extra=roi)
    for i, (o, r) in enumerate(zip(outs, dbk)):
        assert np.array_equal(cq.deblock_cu_qps(w, h, 0, 0, o["rec"], o["depth"], o["cu_qp"]), r), (name, i, "deblocking at the simulation's CU QPs is not the reference's")
    sao = mg.reference_encoder_recon(w, h, frames, qp, 1, workdir, None, bool(no_wpp), None, False, True, preset, extra=roi)
    cm = cq.models(lib, name)
    for i, (o, d, s) in enumerate(zip(outs, dbk, sao)):
        got_d, got_s = cq.sim_loop_filters(sim, oracle, cm, i, w, h, frames[i], o)
        assert np.array_equal(got_d, d) and np.array_equal(got_s, s), (name, i, "the host simulation's SAO decision under a lambda per CTU is not the reference's")
    entry = {"rec": [cq.sha(r) for r in recs], "cu": [mg.cu_digest(d, m) for d, m in maps], "deblock": [cq.sha(r) for r in dbk], "sao": [cq.sha(r) for r in sao],
             "cu_qp": [cq.sha(o["cu_qp"]) for o in outs], "ctu_qp": [[int(v) for v in o["ctu_qp"]] for o in outs], "census": cq.census(name, [o["ctu_qp"] for o in outs])}
    entry["entropy"] = slice_data(name, sim, cm, outs, workdir, False)
    if name == cq.ZERO_MAP:  # an all-zero map: the plain encode's reconstruction, byte for byte
        zero = mg.reference_encoder_recon(w, h, frames, qp, 0, workdir, None, bool(no_wpp), None, False, False, preset, extra=("--roi", cq.roi_file(os.path.join(workdir, "zero.txt"), name, True)))
        assert all(np.array_equal(a, b) for a, b in zip(zero, plain)), (name, "an all-zero map changes the reconstruction")
        entry["plain_rec"] = [cq.sha(r) for r in plain]
        zero_cm = cq.models(lib, name, True)  # ... but other slice data: a delta of 0 in every CTU that has a coefficient
        entry["entropy_zero_map"] = slice_data(name, sim, zero_cm, cq.sim_pass(sim, zero_cm, w, h, frames), workdir, True)
        assert [p["sha"] for p in entry["entropy_zero_map"]] != [p["sha"] for p in entry["entropy"]]
    print(name, entry["census"], flush=True)
    return entry


def main():
    import kvazaar_amd
    lib = C.CDLL(kvazaar_amd.build_library())  # host-side functions only: the cost model of a QP
    sim, oracle = cq.load_sim(), cq.flatapi.load_oracle()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name in cq.CLIPS:
            out[name] = clip_entry(name, sim, lib, oracle, d)
    assert cq.census_complete({name: e["census"] for name, e in out.items()}), "the clips miss a count of the census: change their content or maps, not the count"
    wpp, raster = out["3x3"]["ctu_qp"], out["3x3-nowpp"]["ctu_qp"]
    wc = cq.grid("3x3")[0]
    assert any((a & 255) != (b & 255) for pa, pb in zip(wpp, raster) for i, (a, b) in enumerate(zip(pa, pb)) if i % wc == 0), "no row-start CTU whose predictor differs without WPP"
    json.dump(out, open(cq.FIXTURE, "w"), indent=0, sort_keys=True)
    print("wrote ctu_qp.json:", len(out), "clips")


if __name__ == "__main__":
    main()
