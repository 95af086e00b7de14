"""Helpers of the tests of the inter CTU pass's choice of integer motion search (kvz_hip_inter_params me_algorithm / me_max_steps / me_early_termination: kvazaar's
--me, --me-steps, --me-early-termination): the options and clips of tests/golden/inter_me.json, the host simulation with both forms of the inter program
(tests/hostsim/hostsim_inter_me.cpp) and the chain I picture -> loop filters -> B pictures -> loop filters -> B-slice coder on the host.  Used by
tests/test_inter_me_sim.py, tests/test_me_search_reference.py, tests/test_gpu_inter_me.py, tests/golden/make_inter_me_golden.py and tools/bench_inter_me.py.
TEST INFRASTRUCTURE -- never imported by the product."""
import ctypes as C
import json
import os

import numpy as np

import inter_common as ic
import inter_lists_common as ilc
import inter_mixed_common as imc
import scaling_lists_common as slc

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "inter_me.json")

# name -> (the reference encoder's switches, the arguments of kvazaar_amd.inter.me_search_fields)
OPTIONS = {
    "hexbs": ((), dict()),
    "dia": (("--me", "dia"), dict(me="dia")),
    "tz": (("--me", "tz"), dict(me="tz")),
    "full8": (("--me", "full8"), dict(me="full8")),
    "full16": (("--me", "full16"), dict(me="full16")),
    "full32": (("--me", "full32"), dict(me="full32")),
    "full64": (("--me", "full64"), dict(me="full64")),
    "steps1": (("--me-steps", "1"), dict(me_steps=1)),
    "steps2": (("--me-steps", "2"), dict(me_steps=2)),
    "dia-steps2": (("--me", "dia", "--me-steps", "2"), dict(me="dia", me_steps=2)),
    "et-on": (("--me-early-termination", "on"), dict(me_early_termination="on")),
    "et-off": (("--me-early-termination", "off"), dict(me_early_termination="off")),
    "tz-et-off": (("--me", "tz", "--me-early-termination", "off"), dict(me="tz", me_early_termination="off")),
    "full16-et-off": (("--me", "full16", "--me-early-termination", "off"), dict(me="full16", me_early_termination="off")),  # the search entered AT a merge candidate: no window of its own
}
ALL = tuple(OPTIONS)
# (name, width, height, frames, qp, preset, deblock, sao, owf, clip) as tests/inter_common.py CASES, low-delay encodes (--gop lp-g4d3t1); then the options run on it
CLIPS = [
    (("pan11", 136, 72, 3, 27, "veryfast", 1, 1, 0, ("motion", 5, 1.5, (11, -6))), ALL),  # every option differs from every other here
    # the fast pan: windows leave the frame on two sides, mv_allowed refuses probes (--owf 2); tz and the large windows find what hexbs does not
    (("pan37-owf2", 200, 136, 3, 27, "ultrafast", 1, 0, 2, ("motion", 5, 1.5, (37, -18))), ("hexbs", "dia", "tz", "full8", "full16", "full32", "full64")),
    (("one-ctu-qp20", 64, 64, 3, 20, "veryfast", 1, 1, 0, ("motion", 48, 1.5, (5, -3))), ("hexbs", "tz", "full16", "dia", "et-on", "steps1")),  # kvz_fast_coeff_cost: the _me_fast build
    (("pan9-qp32-owf2", 136, 72, 4, 32, "veryfast", 1, 1, 2, ("motion", 7, 1.0, (-9, 7))), ("hexbs", "tz", "full8", "et-off", "dia-steps2")),  # the _me_cabac build under the MV constraint
]
# the small clip the device tests run every option on
DEVICE_CLIP = "pan11"


def fixture():
    return json.load(open(FIXTURE))


def clip_named(name):
    return [c for c, _ in CLIPS if c[0] == name][0]


def options_of(name):
    return [o for c, o in CLIPS if c[0] == name][0]


def cases():
    return [(c[0], o) for c, opts in CLIPS for o in opts]


def key(clip_name, option):
    return f"{clip_name}/{option}"


def params_of(clip, qp, poc, option):
    """the launch's kvz_hip_inter_params: the clip's preset and switches, the option's three members"""
    from kvazaar_amd import inter
    p = ilc.params_of(clip, qp, poc)
    for k, v in inter.me_search_fields(**OPTIONS[option][1]).items():
        setattr(p, k, v)
    return p


def load_sim():
    """the simulation with both forms of the inter program and the twin of a launch that chooses its search"""
    return ilc._load_hostsim("hostsim_inter_me", ("hostsim_inter_models", "hostsim"))


def me_events(sim, reset=False):
    """what the chosen searches met since the last reset (kvz_inter_ctu_pix.inc IC_ME_EVENT), by name"""
    names = ("tz_from_zero", "star_two_rounds", "tz_distance_16", "full_extra_run", "full_extra_skipped", "merge_window_covered", "mv_refused", "leaves_left", "leaves_right",
             "leaves_top", "leaves_bottom", "dia_step_limit", "hex_step_limit", "sweeps", "sweep_acceptances")
    out = (C.c_ulonglong * 16)()
    sim.kvz_hostsim_me_events.restype = None
    sim.kvz_hostsim_me_events(out, int(reset))
    return {n: int(out[i]) for i, n in enumerate(names)}


def sim_pass(sim, pics, params, pictures, w, h):
    """kvz_hostsim_inter_pass_me on the pictures `pics` (dicts with src, ref, ref_cu) -> (rc, rec [n, fs], cu [n, h/4, w/4], coeff [n, ctus * 6144])"""
    n = len(pics)
    fs, cells, ctus = w * h * 3 // 2, (w // 4) * (h // 4), ((w + 63) // 64) * ((h + 63) // 64)
    fb, wts = imc.model_constants()
    src, ref = imc.stacked(pics, "src"), imc.stacked(pics, "ref")
    ref_cu = np.concatenate([np.ascontiguousarray(p["ref_cu"]).reshape(-1) for p in pics])
    rec, cu, coeff = np.zeros(n * fs, np.uint8), np.zeros(n * cells, ic.CU_DTYPE), np.zeros(n * ctus * 6144, np.int16)
    f = sim.kvz_hostsim_inter_pass_me
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 3 + [C.c_void_p] * 11 + [C.c_int]
    rc = f(w, h, n, C.addressof(params), pictures.ptr if pictures is not None else None, wts.ctypes.data, fb.ctypes.data, src.ctypes.data, ref.ctypes.data, ref_cu.ctypes.data,
           rec.ctypes.data, cu.ctypes.data, coeff.ctypes.data, None, 0)
    return rc, rec.reshape(n, fs), cu.reshape(n, h // 4, w // 4), coeff.reshape(n, ctus * 6144)


def me_check(sim, params, has_tiles=False, n_sets=0, joint=False):
    """the twin of the entry points' check of the three members: 0 accepted, -1 refused"""
    f = sim.kvz_hostsim_inter_me_check
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    return f(C.addressof(params), int(has_tiles), int(n_sets), int(joint))


_intra = {}


def intra_picture(intra_sim, oracle, lib, clip):
    """picture 0 of the clip through the simulation of the all-intra pass and the oracle's loop filters -> (final picture, CU records); shared by the clip's options"""
    name, w, h, n, base_qp, preset, dbk, sao, owf, _ = clip
    if name not in _intra:
        frames, qps = ic.case_frames(clip), ilc.picture_qps(clip)
        pm = slc.table(lib, [qps[0]], coeff_cabac=int(ilc.prices_with_cabac(clip, qps[0])))
        o = slc.sim_pass(intra_sim, pm, [], None, w, h, [frames[0]])[0]
        cu = ilc.intra_cu_records(o["depth"], o["mode"], w, h)
        final, _, _ = ilc.oracle_loop_filters(oracle, clip, qps[0], False, frames[0], o["rec"], cu)
        final.setflags(write=False)
        _intra[name] = (frames, qps, final, cu)
    return _intra[name]


def sim_chain(sim, intra_sim, oracle, lib, clip, option, passes=None):
    """The clip through the host simulations under `option`: picture 0 as intra_picture, every B picture through `passes` (default: kvz_hostsim_inter_pass_me) from
    the chain's own previous picture, the oracle's loop filters, the B-slice coder simulation.
    -> dict: final [n] pictures, rec [n], cu [n], coeff [n] (None for the I picture), qps, slices [n] of (bytes, sizes) or None"""
    name, w, h, n, base_qp, preset, dbk, sao, owf, _ = clip
    frames, qps, final0, cu0 = intra_picture(intra_sim, oracle, lib, clip)
    out = dict(final=[final0], cu=[cu0], coeff=[None], qps=qps, slices=[None], rec=[None])
    for k in range(1, n):
        pic = dict(src=frames[k], ref=out["final"][k - 1], ref_cu=out["cu"][k - 1])
        prm = params_of(clip, qps[k], k, option)
        rc, rec, cus, coeff = passes(pic, prm) if passes else sim_pass(sim, [pic], prm, None, w, h)
        assert rc == 0, (name, option, k, rc)
        final, recs, merge = ilc.oracle_loop_filters(oracle, clip, qps[k], True, frames[k], rec[0], cus[0])
        out["rec"].append(rec[0]); out["final"].append(final); out["cu"].append(cus[0]); out["coeff"].append(coeff[0])
        out["slices"].append(ilc.sim_slice_data(sim, oracle, w, h, qps[k], k, cus[0], out["cu"][k - 1], coeff[0], recs, merge))
    return out


def assert_chain_equals_fixture(chain, entry, what):
    """every final picture and every B picture's slice data against the fixture's entry of the case"""
    assert chain["qps"] == entry["qps"], what
    for k, final in enumerate(chain["final"]):
        assert ilc.sha(final) == entry["rec"][k], (what, k, "picture")
        if k > 0:
            data, sizes = chain["slices"][k]
            assert sizes == entry["slices"][k]["sizes"] and ilc.sha(np.frombuffer(data, np.uint8)) == entry["slices"][k]["sha"], (what, k, "slice data")
