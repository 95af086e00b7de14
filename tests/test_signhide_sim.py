"""Sign data hiding (kvz_hip_intra_cost_model::signhide, kvazaar's --signhide) without a GPU: the device sources compiled for the host with the sign-hiding
instantiations of the CTU program (tests/hostsim/hostsim_signhide.cpp).  The references exist independently of the code under test: the per-call oracle's
kvz_oracle_quant with signhide = 1 (pinned to the compiled reference by tests/test_oracle_vs_ref.py) for the rule on one block, and the reference encoder run with
--signhide (tests/golden/signhide.json, made by tests/golden/make_signhide_golden.py) for the pass and the slice data."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import ctu_common as cc
import deblock_common as dc
import flatapi
import signhide_common as sc
from flatapi import A, ptr

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as mg  # noqa: E402

RECON = json.load(open(os.path.join(HERE, "golden", "encoder_recon.json")))


@pytest.fixture(scope="module")
def sim():
    return sc.load_sim()


@pytest.fixture(scope="module")
def hiplib():
    """libkvz_hip.so for its host-side functions only (the cost model of a QP): nothing here touches a device"""
    import kvazaar_amd
    return C.CDLL(kvazaar_amd.build_library())


@pytest.fixture(scope="module")
def gold():
    return sc.fixture()


@pytest.fixture(scope="module")
def passes(sim, hiplib):
    """the host simulation of the pass on every fixture clip, computed once: name -> (table, outputs per picture)"""
    out = {}
    for clip in sc.CLIPS:
        name, w, h, n, seed, kind, qp, preset, no_wpp = clip
        pm = sc.table(hiplib, [qp] * n, **sc.switches(clip))
        out[name] = (pm, sc.sim_pass(sim, pm, w, h, sc.clip_frames(clip)))
    return out


# ---------------------------------------------------------------------------------------------------- 1. the rule on one block, against the per-call oracle
def _quant_params(qp, log2w, typ):
    """quant-generic.c:57-63 at 8 bit, I slice, flat lists -> (scale, q_bits, add): restated here, so that the constructed cases below know what they construct"""
    qs = qp if typ == 0 else (qp if qp < 30 else (qp - 6 if qp >= 43 else (29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37)[qp - 30]))
    q_bits = 14 + qs // 6 + (15 - 8 - log2w)
    return (26214, 23302, 20560, 18396, 16384, 14564)[qs % 6], q_bits, 171 << (q_bits - 9)


def _level_du(c, par):
    scale, q_bits, add = par
    level = (abs(c) * scale + add) >> q_bits
    return level, (abs(c) * scale - (level << q_bits)) >> (q_bits - 8)


def _sim_quant(sim, log2w, scan, typ, qp, coef):
    out = A(np.zeros(coef.size, np.int16))
    f = sim.kvz_hostsim_signhide_quant
    f.restype = None
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, flatapi.i16p, flatapi.i16p]
    f(log2w, scan, typ, qp, ptr(coef), ptr(out))
    return out


def _oracle_quant(oracle, log2w, scan, typ, qp, coef, signhide=1):
    p = flatapi.QuantParams(qp=qp, bitdepth=8, slice_is_intra=1, signhide=signhide, scaling_list=0, cu_is_intra=1, quant_coeff=None, dequant_coeff=None)
    out = A(np.zeros(coef.size, np.int16))
    oracle.quant(C.byref(p), ptr(coef), ptr(out), 1 << log2w, 1 << log2w, typ, scan, 1)
    return out


# the scans that occur (kvz_syntax.hpp intra_scan_order): horizontal and vertical only for 4x4 and 8x8 blocks
SHAPES = [(l2, scan) for l2 in (2, 3) for scan in (0, 1, 2)] + [(4, 0), (5, 0)]


@pytest.mark.parametrize("qp", [0, 22, 37, 51])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{1 << s[0]}x{1 << s[0]}-scan{s[1]}")
def test_shared_hiding_rule_equals_the_oracle_on_seeded_blocks(oracle, sim, shape, qp):
    """kvz_recon.hpp sign_hide_block behind quant_level == kvz_oracle_quant with signhide = 1: luma and chroma, sparse and dense blocks, small and large levels"""
    log2w, scan = shape
    rng = np.random.default_rng(1000 * log2w + 100 * scan + qp)
    n, changed = 1 << (2 * log2w), 0
    scale, q_bits, _ = _quant_params(qp, log2w, 0)
    step = (1 << q_bits) / scale  # one quantisation step in coefficient units
    for k in range(300):
        typ = (0, 2)[k & 1]
        amp = max(2.0, step * (0.8, 2.0, 6.0, 40.0)[(k >> 1) & 3])
        coef = rng.normal(0, amp, n)
        if (k >> 3) & 1:  # sparse: most groups empty, short spans
            coef *= rng.random(n) < 0.15
        coef = A(np.clip(np.rint(coef), -32768, 32767).astype(np.int16))
        got, want = _sim_quant(sim, log2w, scan, typ, qp, coef), _oracle_quant(oracle, log2w, scan, typ, qp, coef)
        assert np.array_equal(got, want), (k, typ, np.flatnonzero(got != want)[:8])
        changed += not np.array_equal(want, _oracle_quant(oracle, log2w, scan, typ, qp, coef, 0))
    assert changed > 30, changed  # the blocks are not ones the rule leaves alone


def _constructed(oracle, sim, levels_du, scan=0, qp=22, negative=(), log2w=2, group=0):
    """a block whose group `group` (scan order) holds, at scan positions 0.., coefficients with the given (level, delta_u) pairs; the rest zero.  Runs both sides,
    asserts they agree, and returns (levels before hiding, levels after) of that group in scan order."""
    par = _quant_params(qp, log2w, 0)
    by_pair = {}
    for c in range(0, 4000):
        by_pair.setdefault(_level_du(c, par), c)
    order = np.ctypeslib.as_array(oracle.lib.kvz_oracle_scan_table(scan, log2w), shape=(1 << (2 * log2w),)).copy()
    coef = np.zeros(1 << (2 * log2w), np.int16)
    for pos, pair in enumerate(levels_du):
        c = by_pair[pair]
        coef[order[16 * group + pos]] = -c if pos in negative else c
    coef = A(coef)
    before = _oracle_quant(oracle, log2w, scan, 0, qp, coef, 0)
    got, want = _sim_quant(sim, log2w, scan, 0, qp, coef), _oracle_quant(oracle, log2w, scan, 0, qp, coef)
    assert np.array_equal(got, want), (levels_du, got, want)
    other = np.setdiff1d(np.arange(coef.size), order[16 * group:16 * group + 16])
    assert np.array_equal(got[other], before[other])  # a group never changes another
    return [int(v) for v in before[order[16 * group:16 * group + 16]]], [int(v) for v in got[order[16 * group:16 * group + 16]]]


Z = (0, 0)  # a zero coefficient


def test_constructed_blocks(oracle, sim):
    """the corners of quant-generic.c:84-176, each built on purpose: the expected outcome is stated, and both sides must produce it"""
    # sum of absolute levels below 2: one level of 1 -- untouched (no group can take part)
    b, a = _constructed(oracle, sim, [(1, 20)])
    assert a == b == [1] + [0] * 15
    # span of exactly 3 (positions 0 and 3), parity wrong (1 + 2 odd, first level positive): untouched
    b, a = _constructed(oracle, sim, [(1, 20), Z, Z, (2, 30)])
    assert a == b
    # span of exactly 4, same levels: now something must change, and the parity must come out even
    b, a = _constructed(oracle, sim, [(1, 20), Z, Z, Z, (2, 30)])
    assert a != b and sum(a) % 2 == 0 and sum(abs(x - y) for x, y in zip(a, b)) == 1
    # ... and with the parity already right nothing moves
    b, a = _constructed(oracle, sim, [(1, 20), Z, Z, Z, (1, 30)])
    assert a == b
    # magnitude 1 at first_nz with delta_u <= 0 is excluded although lowering it would be cheapest (-80): the last level is lowered instead (cost -5)
    b, a = _constructed(oracle, sim, [(1, -80), Z, Z, Z, (2, -5)])
    assert a[0] == 1 and a[4] == 1
    # the same first level with a magnitude of 2 is allowed: -80 beats -5
    b, a = _constructed(oracle, sim, [(2, -80), Z, Z, Z, (1, -5)])
    assert a[0] == 1 and a[4] == 1
    # two candidates of equal cost: positions 2 and 4, both level 2 with delta_u 40 (cost -40, change +1) -- the HIGHER scan position wins
    b, a = _constructed(oracle, sim, [(1, -10), Z, (2, 40), Z, (2, 40)])
    assert a == [1, 0, 2, 0, 3] + [0] * 11
    # ... also among zero levels: zeros at positions 1 and 3 with delta_u 100 each
    b, a = _constructed(oracle, sim, [(1, -10), (0, 100), Z, (0, 100), (2, 30)])
    assert a[:5] == [1, 0, 0, 1, 2]
    # the group visited first starts its walk at last_nz: the zero at position 9 with the best price (delta_u 150) is out of reach in the block's only group ...
    b, a = _constructed(oracle, sim, [(1, -10), Z, Z, Z, (2, 30), Z, Z, Z, Z, (0, 150)])
    assert a[9] == 0 and a[4] == 3
    # ... and within reach in a group that is not the last with a level (8x8: group 0 while group 1 holds a level; cf. the walk from position 15)
    one_later = [(1, -10), Z, Z, Z, (2, 30), Z, Z, Z, Z, (0, 150)]
    par = _quant_params(22, 3, 0)
    by_pair = {}
    for c in range(0, 4000):
        by_pair.setdefault(_level_du(c, par), c)
    order = np.ctypeslib.as_array(oracle.lib.kvz_oracle_scan_table(0, 3), shape=(64,)).copy()
    coef = np.zeros(64, np.int16)
    for pos, pair in enumerate(one_later):
        coef[order[pos]] = by_pair[pair]
    coef[order[16 + 7]] = by_pair[(3, 0)]
    coef = A(coef)
    got, want = _sim_quant(sim, 3, 0, 0, 22, coef), _oracle_quant(oracle, 3, 0, 0, 22, coef)
    assert np.array_equal(got, want) and got[order[9]] == 1 and got[order[4]] == 2 and got[order[16 + 7]] == 3
    # zero levels below first_nz: a positive coefficient under a positive first level may rise (it becomes the first level, its sign is the hidden one) ...
    b, a = _constructed(oracle, sim, [(0, 160), Z, (1, -10), Z, Z, Z, (2, 30)])
    assert a[0] == 1 and a[6] == 2
    # ... a negative one may not: its sign would contradict the parity it creates; the next best candidate takes the change
    b, a = _constructed(oracle, sim, [(0, 160), Z, (1, -10), Z, Z, Z, (2, 30)], negative=(0,))
    assert a[0] == 0 and a[6] == 3
    # ... and under a NEGATIVE first level it is the negative coefficient that may (levels 1 + 1: even sum, sign bit 1)
    b, a = _constructed(oracle, sim, [(0, 160), Z, (1, -10), Z, Z, Z, (1, 30)], negative=(0, 2))
    assert a[0] == -1 and a[2] == -1 and a[6] == 1
    b, a = _constructed(oracle, sim, [(0, 160), Z, (1, -10), Z, Z, Z, (1, 30)], negative=(2,))
    assert a[0] == 0 and a[2] == -1 and a[6] == 2
    # the change carries the COEFFICIENT's sign: a negative last level of 2 with delta_u 30 goes to -3
    b, a = _constructed(oracle, sim, [(1, -10), Z, Z, Z, (2, 30)], negative=(4,))
    assert a[4] == -3


def test_delta_u_range(sim):
    """what the stages between quantisation and hiding would have to carry: -86 .. 170 in an I slice (nine bits), at every block size and QP"""
    f = sim.kvz_hostsim_signhide_delta_u
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 4
    lo, hi = 0, 0
    for log2w in (2, 3, 4, 5):
        for qp in (0, 17, 22, 37, 51):
            par = _quant_params(qp, log2w, 0)
            for c in list(range(0, 3000)) + [32767, -32768, -1234]:
                du = f(log2w, 0, qp, c)
                assert du == _level_du(c, par)[1], (log2w, qp, c)
                lo, hi = min(lo, du), max(hi, du)
    assert -86 <= lo and hi <= 170, (lo, hi)


# ---------------------------------------------------------------------------------------------------- 2. the pass, against the reference encoder
@pytest.mark.parametrize("clip", sc.CLIPS, ids=lambda c: c[0])
def test_host_pass_reproduces_the_reference_encoder_with_signhide(oracle, passes, gold, clip):
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    pm, outs = passes[name]
    g = gold[name]
    assert [sc.sha(o["rec"]) for o in outs] == g["rec"]
    assert [mg.cu_digest(o["depth"].reshape(h // 8, w // 8), o["mode"].reshape(h // 8, w // 8)) for o in outs] == g["cu"]
    assert sorted({int(v) for o in outs for v in np.unique(o["depth"])}) == g["depths"]
    if "deblock" in g:  # the host deblocking that exists, on the sign-hidden reconstruction
        deb = [dc.run_cpu(oracle.lib.kvz_oracle_deblock_frame, w, h, qp, 0, 0, o["rec"], o["depth"].reshape(h // 8, w // 8)) for o in outs]
        assert [sc.sha(d) for d in deb] == g["deblock"]
    # the switch is what makes these pictures: where the same clip has a digest without it, the two differ
    key = mg.clip_key(w, h, n, seed, kind, qp, 0, bool(no_wpp)) + ("/fast" if preset == "fast" else "")
    if key in RECON:
        assert all(a != b for i, (a, b) in enumerate(zip(g["rec"], RECON[key])) if not (kind == "adversarial" and i == 0))


def test_fixture_covers_what_it_claims(gold):
    assert gold["ultrafast-64x64-qp22"]["depths"] == [0] and gold["ultrafast-64x64-qp30"]["depths"] == [0]
    assert gold["ultrafast-200x136-qp27"]["depths"] == [0, 1, 2, 3]
    assert {2, 3} <= set(gold["ultrafast-72x88-qp12"]["depths"])
    assert {1, 2, 3} <= set(gold["fast-200x136-qp27"]["depths"]) and {1, 2, 3} <= set(gold["fast-noise-qp22"]["depths"])
    for clip in sc.CLIPS:
        changed = gold[clip[0]]["samples_changed_by_the_switch"]
        assert all(c > 1000 for i, c in enumerate(changed) if not (clip[5] == "adversarial" and i == 0)), clip[0]
    assert len(gold[sc.BENCH_CLIP[0]]["rec"]) == 8


# ---------------------------------------------------------------------------------------------------- 3. the coder
@pytest.mark.parametrize("clip", sc.CLIPS, ids=lambda c: c[0])
def test_host_coder_reproduces_the_reference_slice_data(sim, passes, gold, clip):
    """the entropy coder compiled for the host, on the host pass's outputs, the switch read from the model's row: slice data and substream sizes == the reference
    bitstream's (sim_entropy also runs every substream in counting mode and asserts the count equals what was written)"""
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    pm, outs = passes[name]
    for i, (data, sizes) in enumerate(sc.sim_entropy(sim, pm, w, h, outs)):
        assert sizes == gold[name]["entropy"][i]["sizes"], i
        assert sc.sha(np.frombuffer(data, np.uint8)) == gold[name]["entropy"][i]["sha"], i


def test_coder_without_the_switch_codes_other_bytes(sim, hiplib, passes, gold):
    """the same levels coded without the switch: one more bypass bin per hidden sign, so the bytes must differ -- the walk does read the switch"""
    clip = sc.CLIPS[2]
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    plain = sc.table(hiplib, [qp] * n, **sc.switches(clip, 0))
    for i, (data, sizes) in enumerate(sc.sim_entropy(sim, plain, w, h, passes[name][1])):
        assert sum(sizes) > sum(gold[name]["entropy"][i]["sizes"])


# ---------------------------------------------------------------------------------------------------- 4. model tables
def test_mixed_table_gives_every_picture_its_uniform_batch_result(sim, hiplib, passes, gold):
    """[p0 hidden @ 27, p0 plain @ 37, p1 plain @ 27, p1 hidden @ 37] in one batch through ONE sign-hiding instantiation: the hidden pictures are the fixture's, the
    plain ones the EXISTING goldens (encoder_recon.json, entropy.json) -- and so is their slice data"""
    w, h, n, seed, kind = 200, 136, 2, 3, "small"
    p = cc.yuv_frames(w, h, n, seed, kind)
    qps, hide = [27, 37, 27, 37], [1, 0, 0, 1]
    pm = sc.table(hiplib, qps, signhide=hide)
    assert pm.struct.n_models == 4 and [int(pm.model_of(i).signhide) for i in range(4)] == hide and [int(pm.model_of(i).qp) for i in range(4)] == qps
    outs = sc.sim_pass(sim, pm, w, h, [p[0], p[0], p[1], p[1]])
    plain = {qp: RECON[mg.clip_key(w, h, n, seed, kind, qp, 0)] for qp in (27, 37)}
    want = [gold["ultrafast-200x136-qp27"]["rec"][0], plain[37][0], plain[27][1], gold["ultrafast-200x136-qp37"]["rec"][1]]
    assert [sc.sha(o["rec"]) for o in outs] == want
    for i, name in ((0, "ultrafast-200x136-qp27"), (3, "ultrafast-200x136-qp37")):  # ... output by output what the uniform batch computed
        assert not cc.compare(outs[i], passes[name][1][i & 1]), i
    entropy = json.load(open(os.path.join(HERE, "golden", "entropy.json")))["partial-ctus-qp27"]  # the same clip at QP 27, without the switch
    coded = sc.sim_entropy(sim, pm, w, h, outs)
    want = [gold["ultrafast-200x136-qp27"]["entropy"][0], None, entropy[1], gold["ultrafast-200x136-qp37"]["entropy"][1]]
    for i, g in enumerate(want):
        if g is not None:
            assert coded[i][1] == g["sizes"] and sc.sha(np.frombuffer(coded[i][0], np.uint8)) == g["sha"], i
    uniform = sc.table(hiplib, [37, 37])
    alone = sc.sim_entropy(sim, uniform, w, h, sc.sim_pass(sim, uniform, w, h, p))
    assert coded[1] == alone[0]


def test_tables_and_models_the_library_refuses(sim, hiplib, capfd):
    check = sim.kvz_hostsim_picture_models_check
    check.restype = C.c_int
    check.argtypes = [C.c_void_p, C.c_int, C.c_int]
    ok = sc.table(hiplib, [22, 32], signhide=[1, 0])
    assert check(C.addressof(ok.struct), 2, 1) == 0  # the models of one launch may differ in the switch
    assert check(C.addressof(ok.struct), 2, 0) == -1  # model tables need the ticket schedule
    one = sim.kvz_hostsim_signhide_model_check
    one.restype = C.c_int
    one.argtypes = [C.c_void_p, C.c_int]
    for sw in (dict(rdoq=1, coeff_cabac=1, search_32x32=1), dict(search_nxn=1, coeff_cabac=1, search_32x32=1)):
        pm = sc.table(hiplib, [27, 37], signhide=1, **sw)
        assert check(C.addressof(pm.struct), 2, 1) == -1, sw
        assert one(C.addressof(pm.models[0]), 1) == -1, sw
        assert "signhide together with" in capfd.readouterr().err
        pm = sc.table(hiplib, [27, 37], **sw)  # ... and it is the switch that is refused
        assert check(C.addressof(pm.struct), 2, 1) == 0 and one(C.addressof(pm.models[0]), 1) == 0
        assert sc.sim_pass(sim, sc.table(hiplib, [27], signhide=1, **sw), 64, 64, [np.zeros(6144, np.uint8)]) is None  # nothing is computed
    m = sc.table(hiplib, [27], signhide=1).models[0]
    assert one(C.addressof(m), 1) == 0 and one(C.addressof(m), 0) == -1  # KVZ_HIP_SCHED=wave
    assert "ticket schedule" in capfd.readouterr().err
    m.signhide = 0
    assert one(C.addressof(m), 0) == 0


def test_abi(hiplib):
    """the switch sits at the END of kvz_hip_intra_cost_model, kvz_hip_intra_cost_model_init clears it, and the Python view has it as a FIELD (a ctypes setattr of an
    unknown name would silently create an attribute the library never sees)"""
    from kvazaar_amd.batch import CostModel, cost_model
    assert CostModel._fields_[-1][0] == "signhide" and CostModel.signhide.offset + 4 <= C.sizeof(CostModel)
    assert CostModel.signhide.offset >= CostModel.entropy_fbits.offset + 512
    m = cost_model(hiplib, 22)
    assert m.struct_size == C.sizeof(CostModel) and m.signhide == 0
    text = open(os.path.join(flatapi.ROOT, "include", "kvz_hip_types.h")).read()
    body = text[text.index("typedef struct kvz_hip_intra_cost_model"):text.index("} kvz_hip_intra_cost_model;")]
    assert body.rstrip().endswith("int32_t  signhide;")


# ---------------------------------------------------------------------------------------------------- 5. against the encoder run live
def test_live_reference_encoder(passes, tmp_path):
    """where oracle/_ref is built: one clip against the encoder run now, as tests/test_encoder_parity.py does for the fixtures without the switch"""
    if not os.path.exists(os.path.join(flatapi.ROOT, "oracle", "_ref", "kvazaar_ref")):
        pytest.skip("oracle/_ref not built (the GPU box): the committed digests are the check there")
    clip = sc.CLIPS[1]
    name, w, h, n, seed, kind, qp, preset, no_wpp = clip
    recs = mg.reference_encoder_recon(w, h, sc.clip_frames(clip), qp, 0, str(tmp_path), None, bool(no_wpp), None, False, False, preset, extra=("--signhide",))
    assert [sc.sha(r) for r in recs] == [sc.sha(o["rec"]) for o in passes[name][1]]
