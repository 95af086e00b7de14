"""The entropy coder on constructed decisions, without a GPU (tests/entropy_atlas.py; the device's half is tests/test_gpu_entropy_paths.py):
  - the census: the atlas reaches every branch of the slice-data syntax the issue of this work lists, counted in Python from the inputs alone;
  - the device sources in host simulation (tests/hostsim: kvz_hostsim_entropy_code_tiles, kvz_hostsim_entropy_code_inter) write the oracle's bytes for every atlas
    picture, so a later difference on the device lies on the device's side of the simulation;
  - the emulation prevention rule by position (kvz_entropy.hpp entropy_escape_at / entropy_escape_chunk) equals the serial rule on the stage pictures' raw bytes;
  - sensitivity: one token changed changes the oracle's bytes -- the comparison would notice a coder that ignored it.
Not built: a 64x64 inter CU WITH levels.  kvazaar codes it as four 32x32 luma transform blocks; the inter pass never makes one (its PU depth starts at 1) and neither the
device's coder nor the oracle's walks that transform tree, so the atlas has 64x64 inter CUs skipped or with root cbf 0 only.
A level of -32768: the oracle takes |level| in int, so it is accepted and part of the atlas."""
import copy
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import entropy_atlas as ea
import entropy_common as ec
import flatapi

FLOOR = 16  # occurrences of every census line


@pytest.fixture(scope="module")
def hostsim_cdll():
    return C.CDLL(flatapi.hostsim_path())


@pytest.fixture(scope="module")
def intra_census():
    c = Counter()
    for name, w, h, sw, pictures in ea.intra_groups():
        for k, p in enumerate(pictures):
            ea.intra_census(c, p, dict(sw, not_last=sw["not_last"][k] if sw["not_last"] else 0))
    return c


def lacking(c, keys):
    return [(k, c[k]) for k in keys if c[k] < FLOOR]


def test_python_scan_orders_are_the_oracles(oracle):
    for log2 in (2, 3, 4, 5):
        for mode in ((0, 1, 2) if log2 <= 3 else (0,)):
            tab = oracle.lib.kvz_oracle_scan_table(mode, log2)
            assert [int(tab[i]) for i in range(1 << (2 * log2))] == ea.scan_positions(mode, log2).tolist(), (mode, log2)


def test_intra_atlas_sizes_and_switches():
    groups = ea.intra_groups()
    sizes = {(w, h) for _, w, h, _, _ in groups}
    assert all(64 <= w <= 264 and 64 <= h <= 200 for w, h in sizes)
    assert {(w + 63) // 64 for w, _ in sizes} >= {1, 2, 3, 5}
    assert any(w % 64 and not h % 64 for w, h in sizes) and any(h % 64 and not w % 64 for w, h in sizes) and any(w % 64 and h % 64 for w, h in sizes)
    for key in ("no_wpp", "sao", "nxn", "signhide"):
        assert {bool(sw[key]) for _, _, _, sw, _ in groups} == {False, True}, key
    assert {sw["qp"] for _, _, _, sw, _ in groups} == {0, 22, 51}
    assert any(len(pictures) > 1 for _, _, _, _, pictures in groups)


def test_intra_census_coding_tree(intra_census):
    c = intra_census
    keys = [("split flag", d, v) for d in (0, 1, 2) for v in (0, 1)]
    keys += [("implicit split", "children " + s) for s in ("0", "01", "02", "0123")]
    keys += [("luma mode", size, m) for size in (64, 32, 16, 8, "NxN") for m in range(35)]
    keys += [("scan order", what, scan) for what in ("luma 4x4", "luma 8x8", "chroma 4x4") for scan in (0, 1, 2)]
    keys += [("mpm index", i) for i in range(3)] + [("mpm remainder",), ("NxN CU with four different modes",), ("part mode", "NxN"), ("part mode", "2Nx2N")]
    keys += [("neighbours", l, a) for l in ("left", "no left") for a in ("above", "no above")]
    keys += [("coded block flags (Y, U, V)", y, u, v) for y in (False, True) for u in (False, True) for v in (False, True)]
    keys += [("ctu", "no level"), ("ctu", "levels")]
    assert not lacking(c, keys)


def test_intra_census_residual(intra_census):
    c = intra_census
    keys = []
    for w in (4, 8, 16, 32):
        keys += [("last at corner", w, name) for name in ("top-left", "top-right", "bottom-left", "bottom-right")]
        keys += [("last in first group", w), ("last in last group", w), ("more than 8 levels above 1 in a group", w), ("escape prefix", w), ("level -32768", w)]
        keys += [("rice parameter", w, r) for r in range(5)] + [("level magnitude", w, v) for v in (300, 3000, 32767)]
        keys += [("sign hidden", w), ("sign not hidden", w)]
        if w > 4:  # (a 4x4 block is one group)
            keys.append(("zero group between coded ones", w))
    assert not lacking(c, keys)


def test_intra_census_sao_and_substream_ends(intra_census):
    c = intra_census
    keys = [("sao", "no syntax")] + [("sao type", plane, t) for plane in ("luma", "chroma") for t in ("off", "band", "edge")]
    keys += [("sao edge class", k) for k in range(4)] + [("sao band position", 0), ("sao band position", 31), ("sao offset", 0), ("sao offset", 7), ("sao offset", -7)]
    keys += [("sao merge", "left", "", ""), ("sao merge", "left", "", "first row"), ("sao merge", "up", "", ""), ("sao merge", "up", "first column", ""),
             ("sao merge", "none", "first column", ""), ("sao merge", "none", "", "first row"), ("sao merge", "none", "first column", "first row")]
    keys += [("end of substream", k) for k in ("row with wpp", "last row with wpp", "picture without wpp", "tile that is not the last")]
    assert not lacking(c, keys)
    assert not [k for k in c if k[0] == "sao merge" and ((k[1] == "left" and k[2]) or (k[1] == "up" and k[3]))]  # no merge candidate outside the picture


def test_b_atlas_records_and_census():
    c = Counter()
    groups = ea.b_groups()
    assert all(64 <= w <= 200 and 64 <= h <= 136 for _, w, h, _, _ in groups) and {sw["poc"] for _, _, _, sw, _ in groups} == {1, 3}
    for name, w, h, sw, pictures in groups:
        for p in pictures:
            ea.check_b_records(p)
            ea.b_census(c, p)
            assert (sw["poc"] > 1) == bool((p.ref_cu["type"] == 2).any())  # POC 3: reference records that carry motion
    keys = [("skip, merge index", i) for i in range(5)] + [("merge without skip, merge index", i) for i in range(5)]
    keys += [("inter_dir", d, depth) for d in ("L0", "L1", "BI") for depth in range(4)]
    keys += [("mvd component", v) for v in (0, 1, -1, 2, -2, "large")] + [("mvp index", 0), ("mvp index", 1), ("root cbf", 0), ("root cbf", 1), ("64x64 inter CU",)]
    keys += [("inter coded block flags (Y, U, V)", y, u, v) for y in (False, True) for u in (False, True) for v in (False, True) if y or u or v]
    keys += [("intra CU in the B slice, scan order", s) for s in range(3)] + [("skip flag context", n) for n in range(3)]
    assert not lacking(c, keys)
    assert max(abs(int(v)) for _, _, _, _, pictures in groups for p in pictures for v in p.cu["mv"].reshape(-1)) > 1 << 13  # large vectors, up to 2^14


@pytest.fixture(scope="module")
def stage_oracle(oracle):
    return [(g, ec.atlas_oracle_group(oracle, g)) for g in ea.stage_groups()]


def substreams(data, sizes):
    at = 0
    for s in sizes:
        yield data[at:at + s]
        at += s


def test_stage_census(stage_oracle):
    """what the stage pictures ask of the device-only kernels, from the oracle's bytes and the compaction kernel's piece split (chunk = ceil(n / 256) raw bytes)"""
    rows = {}
    for (name, w, h, sw, pictures), coded in stage_oracle:
        rows[name] = [ea.stage_census(s) for data, sizes in coded for s in substreams(data, sizes)]
    print({name: (len(r), sum(x[2] for x in r), sum(x[3] for x in r)) for name, r in rows.items()})  # substreams, insertions, piece-border crossings
    flat = rows["flat-512-no-wpp"]
    assert max(ins for _, _, ins, _ in flat) >= 200                                     # emulation prevention bytes in one substream
    assert sum(cross for _, chunk, _, cross in flat if chunk <= 4) >= 100               # insertions whose zeros begin in an earlier piece, small pieces
    assert sum(cross for _, chunk, _, cross in flat if chunk >= 32) >= 8                # ... and large ones
    small = [x for x in rows["flat-512x128-wpp"] + rows["tall-272-substreams"] if x[0] < 256 and x[2] > 0]
    assert len(small) >= FLOOR                                                          # one byte per thread, the tail threads idle
    tall = rows["tall-272-substreams"]
    assert len(tall) > 256                                                              # the offsets scan's second block
    assert sum(x[2] == 0 for x in tall) >= FLOOR and sum(x[2] >= 2 for x in tall) >= FLOOR  # substreams without an insertion beside substreams with several


def test_host_simulation_writes_the_oracles_bytes_intra(oracle, hostsim_cdll):
    for g in ea.intra_groups():
        assert ec.atlas_hostsim_group(oracle, hostsim_cdll, g) == ec.atlas_oracle_group(oracle, g), g[0]


def test_host_simulation_writes_the_oracles_bytes_b(oracle, hostsim_cdll):
    for name, w, h, sw, pictures in ea.b_groups():
        for k, p in enumerate(pictures):
            assert ec.hostsim_entropy_b(oracle, hostsim_cdll, sw, w, h, p) == ec.oracle_entropy_b(oracle, sw, w, h, p), (name, k)


def test_host_simulation_writes_the_oracles_bytes_stage(oracle, hostsim_cdll, stage_oracle):
    for g, coded in stage_oracle:
        assert ec.atlas_hostsim_group(oracle, hostsim_cdll, g) == coded, g[0]


def test_capacity_retry_in_host_simulation(oracle, hostsim_cdll):
    """a CTU whose bin list outgrows the capacity is reported, not coded (the device's `again`)"""
    g = ea.intra_groups()[0]
    with pytest.raises(AssertionError):
        ec.atlas_hostsim_group(oracle, hostsim_cdll, g, cap=16)


def test_escape_rule_by_position_on_the_stage_pictures(hostsim_cdll, stage_oracle):
    f = hostsim_cdll.kvz_hostsim_escape
    f.restype = C.c_long
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    for (name, w, h, sw, pictures), coded in stage_oracle:
        for data, sizes in coded:
            for s in substreams(data, sizes):
                raw = ea.unescape(s)
                src = np.frombuffer(raw + b"\0", np.uint8).copy()
                out = np.zeros(len(raw) * 3 // 2 + 8, np.uint8)
                n = f(src.ctypes.data, len(raw), out.ctypes.data)
                assert n == len(s) and out[:n].tobytes() == s, (name, len(raw), n, len(s))


# ---- sensitivity: one token changed, the bytes change ----
def code_intra(oracle, sw, w, h, p, not_last=0):
    return ec.oracle_entropy(oracle, ec.atlas_model(oracle, sw), w, h, p.outputs(sw["nxn"]), p.sao_bytes(), not_last)


def first_cu(p, want):
    return next((x, y, d) for x, y, d in p.leaves() if want(x, y, d))


def first_level(p, want=lambda v: True):
    for i in range(p.coeff.shape[0]):
        for at in np.nonzero(p.coeff[i])[0]:
            if want(int(p.coeff[i][at])):
                return i, int(at)
    raise LookupError


def intra_mutations():
    def mode(p, sw):
        x, y, d = first_cu(p, lambda x, y, d: d == 2)
        p.mode4[y // 4:y // 4 + 4, x // 4:x // 4 + 4] = (int(p.mode4[y // 4, x // 4]) + 5) % 35

    def split(p, sw):
        x, y, d = first_cu(p, lambda x, y, d: d == 2)
        p.depth[y // 8:y // 8 + 2, x // 8:x // 8 + 2] = 3

    def part(p, sw):
        x, y, d = first_cu(p, lambda x, y, d: d == 3 and p.part[y // 8, x // 8])
        p.part[y // 8, x // 8] = 0
        p.mode4[y // 4:y // 4 + 2, x // 4:x // 4 + 2] = p.mode4[y // 4, x // 4]

    def sign(p, sw):
        i, at = first_level(p)
        p.coeff[i][at] = -p.coeff[i][at]

    def magnitude(p, sw):
        i, at = first_level(p, lambda v: abs(v) < 1000)
        p.coeff[i][at] += 1 if p.coeff[i][at] > 0 else -1

    def flag(p, sw):  # a chroma block's levels away: its coded block flag goes to 0
        i = next(i for i in range(p.coeff.shape[0]) if p.coeff[i][4096:5120].any())
        at = 4096 + (int(np.nonzero(p.coeff[i][4096:5120])[0][0]) & ~15)
        p.coeff[i][at:at + 16] = 0

    def sao_offset(p, sw):
        lum, chro, merge = p.sao
        i = next(i for i in range(len(merge)) if merge[i] == 0 and lum[i][0] == 1)
        lum[i][5] = 3 if lum[i][5] != 3 else 2

    def sao_band(p, sw):
        lum, chro, merge = p.sao
        i = next(i for i in range(len(merge)) if merge[i] == 0 and chro[i][0] == 1)
        chro[i][3] ^= 1

    def sao_class(p, sw):
        lum, chro, merge = p.sao
        i = next(i for i in range(len(merge)) if merge[i] == 0 and lum[i][0] == 2)
        lum[i][1] ^= 1

    def sao_merge(p, sw):
        lum, chro, merge = p.sao
        i = next(i for i in range(len(merge)) if merge[i] == 1)
        merge[i] = 0

    def signhide(p, sw):
        sw["signhide"] ^= 1

    def wpp(p, sw):
        sw["no_wpp"] ^= 1

    def qp(p, sw):
        sw["qp"] = 23
    # (mutation, the group it is applied to: one whose pictures have what it changes)
    return [(mode, 3), (split, 3), (part, 3), (sign, 3), (magnitude, 3), (flag, 3), (sao_offset, 3), (sao_band, 3), (sao_class, 3), (sao_merge, 3), (signhide, 4), (wpp, 3), (qp, 3)]


@pytest.mark.parametrize("which", range(len(intra_mutations())), ids=[m.__name__ for m, _ in intra_mutations()])
def test_one_changed_token_changes_the_intra_bytes(oracle, which):
    mutate, gi = intra_mutations()[which]
    name, w, h, sw, pictures = ea.intra_groups()[gi]
    p, sw = copy.deepcopy(pictures[0]), dict(sw)
    before = code_intra(oracle, sw, w, h, p)
    mutate(p, sw)
    assert code_intra(oracle, sw, w, h, p) != before


def test_not_last_changes_the_end_of_the_tile(oracle):
    name, w, h, sw, pictures = ea.intra_groups()[0]
    assert code_intra(oracle, sw, w, h, pictures[0], 0) != code_intra(oracle, sw, w, h, pictures[0], 1)


def b_mutations():
    def cu_where(p, want):
        for y4 in range(p.h // 4):
            for x4 in range(p.w // 4):
                if want(p.cu[y4, x4]):
                    c = p.cu[y4, x4]
                    s4 = 16 >> int(c["depth"])
                    return p.cu[(y4 // s4) * s4:(y4 // s4 + 1) * s4, (x4 // s4) * s4:(x4 // s4 + 1) * s4]
        raise LookupError

    def skip_merge_index(p):
        cells = cu_where(p, lambda c: c["skipped"])
        cells["merge_idx"] = (cells["merge_idx"] + 1) % 5

    def merge_index(p):
        cells = cu_where(p, lambda c: c["merged"] and not c["skipped"])
        cells["merge_idx"] = (cells["merge_idx"] + 1) % 5

    def mvd(p):
        cells = cu_where(p, lambda c: c["type"] == 2 and not c["merged"] and c["mv_dir"] & 1)
        cells["mv"][..., 0, 0] += 1

    def mvp_index(p):  # the other predictor index with the vector kept: the index bin changes (and the difference, where the predictors differ)
        cells = cu_where(p, lambda c: c["type"] == 2 and not c["merged"] and c["mv_dir"] & 1)
        cells["mv_cand"][..., 0] ^= 1

    def inter_dir(p):  # BI -> L0
        cells = cu_where(p, lambda c: c["type"] == 2 and not c["merged"] and c["mv_dir"] == 3)
        cells["mv_dir"] = 1
        cells["mv_ref"][..., 1] = 255
        cells["mv"][..., 1, :] = 0

    def intra_mode(p):
        cells = cu_where(p, lambda c: c["type"] == 1)
        cells["mode"] = (cells["mode"] + 5) % 35

    def level_sign(p):
        i, at = first_level(p)
        p.coeff[i][at] = -p.coeff[i][at]
    return [skip_merge_index, merge_index, mvd, mvp_index, inter_dir, intra_mode, level_sign]


@pytest.mark.parametrize("mutate", b_mutations(), ids=lambda m: m.__name__)
def test_one_changed_token_changes_the_b_bytes(oracle, mutate):
    name, w, h, sw, pictures = ea.b_groups()[1]
    p = copy.deepcopy(pictures[0])
    before = ec.oracle_entropy_b(oracle, sw, w, h, p)
    mutate(p)
    assert ec.oracle_entropy_b(oracle, sw, w, h, p) != before


def test_reference_motion_reaches_the_b_bytes_from_poc_2_on(oracle):
    """the temporal MV predictor: other reference records change the bytes at POC 3 and leave them alone at POC 1"""
    for gi, changes in ((1, True), (0, False)):
        name, w, h, sw, pictures = ea.b_groups()[gi]
        changed = False
        for p in pictures:
            q = copy.deepcopy(p)
            q.ref_cu = ea._motion_reference(np.random.default_rng(1), w, h)
            changed |= ec.oracle_entropy_b(oracle, sw, w, h, q) != ec.oracle_entropy_b(oracle, sw, w, h, p)
        assert changed == changes, name
