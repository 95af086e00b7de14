"""The deblocking filter a third time, in plain Python integers: H.265 clause 8.7.2 with kvazaar's behaviour (filter.c) -- one QP per picture, 8 bit, 4:2:0,
chroma only at boundary strength 2, every vertical edge of the picture first and every horizontal edge on the result.  Written from the standard and from
filter.c, not from the device code or the C oracle, so that the three can be held against each other (tests/test_deblock_paths.py).

Every function reports which way it went: luma_part / chroma_part return the path and the per-line events, the picture-level functions a census (a Counter)
of them per plane and direction, and for inter pictures of the exits of the boundary-strength rule with the value returned.

`mut` names ONE deliberate one-token error (MUTATIONS); the tests use it to show that their inputs would notice that error."""
from collections import Counter

import numpy as np

# H.265 Table 8-12, value by value: beta' for Q = 0 .. 51
BETA_TABLE = [
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 0, 6, 7, 8, 9,
    10, 11, 12, 13, 14, 15, 16, 17, 18, 20,
    22, 24, 26, 28, 30, 32, 34, 36, 38, 40,
    42, 44, 46, 48, 50, 52, 54, 56, 58, 60,
    62, 64]
# ... and tc' for Q = 0 .. 53
TC_TABLE = [
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 0, 0, 0, 1, 1,
    1, 1, 1, 1, 1, 1, 1, 2, 2, 2,
    2, 3, 3, 3, 3, 4, 4, 4, 5, 5,
    6, 6, 7, 8, 9, 10, 11, 13, 14, 16,
    18, 20, 22, 24]
# H.265 Table 8-10 (ChromaArrayType 1): QpC for qPi = 0 .. 57
CHROMA_QP_TABLE = [
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9,
    10, 11, 12, 13, 14, 15, 16, 17, 18, 19,
    20, 21, 22, 23, 24, 25, 26, 27, 28, 29,
    29, 30, 31, 32, 33, 33, 34, 34, 35, 35,
    36, 36, 37, 37, 38, 39, 40, 41, 42, 43,
    44, 45, 46, 47, 48, 49, 50, 51]
assert len(BETA_TABLE) == 52 and len(TC_TABLE) == 54 and len(CHROMA_QP_TABLE) == 58

MUTATIONS = {
    "cut_le": "|delta| < 10 tc  ->  <=",
    "tc2_round": "tc >> 1  ->  (tc + 1) >> 1",
    "strong_beta3": "beta >> 2  ->  beta >> 3 in the strong test",
    "strong_5tc": "(5 tc + 1) >> 1  ->  (5 tc) >> 1",
    "side_beta3": "(beta + (beta >> 1)) >> 3  ->  beta >> 3",
    "no_clip255": "the clip at 255 dropped (wraps to uint8)",
    "no_clip0": "the clip at 0 dropped (wraps to uint8)",
    "strong_clip_tc": "the strong clip +- 2 tc  ->  +- tc",
    "tc1_index": "strength-1 tc index qp + 2 tc_off  ->  qp + 2 + 2 tc_off",
    "tc_clip51": "tc index clip 53  ->  51",
    "chroma_tc_luma_qp": "chroma tc from qp instead of the chroma QP",
    "far_gt4": "vectors far apart: >= 4  ->  > 4",
    "b_same_or": "B slice, one picture twice: straight and crossed  ->  or",
}
LUMA_MUTATIONS = ["cut_le", "tc2_round", "strong_beta3", "strong_5tc", "side_beta3", "no_clip255", "no_clip0", "strong_clip_tc", "tc_clip51"]
CHROMA_MUTATIONS = ["chroma_tc_luma_qp"]
INTER_MUTATIONS = ["tc1_index", "far_gt4", "b_same_or"]

LUMA_PATHS = ["off", "strong", "weak_pq", "weak_p", "weak_q", "weak_none"]
LUMA_EVENTS = ["line_cut", "delta_clipped", "strong_clipped", "clip0", "clip255"]
CHROMA_EVENTS = ["delta_clipped", "clip0", "clip255"]
# exits of the boundary-strength rule (filter.c:405-493) with the values each can return
STRENGTH_EXITS_P = [("intra", 2), ("cbf", 1), ("uni", 1), ("p_slice", 0)]
STRENGTH_EXITS_B = [("intra", 2), ("cbf", 1), ("uni", 1), ("b_diff", 1), ("b_straight", 0), ("b_straight", 1), ("b_crossed", 0), ("b_crossed", 1),
                    ("b_same_twice", 0), ("b_same_twice", 1)]


def clip3(lo, hi, v):
    return lo if v < lo else (hi if v > hi else v)


def thresholds(qp, beta_off, tc_off, mut=None):
    """(beta, tc at strength 2, tc at strength 1, chroma tc) of a picture at `qp` with slice_beta_offset_div2 / slice_tc_offset_div2 (8.7.2.5.3, 8.7.2.5.5)"""
    top = 51 if mut == "tc_clip51" else 53
    beta = BETA_TABLE[clip3(0, 51, qp + 2 * beta_off)]
    tc = TC_TABLE[clip3(0, top, qp + 2 * (2 - 1) + 2 * tc_off)]
    tc1 = TC_TABLE[clip3(0, top, qp + (2 if mut == "tc1_index" else 0) + 2 * tc_off)]
    qp_c = qp if mut == "chroma_tc_luma_qp" else CHROMA_QP_TABLE[qp]
    tc_c = TC_TABLE[clip3(0, top, qp_c + 2 + 2 * tc_off)]
    return beta, tc, tc1, tc_c


def _pixel(v, events, mut):
    """Clip1 of a filtered sample"""
    if v < 0:
        events.append("clip0")
        return v & 255 if mut == "no_clip0" else 0
    if v > 255:
        events.append("clip255")
        return v & 255 if mut == "no_clip255" else 255
    return v


def luma_decision(l0, l3, beta, tc, mut=None):
    """What lines 0 and 3 decide for the whole part: "off", "strong", or "weak_" + which of p1 / q1 the weak filter also modifies"""
    dp0, dq0 = abs(l0[1] - 2 * l0[2] + l0[3]), abs(l0[4] - 2 * l0[5] + l0[6])
    dp3, dq3 = abs(l3[1] - 2 * l3[2] + l3[3]), abs(l3[4] - 2 * l3[5] + l3[6])
    dp, dq = dp0 + dp3, dq0 + dq3
    if dp + dq >= beta:
        return "off"
    flat = beta >> (3 if mut == "strong_beta3" else 2)
    step = (5 * tc + (0 if mut == "strong_5tc" else 1)) >> 1
    if (2 * (dp0 + dq0) < flat and 2 * (dp3 + dq3) < flat and abs(l0[3] - l0[4]) < step and abs(l3[3] - l3[4]) < step
            and abs(l0[0] - l0[3]) + abs(l0[4] - l0[7]) < (beta >> 3) and abs(l3[0] - l3[3]) + abs(l3[4] - l3[7]) < (beta >> 3)):
        return "strong"
    side = beta >> 3 if mut == "side_beta3" else (beta + (beta >> 1)) >> 3
    p_2nd, q_2nd = dp < side, dq < side
    return "weak_" + (("pq" if q_2nd else "p") if p_2nd else ("q" if q_2nd else "none"))


def luma_part(b, beta, tc, mut=None, path=None):
    """One 4-line part of a luma edge.  b: 4 lines of 8 samples p3 p2 p1 p0 | q0 q1 q2 q3.  Returns (the 4 new lines, path, per-line events).
    path: luma_decision(b[0], b[3], ...) where the caller already has it."""
    if path is None:
        path = luma_decision(b[0], b[3], beta, tc, mut)
    if path == "off":
        return b, "off", []
    strong = path == "strong"
    events, out = [], []
    if strong:
        t2 = tc if mut == "strong_clip_tc" else 2 * tc
        for m0, m1, m2, m3, m4, m5, m6, m7 in b:
            raw = ((2 * m0 + 3 * m1 + m2 + m3 + m4 + 4) >> 3, (m1 + m2 + m3 + m4 + 2) >> 2, (m1 + 2 * m2 + 2 * m3 + 2 * m4 + m5 + 4) >> 3,
                   (m2 + 2 * m3 + 2 * m4 + 2 * m5 + m6 + 4) >> 3, (m3 + m4 + m5 + m6 + 2) >> 2, (m3 + m4 + m5 + 3 * m6 + 2 * m7 + 4) >> 3)
            new = [clip3(m - t2, m + t2, r) for m, r in zip((m1, m2, m3, m4, m5, m6), raw)]
            if any(n != r for n, r in zip(new, raw)):
                events.append("strong_clipped")
            out.append([m0] + new + [m7])
        return out, "strong", events
    p_2nd, q_2nd = path in ("weak_pq", "weak_p"), path in ("weak_pq", "weak_q")
    tc2 = (tc + 1) >> 1 if mut == "tc2_round" else tc >> 1
    for m0, m1, m2, m3, m4, m5, m6, m7 in b:
        delta = (9 * (m4 - m3) - 3 * (m5 - m2) + 8) >> 4
        if abs(delta) > 10 * tc or (abs(delta) == 10 * tc and mut != "cut_le"):
            events.append("line_cut")
            out.append([m0, m1, m2, m3, m4, m5, m6, m7])
            continue
        d = clip3(-tc, tc, delta)
        if d != delta:
            events.append("delta_clipped")
        n2, n5 = m2, m5
        n3, n4 = _pixel(m3 + d, events, mut), _pixel(m4 - d, events, mut)
        if p_2nd:
            n2 = _pixel(m2 + clip3(-tc2, tc2, (((m1 + m3 + 1) >> 1) - m2 + d) >> 1), events, mut)
        if q_2nd:
            n5 = _pixel(m5 + clip3(-tc2, tc2, (((m6 + m4 + 1) >> 1) - m5 - d) >> 1), events, mut)
        out.append([m0, m1, n2, n3, n4, n5, m6, m7])
    return out, path, events


def chroma_part(b, tc_c, mut=None):
    """One 4-line part of a chroma edge.  b: 4 lines of 4 samples p1 p0 | q0 q1.  Returns (new lines, "filtered", per-line events)."""
    events, out = [], []
    for m2, m3, m4, m5 in b:
        delta = (((m4 - m3) * 4) + m2 - m5 + 4) >> 3
        d = clip3(-tc_c, tc_c, delta)
        if d != delta:
            events.append("delta_clipped")
        out.append([m2, _pixel(m3 + d, events, mut), _pixel(m4 - d, events, mut), m5])
    return out, "filtered", events


# ---- picture level -------------------------------------------------------------------------------------------------------------------------------------------
def _filter_picture(w, h, thr, frame, unit_edge, part_strength, mut):
    """unit_edge(x, y, vertical) -> (filtered, on a transform edge) for the 8x8 unit at (x, y); part_strength(x, y, vertical, tu_edge, census) -> 0 / 1 / 2 for
    the 4-sample part whose first q sample is (x, y)"""
    beta, tc, tc1, tc_c = thr
    n, cw, ch = w * h, w // 2, h // 2
    flat = np.asarray(frame, np.uint8)
    Y, U, V = flat[:n].tolist(), flat[n:n + n // 4].tolist(), flat[n + n // 4:n + n // 2].tolist()
    census = Counter()
    for vertical in (True, False):
        name = "ver" if vertical else "hor"
        across, along = (1, w) if vertical else (w, 1)
        across_c, along_c = (1, cw) if vertical else (cw, 1)
        for ey in range(0, h, 8):
            for ex in range(0, w, 8):
                if (ex if vertical else ey) == 0:
                    continue
                on, tu_edge = unit_edge(ex, ey, vertical)
                if not on:
                    continue
                for part in range(2):
                    px, py = (ex, ey + 4 * part) if vertical else (ex + 4 * part, ey)
                    s = part_strength(px, py, vertical, tu_edge, census)
                    if s == 0:
                        census["luma", name, "bs0"] += 1
                        continue
                    at = py * w + px
                    tc_s = tc if s == 2 else tc1
                    l0, l3 = [Y[at + k * across] for k in range(-4, 4)], [Y[at + 3 * along + k * across] for k in range(-4, 4)]
                    path = luma_decision(l0, l3, beta, tc_s, mut)  # lines 1 and 2 are only read where the part is filtered
                    if path == "off":
                        census["luma", name, "off"] += 1
                        continue
                    b = [l0, [Y[at + along + k * across] for k in range(-4, 4)], [Y[at + 2 * along + k * across] for k in range(-4, 4)], l3]
                    new, path, events = luma_part(b, beta, tc_s, mut, path)
                    census["luma", name, path] += 1
                    for e in events:
                        census["luma", name, e] += 1
                    for i in range(4):
                        for k in range(1, 7):
                            Y[at + i * along + (k - 4) * across] = new[i][k]
                # chroma: edges on the 8-sample chroma grid, one 4-sample part per 8x8 luma unit, only at strength 2
                xc, yc = ex >> 1, ey >> 1
                if (xc if vertical else yc) & 7:
                    continue
                if part_strength(ex, ey, vertical, tu_edge, None) != 2:
                    continue
                at = yc * cw + xc
                for plane in (U, V):
                    b = [[plane[at + i * along_c + (k - 2) * across_c] for k in range(4)] for i in range(4)]
                    new, _, events = chroma_part(b, tc_c, mut)
                    census["chroma", name, "filtered"] += 1
                    for e in events:
                        census["chroma", name, e] += 1
                    for i in range(4):
                        plane[at + i * along_c - across_c], plane[at + i * along_c] = new[i][1], new[i][2]
    return np.array(Y + U + V, np.uint8), census


def deblock_intra(w, h, qp, b_off, t_off, frame, cu_depth, mut=None):
    """All-intra picture, CU depth per 8x8 unit: transform units are the CUs (32x32 inside a 64x64 CU), every edge has strength 2.  -> (picture, census)"""
    depth = np.asarray(cu_depth).reshape(h // 8, w // 8).tolist()

    def unit_edge(x, y, vertical):
        d = depth[y >> 3][x >> 3]
        return ((x if vertical else y) % (64 >> max(d, 1))) == 0, True

    return _filter_picture(w, h, thresholds(qp, b_off, t_off, mut), frame, unit_edge, lambda x, y, vertical, tu_edge, census: 2, mut)


RECORD_DTYPE = np.dtype([("type", "u1"), ("depth", "u1"), ("tr_depth", "u1"), ("part_size", "u1"), ("cbf_y", "u1"), ("mv_dir", "u1"), ("mv_ref", "i1", 2),
                         ("ref_id", "<i2", 2), ("mv", "<i2", (2, 2))])  # include/kvz_hip_dev.h kvz_hip_cu_dbk
# where the partitions after the first begin, in quarters of the CU: (x offsets, y offsets) per part_size 2Nx2N, 2NxN, Nx2N, NxN, 2NxnU, 2NxnD, nLx2N, nRx2N
PU_STARTS = [((), ()), ((), (2,)), ((2,), ()), ((2,), (2,)), ((), (1,)), ((), (3,)), ((1,), ()), ((3,), ())]


def boundary_strength(p, q, tu_edge, slice_b, mut=None):
    """filter.c:405-493 for the records on the two sides of a part -> (exit, strength)"""
    if p["type"] == 1 or q["type"] == 1:
        return "intra", 2
    if tu_edge and (p["cbf_y"] or q["cbf_y"]):
        return "cbf", 1

    def far(a, b):
        return abs(a - b) > 4 if mut == "far_gt4" else abs(a - b) >= 4

    if p["mv_dir"] != 3 and q["mv_dir"] != 3:
        lp, lq = p["mv_dir"] - 1, q["mv_dir"] - 1
        if far(q["mv"][lq][0], p["mv"][lp][0]) or far(q["mv"][lq][1], p["mv"][lp][1]) or q["mv_ref"][lq] != p["mv_ref"][lp]:
            return "uni", 1
    if not slice_b:
        return "p_slice", 0
    mvp = [p["mv"][l] if p["mv_dir"] & (1 << l) else [0, 0] for l in range(2)]  # undefined vectors count as zero
    mvq = [q["mv"][l] if q["mv_dir"] & (1 << l) else [0, 0] for l in range(2)]
    rp = [p["ref_id"][l] if p["mv_dir"] & (1 << l) else -1 for l in range(2)]
    rq = [q["ref_id"][l] if q["mv_dir"] & (1 << l) else -1 for l in range(2)]
    if not ((rp[0] == rq[0] and rp[1] == rq[1]) or (rp[0] == rq[1] and rp[1] == rq[0])):
        return "b_diff", 1
    straight = far(mvq[0][0], mvp[0][0]) or far(mvq[0][1], mvp[0][1]) or far(mvq[1][0], mvp[1][0]) or far(mvq[1][1], mvp[1][1])
    crossed = far(mvq[1][0], mvp[0][0]) or far(mvq[1][1], mvp[0][1]) or far(mvq[0][0], mvp[1][0]) or far(mvq[0][1], mvp[1][1])
    if rp[0] != rp[1]:
        return ("b_straight", int(straight)) if rp[0] == rq[0] else ("b_crossed", int(crossed))
    return "b_same_twice", int((straight or crossed) if mut == "b_same_or" else (straight and crossed))


def deblock_inter(w, h, qp, b_off, t_off, frame, records, slice_b, mut=None):
    """Picture with inter CUs, one kvz_hip_cu_dbk record per 4x4 unit (a ctypes array or bytes): transform edges and the prediction edges of part_size on
    the 8x8 grid, strength per 4-sample part.  -> (picture, census); the census also counts ("bs", direction, exit, value)."""
    w4 = w // 4
    raw = np.frombuffer(bytes(records), RECORD_DTYPE, (w // 4) * (h // 4))
    rec = [dict(type=int(r["type"]), depth=int(r["depth"]), tr_depth=int(r["tr_depth"]), part_size=int(r["part_size"]), cbf_y=int(r["cbf_y"]), mv_dir=int(r["mv_dir"]),
                mv_ref=r["mv_ref"].tolist(), ref_id=r["ref_id"].tolist(), mv=r["mv"].tolist()) for r in raw]

    def unit_edge(x, y, vertical):
        u = rec[(y >> 2) * w4 + (x >> 2)]
        pos = x if vertical else y
        tu_edge = pos % (64 >> u["tr_depth"]) == 0
        cu_w = 64 >> u["depth"]
        rel = pos % cu_w
        starts = PU_STARTS[u["part_size"]][0 if vertical else 1]
        return tu_edge or rel == 0 or any(rel == s * cu_w // 4 for s in starts), tu_edge

    def part_strength(x, y, vertical, tu_edge, census):
        q = rec[(y >> 2) * w4 + (x >> 2)]
        p = rec[(y >> 2) * w4 + ((x - 1) >> 2)] if vertical else rec[((y - 1) >> 2) * w4 + (x >> 2)]
        exit_, s = boundary_strength(p, q, tu_edge, slice_b, mut)
        if census is not None:
            census["bs", "ver" if vertical else "hor", exit_, s] += 1
        return s

    return _filter_picture(w, h, thresholds(qp, b_off, t_off, mut), frame, unit_edge, part_strength, mut)
