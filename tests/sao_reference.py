"""The SAO search and filter of one picture, stated a third time: plain Python integers (numpy only as a container of samples), LCU by LCU in raster order, written
from H.265 8.7.3 / 9.3 and from what this repository's own comments say about the encoder's decision (kvazaar_amd/csrc/kvz_sao.hpp's header) -- independent of both
oracle/kvz_oracle_sao.c and kvz_sao.hpp: nothing here is derived from statistics the way the device does it, every distortion change is a sum over samples of
(orig - (rec + offset))^2 - (orig - rec)^2.

  prepare()  the picture as the search sees it (the R / V / D view rule), cut into one Block per LCU and plane; the part of the search that needs no CABAC state
  decide()   the chain: mode bits on the two SAO contexts, edge / band / none, merge candidates, merge decision, context updates and the WPP hand-off
  apply()    the filter: out = clip(in + offset); a sample with a neighbour outside the picture keeps its value

Rates are int(float64(float32(bits)) * lambda + 0.5); the 128 bit costs are data (the cost model's entropy_fbits); the two transition tables are typed out below from
H.265 Table 9-45 (tests/test_sao_paths.py holds them against kvz_oracle_next_state_table).

Two quirks of the reference that this statement reproduces on purpose:
  * band offsets: in calc_sao_band_offsets the best distance is never lowered inside the trial loop, so every trial overwrites the last one and the LAST trial -- the
    offset one step from zero -- wins: every band offset is -1, 0 or +1 (decide() asserts it of every band record).
  * the band search total can never reach INT_MAX: a band whose rounded offset is not zero runs the trial loop at least once, and a trial's distortion
    cnt o^2 - 2 o sum is bounded by 4096 * 49 + 2 * 7 * 4096 * 255 = 14 823 424 < 2^24, so the INT_MAX a band starts from is always overwritten; four such terms plus a
    rate stay far below 2^31.  The reference's `band_search < MAX_INT` test is therefore always true and the "all-zero band record" branch behind it (band_valid ==
    false in kvz_sao.hpp) is unreachable; it has no place in the census.  Block.candidates() asserts the bound on every band of every block it sees.

`mutation=` applies exactly one one-token error (MUTATIONS); `census=` (a collections.Counter) counts the events of EVENTS as they happen."""
import numpy as np

ABS_MAX = 7
INT_MAX = 0x7fffffff
B, P, I = 0, 1, 2                                   # slice types, kvazaar's numbering
INIT_MERGE, INIT_TYPE = 153, {B: 160, P: 185, I: 200}  # H.265 Tables 9-5 / 9-6: initValue of sao_merge_*_flag and sao_type_idx_* per initType
# H.265 Table 8-13 (hPos, vPos) of the two neighbours per SaoEoClass
EO_POS = {0: ((-1, 0), (1, 0)), 1: ((0, -1), (0, 1)), 2: ((-1, -1), (1, 1)), 3: ((1, -1), (-1, 1))}
# edgeIdx = 2 + sign(c - a) + sign(c - b), then 0, 1, 2 -> 1, 2, 0 (8.7.3.2): the category whose offset applies
CATEGORY = np.array([1, 2, 0, 3, 4])
NONE = (0, 0, 0, (0, 0, 0, 0))                      # a record: (type 0 none / 1 band / 2 edge, class, band position, offsets of categories 1 .. 4 or bands 0 .. 3)

# H.265 Table 9-45: transIdxLps of pStateIdx 0 .. 63 (transIdxMps is pStateIdx + 1, saturating at 62; 63 stays)
TRANS_IDX_LPS = [0, 0, 1, 2, 2, 4, 4, 5, 6, 7, 8, 9, 9, 11, 11, 12, 13, 13, 15, 15, 16, 16, 18, 18, 19, 19, 21, 21, 22, 22, 23, 24,
                 24, 25, 26, 26, 27, 27, 28, 29, 29, 30, 30, 30, 31, 32, 32, 33, 33, 33, 34, 34, 35, 35, 35, 36, 36, 36, 37, 37, 37, 38, 38, 63]


def next_state_tables():
    """(after an MPS, after an LPS) over the packed state pStateIdx << 1 | valMps"""
    mps, lps = [0] * 128, [0] * 128
    for s in range(64):
        for v in range(2):
            mps[2 * s + v] = 2 * (s if s >= 62 else s + 1) + v
            lps[2 * s + v] = 2 * TRANS_IDX_LPS[s] + (v if s else 1 - v)
    return mps, lps


NEXT_MPS, NEXT_LPS = next_state_tables()

MUTATIONS = {
    "no_round": "drop the cnt >> 1 rounding term of an offset",
    "clip6": "clip offsets at 6 instead of 7",
    "no_sign12": "drop the sign rule of categories 1 - 2",
    "no_sign34": "drop the sign rule of categories 3 - 4",
    "border_stats": "count the block's first and last row into the statistics of class 0",
    "swap_23": "swap the displacements of classes 2 and 3",
    "band_first": "keep the first band trial instead of the last",
    "band_26": "search band positions 0 to 26 only",
    "edge_lt_band": "< for <= in edge against band",
    "nothing_gt": "> for >= against the cost of nothing",
    "up_lt": "< for <= in the up merge",
    "left_le_up": "<= for < in left against up",
    "up_one_bin": "price the up merge with one bin instead of two",
    "handoff_first": "hand the contexts to the next row after the first LCU instead of the second",
    "type_once": "code the type context once instead of twice per unmerged LCU",
    "uv_separate": "decide U and V separately",
    "r_col_3": "read R from column n - 3 instead of n - 4",
    "v_rows_2": "use 2 luma rows of V instead of 3",
    "v_rows_0c": "use no chroma row of V instead of 1",
    "filter_border": "make the filter modify a picture-border sample",
    "filter_noclip": "make the filter wrap instead of clip",
    "band_three": "make band SAO cover three bands instead of four",
    "merge_type_first": "price the merge flags of a candidate with the type context",
    "left_two_bins": "price the left merge with two bins",
}
VIEW_MUTATIONS = ["r_col_3", "v_rows_2", "v_rows_0c"]  # only seen with deblocking
# Two more errors of the view rule change nothing, whatever the picture: deblocking a horizontal edge writes at most 3 luma samples and 1 chroma sample on either
# side, and edges lie on the 8x8 luma grid, so V and D are the same picture on luma row n - 4 and on chroma rows n - 3 and n - 2 of an LCU.  They are kept as
# arguments of prepare() so that tests/test_sao_paths.py can state exactly that.
EQUIVALENT_VIEW_MUTATIONS = {"v_rows_4": "use 4 luma rows of V instead of 3", "v_rows_3c": "use 3 chroma rows of V instead of 1"}

GROUPS = ("Y", "C")
EVENTS = ([("type", g, t) for g in GROUPS for t in ("none", "eo0", "eo1", "eo2", "eo3", "band")]
          + [("band_pos", g, k) for g in GROUPS for k in ("0", "27", "between")]
          + [("clip", s) for s in ("+7", "-7")] + [("zeroed", c) for c in ("12", "34")] + [("cnt0",)]
          + [("pair_differs", p) for p in ("U", "V")]
          + [("tie", k) for k in ("edge==band", "cost==nothing", "up==own", "left==own", "left==up")]
          + [("merge", k) for k in ("left", "up", "no")]
          + [("merge_from", g, t) for g in GROUPS for t in ("none", "band", "edge")]
          + [("merge_of_merged",), ("band_by_merge",), ("wpp_one_wide",), ("handoff",), ("no_wpp",)]
          + [("filter_clip", k) for k in ("0", "255")]
          + [("kept", b, c) for c in range(4) for b in ("left", "right", "top", "bottom") if EO_POS[c][0][0 if b in ("left", "right") else 1]])


def tdiv(a, b):
    """C's integer division: towards zero"""
    return -((-a) // b) if a < 0 else a // b


def ctx_state(init_value, qp):
    """H.265 9.3.2.2 -> pStateIdx << 1 | valMps"""
    m, n = (init_value >> 4) * 5 - 45, ((init_value & 15) << 3) - 16
    pre = min(max(((m * min(max(qp, 0), 51)) >> 4) + n, 1), 126)
    return ((pre - 64) << 1) | 1 if pre > 63 else (63 - pre) << 1


def lambda_of(qp):
    return 0.57 * 2.0 ** ((qp - 12) / 3.0)


def rate(bits, lam):
    return int(np.float64(np.float32(bits)) * np.float64(lam) + 0.5)


def edge_offset_bits(off):
    return sum(abs(o) + 1 if abs(o) in (0, ABS_MAX) else abs(o) + 2 for o in off)


def band_offset_bits(off):
    return sum(1 if o == 0 else (abs(o) + 2 if abs(o) == ABS_MAX else abs(o) + 3) for o in off)


def offsets_of(record, cat, band, bands=4):
    """the offset each sample gets under a record -- cat: the samples' categories under the record's edge class, band: their values >> 3; bands: how many bands a
    band record covers"""
    kind, _, pos, off = record
    if kind == 2:
        return np.array((0,) + off, np.int64)[cat]
    table = np.zeros(32, np.int64)
    for k in range(bands):
        table[(pos + k) & 31] = off[k]
    return table[band]


class Block:
    """one plane of one LCU as the search sees it, and what the search finds on it without a CABAC state"""

    def __init__(self, orig, rec, mutation=None, census=None):
        self.mut = mutation
        self.rec, self.diff = rec.astype(np.int64), orig.astype(np.int64) - rec.astype(np.int64)
        bh, bw = rec.shape
        self.cat = []
        for ec in range(4):
            cls = {2: 3, 3: 2}.get(ec, ec) if mutation == "swap_23" else ec
            (ax, ay), (bx, by) = EO_POS[cls]
            y0, y1 = (0, bh) if (mutation == "border_stats" and ec == 0) else (1, bh - 1)  # the interior: the search never looks across the block's border
            cat = np.zeros((bh, bw), np.int64)
            if y1 > y0 and bw > 2:
                c = self.rec[y0:y1, 1:bw - 1]
                a, b = self.rec[y0 + ay:y1 + ay, 1 + ax:bw - 1 + ax], self.rec[y0 + by:y1 + by, 1 + bx:bw - 1 + bx]
                cat[y0:y1, 1:bw - 1] = CATEGORY[2 + np.sign(c - a) + np.sign(c - b)]
            self.cat.append(cat)
        self.band = self.rec >> 3
        self._dd = {}
        self.candidates(census)

    def offset_of(self, total, cnt, census=None):
        if cnt == 0:
            return 0
        o = tdiv(total + (0 if self.mut == "no_round" else cnt >> 1), cnt)
        top = 6 if self.mut == "clip6" else ABS_MAX
        if census is not None and abs(o) > ABS_MAX:
            census["clip", "+7" if o > 0 else "-7"] += 1
        return min(max(o, -top), top)

    def candidates(self, census):
        self.edge = []  # per class: (offsets of categories 1 .. 4, distortion change, offset bins)
        for ec in range(4):
            off = []
            for cat in range(1, 5):
                m = self.cat[ec] == cat
                cnt, total = int(m.sum()), int(self.diff[m].sum())
                if census is not None and cnt == 0:
                    census["cnt0",] += 1
                o = self.offset_of(total, cnt, census)
                if cat <= 2 and o < 0 and self.mut != "no_sign12":
                    o = 0
                    if census is not None:
                        census["zeroed", "12"] += 1
                if cat >= 3 and o > 0 and self.mut != "no_sign34":
                    o = 0
                    if census is not None:
                        census["zeroed", "34"] += 1
                off.append(o)
            off = tuple(off)
            self.edge.append((off, self.dd((2, ec, 0, off)), edge_offset_bits(off)))
        dist, offs = [0] * 32, [0] * 32
        for band in range(32):
            m = self.band == band
            cnt, total = int(m.sum()), int(self.diff[m].sum())
            o = self.offset_of(total, cnt)
            if o != 0:
                dist[band] = INT_MAX
                while o != 0:  # no trial improves on a best that is never lowered: each overwrites
                    trial = cnt * o * o - 2 * o * total
                    assert abs(trial) < 1 << 24
                    if trial < INT_MAX and (self.mut != "band_first" or dist[band] == INT_MAX):
                        dist[band], offs[band] = trial, o
                    o += -1 if o > 0 else 1
                assert dist[band] != INT_MAX
        best, pos = INT_MAX, 0
        for p in range(27 if self.mut == "band_26" else 28):
            total = dist[p] + dist[p + 1] + dist[p + 2] + dist[p + 3]
            if total < best:
                best, pos = total, p
        assert best < INT_MAX
        off = tuple(offs[pos:pos + 4])
        self.band_rec = (1, 0, pos, off)
        self.band_dd, self.band_bits = self.dd(self.band_rec), band_offset_bits(off)

    def dd(self, record):
        """sum over the samples of (orig - (rec + offset))^2 - (orig - rec)^2"""
        if record[0] == 0:
            return 0
        if record not in self._dd:
            moved = self.diff - offsets_of(record, self.cat[record[1]], self.band)
            self._dd[record] = int((moved * moved - self.diff * self.diff).sum())
        return self._dd[record]


def planes_of(w, h, frame):
    ys, cs = w * h, w * h // 4
    return [frame[:ys].reshape(h, w), frame[ys:ys + cs].reshape(h // 2, w // 2), frame[ys + cs:].reshape(h // 2, w // 2)]


def prepare(w, h, src, R, V=None, D=None, mutation=None, census=None):
    """-> [lcu][plane] Block.  R: the reconstruction before deblocking, V: after the vertical edges, D: after the horizontal edges too (None: no deblocking).  An LCU
    is searched when its right and lower neighbours are not deblocked yet: it sees R in its last four columns unless it is in the last LCU column, else V in its
    last 3 luma rows / last chroma row unless it is in the last LCU row, else D."""
    V, D = R if V is None else V, R if D is None else D
    wl, hl = (w + 63) // 64, (h + 63) // 64
    S, Rp, Vp, Dp = (planes_of(w, h, np.asarray(f)) for f in (src, R, V, D))
    blocks = []
    for ly in range(hl):
        for lx in range(wl):
            row = []
            for c in range(3):
                n = 32 if c else 64
                x0, y0 = lx * n, ly * n
                x1, y1 = min(x0 + n, w >> (c > 0)), min(y0 + n, h >> (c > 0))
                view = Dp[c][y0:y1, x0:x1].copy()
                v_rows = {"v_rows_3c": 3, "v_rows_0c": 0}.get(mutation, 1) if c else {"v_rows_4": 4, "v_rows_2": 2}.get(mutation, 3)
                if ly != hl - 1 and v_rows:
                    view[n - v_rows:, :] = Vp[c][y0 + n - v_rows:y1, x0:x1]
                if lx != wl - 1:
                    cols = 3 if mutation == "r_col_3" else 4
                    view[:, n - cols:] = Rp[c][y0:y1, x0 + n - cols:x1]
                row.append(Block(S[c][y0:y1, x0:x1], view, mutation, census))
            blocks.append(row)
    return blocks


def best_mode(blocks, ctx, lam, fb, top, left, mut, census=None, group=None):
    """the search of the luma plane or of the chroma pair -> (records, [own cost, left merge cost, up merge cost])"""
    merge_ctx, type_ctx = ctx
    flag_ctx = type_ctx if mut == "merge_type_first" else merge_ctx
    head = 0.0
    if left is not None:
        head += fb[flag_ctx ^ 0]
    if top is not None:
        head += fb[flag_ctx ^ 0]
    sao_on = head + fb[type_ctx ^ 1]
    edge_cost, edge_class = INT_MAX, 0
    for ec in range(4):
        cost = sum(b.edge[ec][1] for b in blocks) + rate(sao_on + 1.0 + sum(b.edge[ec][2] for b in blocks) + 2.0, lam)
        if cost < edge_cost:
            edge_cost, edge_class = cost, ec
    band_cost = rate(sao_on + 1.0 + sum(b.band_bits for b in blocks) + 5.0 * len(blocks), lam) + sum(b.band_dd for b in blocks)
    if (edge_cost < band_cost) if mut == "edge_lt_band" else (edge_cost <= band_cost):
        cost, out = edge_cost, [(2, edge_class, 0, b.edge[edge_class][0]) for b in blocks]
    else:
        cost, out = band_cost, [b.band_rec for b in blocks]
        assert all(abs(o) <= 1 for r in out for o in r[3]) or mut == "band_first"
    nothing = rate(head + fb[type_ctx ^ 0], lam)
    if census is not None:  # (edge against band only where the winner goes on to beat "nothing": otherwise either comparison ends at "none")
        census["tie", "edge==band"] += edge_cost == band_cost and cost < nothing
        census["tie", "cost==nothing"] += cost == nothing
    if (cost > nothing) if mut == "nothing_gt" else (cost >= nothing):
        cost, out = nothing, [NONE] * len(blocks)
    if census is not None:
        census["type", group, ("none", "band", "eo%d" % out[0][1])[out[0][0]]] += 1
        if out[0][0] == 1:
            for r in out:
                census["band_pos", group, "0" if r[2] == 0 else ("27" if r[2] == 27 else "between")] += 1
    costs = [cost, 0, 0]
    for i, cand in ((1, left), (2, top)):
        if cand is None:
            continue
        bits = fb[merge_ctx ^ 1] if i == 1 else fb[merge_ctx ^ 0] + fb[merge_ctx ^ 1]  # left: one bin (1); up: two bins (0, 1)
        if (i == 2 and mut == "up_one_bin"):
            bits = fb[merge_ctx ^ 1]
        if (i == 1 and mut == "left_two_bins"):
            bits = fb[merge_ctx ^ 0] + fb[merge_ctx ^ 1]
        costs[i] = rate(bits, lam) + sum(b.dd(r) for b, r in zip(blocks, cand))
    return out, costs


def code_bin(state, bin_):
    return NEXT_LPS[state] if bin_ != (state & 1) else NEXT_MPS[state]


def decide(w, h, blocks, qp, slice_type, no_wpp, fbits, mutation=None, census=None):
    """-> (records [lcu][3], merge flags [lcu]: 0 none / 1 left / 2 up)"""
    wl, hl = (w + 63) // 64, (h + 63) // 64
    fb = [float(np.float32(v)) for v in fbits]
    lam = lambda_of(qp)
    start = (ctx_state(INIT_MERGE, qp), ctx_state(INIT_TYPE[slice_type], qp))
    ctx = next_row = start
    recs, merge = [], []
    for ly in range(hl):
        if not no_wpp:
            ctx = start if ly == 0 else next_row
            if census is not None and ly > 0:
                census[("wpp_one_wide",) if wl == 1 else ("handoff",)] += 1
        elif census is not None and ly > 0:
            census["no_wpp",] += 1
        for lx in range(wl):
            i = ly * wl + lx
            top, left = (recs[i - wl] if ly else None), (recs[i - 1] if lx else None)
            luma, cost_l = best_mode(blocks[i][:1], ctx, lam, fb, top and top[:1], left and left[:1], mutation, census, "Y")
            if mutation == "uv_separate":
                parts = [best_mode(blocks[i][c:c + 1], ctx, lam, fb, top and top[c:c + 1], left and left[c:c + 1], mutation) for c in (1, 2)]
                chroma, cost_c = parts[0][0] + parts[1][0], [a + b for a, b in zip(parts[0][1], parts[1][1])]
            else:
                chroma, cost_c = best_mode(blocks[i][1:], ctx, lam, fb, top and top[1:], left and left[1:], mutation, census, "C")
            if census is not None:
                for c, name in ((1, "U"), (2, "V")):
                    alone, _ = best_mode(blocks[i][c:c + 1], ctx, lam, fb, top and top[c:c + 1], left and left[c:c + 1], mutation)
                    census["pair_differs", name] += alone[0][:2] != chroma[0][:2]
            own, c_left, c_up = (a + b for a, b in zip(cost_l, cost_c))
            m = 0
            if top is not None and ((c_up < own) if mutation == "up_lt" else (c_up <= own)):
                m = 2
            if left is not None and c_left <= own and (m != 2 or ((c_left <= c_up) if mutation == "left_le_up" else (c_left < c_up))):
                m = 1
            if census is not None and top is not None and left is not None:
                census["merge", ("no", "left", "up")[m]] += 1
                census["tie", "up==own"] += c_up == own
                census["tie", "left==own"] += c_left == own
                census["tie", "left==up"] += c_left == c_up and c_up <= own
            if census is not None and m:
                from_ = recs[i - 1] if m == 1 else recs[i - wl]
                for g, r in (("Y", from_[0]), ("C", from_[1])):
                    census["merge_from", g, ("none", "band", "edge")[r[0]]] += 1
                census["merge_of_merged",] += merge[i - 1 if m == 1 else i - wl] != 0
                census["band_by_merge",] += any(r[0] == 1 for r in from_)
            recs.append(list(top) if m == 2 else (list(left) if m == 1 else luma + chroma))
            merge.append(m)
            merge_ctx, type_ctx = ctx
            if lx > 0:
                merge_ctx = code_bin(merge_ctx, m == 1)
            if ly > 0 and m != 1:
                merge_ctx = code_bin(merge_ctx, m == 2)
            if not m:
                type_ctx = code_bin(type_ctx, recs[i][0][0] != 0)
                if mutation != "type_once":
                    type_ctx = code_bin(type_ctx, recs[i][1][0] != 0)
            ctx = (merge_ctx, type_ctx)
            if lx == (0 if mutation == "handoff_first" else 1):
                next_row = ctx
    return recs, merge


def apply(w, h, picture, recs, mutation=None, census=None):
    """H.265 8.7.3 on a whole picture (the deblocked one): records [lcu][3] -> the filtered picture"""
    wl, hl = (w + 63) // 64, (h + 63) // 64
    planes = planes_of(w, h, np.asarray(picture))
    out = [p.astype(np.int64) for p in planes]
    for c in range(3):
        n, fw, fh = (32 if c else 64), w >> (c > 0), h >> (c > 0)
        full = planes[c].astype(np.int64)
        padded = np.pad(full, 1, mode="edge") if mutation == "filter_border" else np.pad(full, 1, constant_values=-1)
        for i in range(wl * hl):
            rec = recs[i][c]
            if rec[0] == 0:
                continue
            x0, y0 = (i % wl) * n, (i // wl) * n
            x1, y1 = min(x0 + n, fw), min(y0 + n, fh)
            cur = full[y0:y1, x0:x1]
            if rec[0] == 1:
                off = offsets_of(rec, None, cur >> 3, bands=3 if mutation == "band_three" else 4)
            else:
                cls = {2: 3, 3: 2}.get(rec[1], rec[1]) if mutation == "swap_23" else rec[1]
                (ax, ay), (bx, by) = EO_POS[cls]
                a, b = padded[y0 + 1 + ay:y1 + 1 + ay, x0 + 1 + ax:x1 + 1 + ax], padded[y0 + 1 + by:y1 + 1 + by, x0 + 1 + bx:x1 + 1 + bx]
                inside = (a >= 0) & (b >= 0)
                cat = np.where(inside, CATEGORY[2 + np.sign(cur - a) + np.sign(cur - b)], 0)
                off = offsets_of(rec, cat, None)
                if census is not None:
                    if ax:
                        census["kept", "left", rec[1]] += (y1 - y0) * (x0 == 0)
                        census["kept", "right", rec[1]] += (y1 - y0) * (x1 == fw)
                    if ay:
                        census["kept", "top", rec[1]] += (x1 - x0) * (y0 == 0)
                        census["kept", "bottom", rec[1]] += (x1 - x0) * (y1 == fh)
            moved = cur + off
            if census is not None:
                census["filter_clip", "0"] += int((moved < 0).sum())
                census["filter_clip", "255"] += int((moved > 255).sum())
            out[c][y0:y1, x0:x1] = (moved & 255) if mutation == "filter_noclip" else np.clip(moved, 0, 255)
    return np.concatenate([p.reshape(-1) for p in out]).astype(np.uint8)
