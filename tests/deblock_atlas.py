"""The inputs of the deblocking path tests, deterministic from fixed seeds and shared by tests/test_deblock_paths.py (CPU: census, mutations, oracle against the
Python reference) and tests/test_gpu_deblock_paths.py (device against oracle) -- so that the census asserted on the CPU is the census of what the GPU runs.

Pictures are built from 8x8 blocks (base levels at both ends of the sample range and in between, gentle ramps, steps to a neighbour from a wide set, +-1 noise,
outlier lines on rows / columns 1, 2 mod 4 that meet the per-line decisions after lines 0 and 3 decided the part) plus directed parts that clip samples at
0 and 255.  Inter records add constructed neighbour pairs that enumerate the boundary-strength rule on both edge directions."""
import functools

import numpy as np

import deblock_common as dc
from test_deblock_inter import CuDbk, PART_SIZES, random_inter_picture

GEOMETRIES = [(64, 64), (72, 72), (136, 72)]
PICTURES = 4  # per geometry
CORNERS = [(6, 6), (-6, -6), (6, -6), (-6, 6)]
# steps between neighbouring blocks: small ones (strong filter), the values around (5 tc + 1) >> 1 for odd tc, medium ones (weak filter, delta clipped), large ones (cut / off)
STEPS = [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 13, 15, 17, 18, 20, 22, 23, 25, 27, 28, 30, 32, 33, 36, 40, 45, 50, 56, 60, 64, 72, 80, 96, 110, 120]


def _base_level(rng):
    k = rng.integers(0, 4)
    if k == 0:
        return int(rng.integers(0, 5))
    if k == 1:
        return int(rng.integers(251, 256))
    if k == 2:
        return 128 + int(rng.integers(-3, 4))
    return int(rng.integers(0, 256))


def _blocky_plane(w, h, rng, fresh=0.12, noisy=0.3, outliers=0.3, wild=0.05):
    """a plane of 8x8 blocks as the module docstring describes; int array, clipped to 0 .. 255"""
    hb, wb = (h + 7) // 8, (w + 7) // 8
    level = np.zeros((hb, wb), np.int64)
    plane = np.zeros((hb * 8, wb * 8), np.int64)
    yy, xx = np.mgrid[0:8, 0:8]
    for by in range(hb):
        for bx in range(wb):
            if (bx == 0 and by == 0) or rng.random() < fresh:
                base = _base_level(rng)
            else:
                left = bx > 0 and (by == 0 or rng.random() < 0.5)
                near = level[by, bx - 1] if left else level[by - 1, bx]
                step = STEPS[int(rng.integers(0, len(STEPS)))] * (1 if rng.random() < 0.5 else -1)
                base = near + step if 0 <= near + step <= 255 else near - step
                base = int(np.clip(base, 0, 255))
            level[by, bx] = base
            blk = np.full((8, 8), base, np.int64)
            if rng.random() < 0.4:  # a gentle ramp: at most one level per two samples
                gx, gy = int(rng.integers(-1, 2)), int(rng.integers(-1, 2))
                blk += (gx * xx + gy * yy) // int(rng.integers(2, 5))
            if rng.random() < noisy:
                blk += rng.integers(-1, 2, (8, 8))
            if rng.random() < wild:
                blk = rng.integers(0, 256, (8, 8))
            if rng.random() < outliers:  # lines 1 / 2 mod 4 moved on this side of the block's edges
                lines = [int(v) for v in rng.choice([1, 2, 5, 6], int(rng.integers(1, 4)), replace=False)]
                shift = int(rng.integers(30, 201)) * (1 if base < 128 else -1)
                if rng.random() < 0.5:
                    blk[lines, :] += shift  # rows: met by the vertical edges
                else:
                    blk[:, lines] += shift  # columns: met by the horizontal edges
            plane[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = blk
    return np.clip(plane[:h, :w], 0, 255)


def _directed_luma(Y, x, y, vertical, part):
    """the part of the edge at (x, y) (first q sample; `part` 0 / 1 along the edge) whose lines 0 and 3 choose the weak filter and whose lines 1 and 2 clip
    a sample at 0 and at 255 from tc = 5 on"""
    profile = [[0, 0, 0, 0, 60, 60, 60, 60], [0, 0, 0, 0, 0, 255, 255, 255], [255, 255, 255, 255, 255, 0, 0, 0], [0, 0, 0, 0, 60, 60, 60, 60]]
    for i in range(4):
        for k in range(8):
            if vertical:
                Y[y + 4 * part + i, x - 4 + k] = profile[i][k]
            else:
                Y[y - 4 + k, x + 4 * part + i] = profile[i][k]


def _directed_chroma(P, xc, yc, vertical):
    """lines 1 and 2 of the chroma part at (xc, yc): delta clipped to +-tc_c and a sample pushed below 0 / above 255"""
    profile = {1: [200, 1, 1, 0], 2: [55, 254, 254, 255]}
    for i, line in profile.items():
        for k in range(4):
            if vertical:
                P[yc + i, xc - 2 + k] = line[k]
            else:
                P[yc - 2 + k, xc + i] = line[k]


@functools.lru_cache(maxsize=None)
def pictures(w, h):
    """[(frame: planar 4:2:0 uint8, cu_depth: [h/8][w/8] uint8)] of one geometry; depth maps: random quadtrees, all depth 3, all depth 0"""
    out = []
    assert PICTURES == 4  # the positions of the directed parts below are listed per picture
    for i in range(PICTURES):
        rng = np.random.default_rng(1000 * w + 10 * h + i)
        Y = _blocky_plane(w, h, rng)
        C = [_blocky_plane(w // 2, h // 2, rng, fresh=0.3, noisy=0.3, outliers=0.15, wild=0.15) for _ in range(2)]
        # directed parts on the edges at 32, which every depth map filters (a 64x64 CU's transform units are 32x32)
        for part in range(2):
            _directed_luma(Y, 32, (8, 24, 40, 16)[i], True, part)
            _directed_luma(Y, (16, 40, 16, 40)[i], 32, False, part)
        for P in C:
            _directed_chroma(P, 16, (4, 20, 24, 28)[i], True)
            _directed_chroma(P, (20, 24, 28, 4)[i], 16, False)
        frame = np.concatenate([Y.reshape(-1), C[0].reshape(-1), C[1].reshape(-1)]).astype(np.uint8)
        if i == PICTURES - 2:
            depth = np.full((h // 8, w // 8), 3, np.uint8)
        elif i == PICTURES - 1:
            depth = np.zeros((h // 8, w // 8), np.uint8)
        else:
            depth = dc.random_depth_map(w, h, rng)
        frame.setflags(write=False)
        depth.setflags(write=False)
        out.append((frame, depth))
    return out


# ---- records of inter pictures ------------------------------------------------------------------------------------------------------------------------------
REF_LX = [[0, 1, 2], [0, 3, 1]]  # (list, index) -> picture: picture 0 is L0[0] and L1[0], picture 1 is L0[1] and L1[2]


def records_from_depth(w, h, depth):
    """all-intra records of a CU depth map: what the inter entry points must filter exactly like kvz_hip_dev_deblock_frames filters the map"""
    info = (CuDbk * ((w // 4) * (h // 4)))()
    for y4 in range(h // 4):
        for x4 in range(w // 4):
            d = int(depth[y4 // 2, x4 // 2])
            r = info[y4 * (w // 4) + x4]
            r.type, r.depth, r.tr_depth, r.part_size, r.cbf_y = 1, d, max(d, 1), 0, 1
    return info


def _motion(mv_dir, mv0=(0, 0), mv1=(0, 0), ref0=0, ref1=0, cbf=0, intra=False):
    return dict(mv_dir=mv_dir, mv=(mv0, mv1), mref=(ref0, ref1), cbf=cbf, intra=intra)


def _pairs(slice_b):
    """(p side, q side) motion of neighbouring prediction units, one pair per outcome of the boundary-strength rule"""
    A, B = (8, -12), (-20, 5)
    out = []
    for d in (3, 4, -3, -4):  # exactly 3 and exactly 4 quarter samples, in x and in y
        out.append((_motion(1, A), _motion(1, (A[0] + d, A[1]))))
        out.append((_motion(1, A), _motion(1, (A[0], A[1] + d))))
    out.append((_motion(1, A), _motion(1, A)))
    out.append((_motion(1, A, ref0=0), _motion(1, A, ref0=1)))          # equal vectors, another reference
    out.append((_motion(1, A, cbf=1), _motion(1, A)))                   # coded coefficients on either side
    out.append((_motion(1, A), _motion(1, A, cbf=1)))
    out.append((_motion(1, A, intra=True), _motion(1, A)))              # an intra CU on either side
    out.append((_motion(1, A), _motion(1, A, intra=True)))
    if not slice_b:
        return out
    out.append((_motion(1, A), _motion(3, A, B, 0, 1)))                 # uni against bi
    out.append((_motion(3, A, B, 0, 1), _motion(2, A, B, 0, 1)))
    for d in (0, 3, 4, -4):                                             # L0 only against L1 only, the same picture: crossed
        out.append((_motion(1, A, ref0=0), _motion(2, (0, 0), (A[0] + d, A[1]), 0, 0)))
        out.append((_motion(2, (0, 0), A, 0, 0), _motion(1, (A[0], A[1] - d), ref0=0)))
    for d in (0, 3, 4, -4):
        out.append((_motion(3, A, B, 0, 1), _motion(3, (A[0] + d, A[1]), B, 0, 1)))                  # bi against bi, lists straight
        out.append((_motion(3, A, B, 0, 1), _motion(3, A, (B[0], B[1] + d), 0, 1)))
        out.append((_motion(3, A, B, 0, 2), _motion(3, (B[0], B[1] + d), A, 1, 0)))                  # lists crossed: pictures (0, 1) against (1, 0)
        out.append((_motion(3, A, B, 0, 2), _motion(3, B, (A[0] - d, A[1]), 1, 0)))
    far = (A[0] + 8, A[1])
    out.append((_motion(3, A, A, 0, 0), _motion(3, A, A, 0, 0)))        # one picture twice: neither straight nor crossed apart
    out.append((_motion(3, A, far, 0, 0), _motion(3, A, far, 0, 0)))    # crossed apart only
    out.append((_motion(3, A, far, 0, 0), _motion(3, far, A, 0, 0)))    # straight apart only
    out.append((_motion(3, A, A, 0, 0), _motion(3, far, far, 0, 0)))    # both: the only one that filters
    out.append((_motion(3, A, B, 0, 0), _motion(3, (A[0] + 4, A[1]), (B[0], B[1] - 4), 0, 0)))
    return out


def _fill(info, w, h, x, y, bw, bh, depth, tr_depth, part_size, m):
    for uy in range(y, min(h, y + bh), 4):
        for ux in range(x, min(w, x + bw), 4):
            r = info[(uy // 4) * (w // 4) + ux // 4]
            r.type, r.depth, r.tr_depth, r.part_size, r.cbf_y = (1 if m["intra"] else 2), depth, tr_depth, part_size, m["cbf"]
            if not m["intra"]:
                r.mv_dir = m["mv_dir"]
                for l in range(2):
                    r.mv_ref[l], r.ref_id[l] = m["mref"][l], REF_LX[l][m["mref"][l]]
                    r.mv[l][0], r.mv[l][1] = m["mv"][l]


def paired_records(w, h, slice_b, vertical, shift):
    """8x8 CUs (every edge of the 8x8 grid a transform edge); columns (vertical) or rows alternate between the p and the q side of the pairs, which cycle"""
    info = (CuDbk * ((w // 4) * (h // 4)))()
    pairs = _pairs(slice_b)
    k = shift
    for a in range(0, (h if vertical else w), 8):          # along the edges
        for b in range(0, (w if vertical else h), 16):     # across them: p at b, q at b + 8
            p, q = pairs[k % len(pairs)]
            k += 1
            for side, m in ((0, p), (8, q)):
                x, y = (b + side, a) if vertical else (a, b + side)
                if x < w and y < h:
                    _fill(info, w, h, x, y, 8, 8, 3, 3, 0, m)
    return info


def partitioned_records(w, h, slice_b, seed):
    """CUs of 64, 32 and 16 samples with every part_size whose second partition starts on the 8x8 grid, transform units as large as the CU allows: prediction
    edges that are no transform edges.  Both partitions carry coded coefficients; their motion is equal (strength 0 on a prediction edge: the coefficients do
    not count there) or a sample apart."""
    rng = np.random.default_rng(seed)
    info = (CuDbk * ((w // 4) * (h // 4)))()
    A = (8, -12)
    for cy in range(0, h, 64):
        for cx in range(0, w, 64):
            size = (64, 32, 16)[((cx + cy) // 64 + seed) % 3]
            for y in range(cy, min(h, cy + 64), size):
                for x in range(cx, min(w, cx + 64), size):
                    depth = {64: 0, 32: 1, 16: 2}[size]
                    ps = int(rng.choice([1, 2, 3] if size == 16 else [1, 2, 4, 5, 6, 7]))
                    apart = rng.random() < 0.5
                    for n, (ox, oy, pw, ph) in enumerate(PART_SIZES[ps]):
                        mv = (A[0] + (4 * n if apart else 3 * (n & 1)), A[1])
                        m = _motion(3, mv, mv, 0, 0, cbf=1) if slice_b and rng.random() < 0.3 else _motion(1, mv, cbf=1)
                        _fill(info, w, h, x + ox * size // 4, y + oy * size // 4, pw * size // 4, ph * size // 4, depth, max(depth, 1), ps, m)
    return info


@functools.lru_cache(maxsize=None)
def inter_records(w, h, slice_b):
    """record sets of one geometry and slice type: constructed pairs on vertical and on horizontal edges, partitioned CUs, random pictures"""
    rng = np.random.default_rng(77 + w + h + slice_b)
    return [paired_records(w, h, slice_b, True, 0), paired_records(w, h, slice_b, False, 5), partitioned_records(w, h, slice_b, 1),
            random_inter_picture(w, h, rng, slice_b), paired_records(w, h, slice_b, True, 17), paired_records(w, h, slice_b, False, 23),
            partitioned_records(w, h, slice_b, 2), random_inter_picture(w, h, rng, slice_b)]


def launch_of_52(w, h, kind):
    """GPU test (b): picture i at QP i, content cycling.  kind: "intra" (records from the depth maps), "P", "B".  -> (frames, records, depths or None)"""
    pics = pictures(w, h)
    frames = [pics[i % len(pics)][0] for i in range(52)]
    if kind == "intra":
        sets = [records_from_depth(w, h, d) for _, d in pics]
        return frames, [sets[i % len(pics)] for i in range(52)], [pics[i % len(pics)][1] for i in range(52)]
    sets = inter_records(w, h, 1 if kind == "B" else 0)
    return frames, [sets[i % len(sets)] for i in range(52)], None
