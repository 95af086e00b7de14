"""The inputs of the SAO path tests, deterministic from fixed seeds and shared by tests/test_sao_paths.py (CPU: the Python statement against the oracle and the host
simulation, census, mutations) and tests/test_gpu_sao_paths.py (device against oracle) -- so that the census asserted on the CPU is the census of what the GPU runs.

A picture is a (source, reconstruction) pair of planar 4:2:0 frames plus a CU depth map (the edges deblocking filters when it is on).  The reconstruction is built
LCU by LCU and plane by plane from one of the KINDS below, the source is the reconstruction plus a constructed error; an LCU may instead be a byte copy of its left
or upper neighbour of the same size (merge wins, equal merge costs)."""
import functools

import numpy as np

import deblock_common as dc
from deblock_atlas import records_from_depth  # noqa: F401  (what the inter entry points take for a depth map)

# the smallest sizes at which each mechanism can still fail (see tests/test_sao_paths.py): one LCU; 8-wide last column and row (chroma 4x4 with a 2x2 interior);
# a third LCU after the WPP hand-off; one LCU wide and three high; the three row-tail lengths of the filter kernel (chroma 36, 68: one dword, 40: two, 44: three)
GEOMETRIES = [(64, 64), (72, 72), (136, 72), (64, 136), (88, 72), (80, 64)]
PICTURES = 6  # per geometry
KINDS = ["band", "band0", "band27", "eo0", "eo1", "eo2", "eo3", "noise", "big", "flatbig", "wrong", "exact", "sat", "tie"]
LAUNCH = 104  # pictures of a GPU launch: picture i runs at QP i % 52 (more than 64: the chain kernel's second workgroup)


def launch_content(n, slice_b=0, no_wpp=0):
    """which atlas picture each of the n pictures of a launch of tests/test_gpu_sao_paths.py holds.  52 = 4 mod 6, so pictures i and i + 52 differ, and the four
    (slice type, WPP) launches of a geometry bring pictures q and q + 4, q + 1 and q + 5, q + 3 and q + 1, q + 4 and q + 2 to QP q: all six"""
    return [(i + 3 * no_wpp + slice_b) % PICTURES for i in range(n)]


def launch_cases():
    """every (slice_is_b, deblock, no_wpp, [(picture, QP)]) that test_every_qp_in_one_launch runs per geometry: what the census of tests/test_sao_paths.py counts"""
    return [(slice_b, deblock, no_wpp, list(zip(launch_content(LAUNCH, slice_b, no_wpp), [i % 52 for i in range(LAUNCH)])))
            for slice_b in (0, 1) for deblock in (0, 1) for no_wpp in (0, 1)]


def _ramp(bh, bw, rng, lo=None, span=None):
    yy, xx = np.mgrid[0:bh, 0:bw]
    lo = int(rng.integers(30, 180)) if lo is None else lo
    span = int(rng.integers(8, 48)) if span is None else span
    gx, gy = int(rng.integers(1, 4)), int(rng.integers(0, 3))
    t = gx * xx + gy * yy
    return lo + t * span // max(int(t.max()), 1)


def _pattern(k, bh, bw):
    """1 where a sample sticks out of both its neighbours along the direction of edge class k and of no other diagonal"""
    yy, xx = np.mgrid[0:bh, 0:bw]
    if k == 0:
        return xx & 1
    if k == 1:
        return yy & 1
    return (((xx + yy) if k == 2 else (xx - yy)) & 3) >> 1


def _block(kind, bh, bw, rng):
    """-> (source, reconstruction) of one plane of one LCU, int arrays not yet clipped"""
    if kind.startswith("band"):
        pos = {"band0": 0, "band27": 27}.get(kind, int(rng.integers(1, 27)))
        rec = _ramp(bh, bw, rng, lo=max(8 * pos - 12, 0), span=min(52, 255 - max(8 * pos - 12, 0)))
        bias = int(rng.choice([-2, -1, 1, 2, 3]))
        if pos == 0:
            bias = abs(bias)
        inside = (rec >> 3 >= pos) & (rec >> 3 < pos + 4)
        return rec + bias * inside, rec
    if kind.startswith("eo"):
        base = _ramp(bh, bw, rng)
        d = int(rng.integers(2, 7)) * (1 if rng.random() < 0.5 else -1)
        return base + rng.integers(0, 2, (bh, bw)) * (rng.random() < 0.3), base + d * _pattern(int(kind[2]), bh, bw)
    if kind == "noise":
        src = _ramp(bh, bw, rng) + rng.integers(-2, 3, (bh, bw))
        return src, src + rng.integers(-1, 2, (bh, bw))
    if kind == "big":  # extrema 40 .. 200 levels off: offsets clipped at +-7, large sums of either sign
        base = _ramp(bh, bw, rng, lo=int(rng.integers(100, 150)), span=10)
        d = int(rng.integers(40, 100)) * (1 if rng.random() < 0.5 else -1)
        return base, base + d * _pattern(int(rng.integers(0, 4)), bh, bw) + rng.integers(0, 2, (bh, bw))
    if kind == "flatbig":  # the whole block far off: |sum| up to 4096 x 200 in one band accumulator
        a, b = int(rng.integers(0, 40)), int(rng.integers(215, 256))
        src, rec = (a, b) if rng.random() < 0.5 else (b, a)
        return np.full((bh, bw), src), np.full((bh, bw), rec) + rng.integers(0, 3, (bh, bw))
    if kind == "wrong":  # extrema that would have to be sharpened: the natural offset has the sign that cannot be coded
        base = _ramp(bh, bw, rng)
        d = int(rng.integers(2, 6)) * (1 if rng.random() < 0.5 else -1)
        p = _pattern(int(rng.integers(0, 4)), bh, bw)
        return base + 2 * d * p, base + d * p
    if kind == "exact":
        src = _ramp(bh, bw, rng) + rng.integers(-2, 3, (bh, bw))
        return src, src
    if kind == "sat":  # offsets applied to samples within 7 of 0 / 255
        p = _pattern(int(rng.integers(0, 4)), bh, bw)
        if rng.random() < 0.5:
            return np.zeros((bh, bw), np.int64) + rng.integers(0, 2, (bh, bw)), rng.integers(0, 4, (bh, bw)) + 4 * p
        return np.full((bh, bw), 255) - rng.integers(0, 2, (bh, bw)), 255 - rng.integers(0, 4, (bh, bw)) - 4 * p
    if kind == "tie":
        # Edge and band SAO catch the same samples at the same offset: valleys (or peaks) one band away from a flat block, only in its interior, so that category 1
        # (4) of class 0 and one band hold exactly them.  k more samples of that band in the first and last row, which the edge statistics leave out, give band a
        # lead of k in distortion; band's mode costs 4 bits more, so wherever round(4 lambda) = k the two costs are equal -- and far below the cost of nothing.
        yy, xx = np.mgrid[0:bh, 0:bw]
        inner = ((xx & 1) == 1) & (yy > 0) & (yy < bh - 1) & (xx < bw - 1)
        level, err = (92, 1) if rng.random() < 0.6 else (108, -2)
        rec = np.where(inner, level, 100)
        k = min(int(rng.choice([0, 1, 1, 2, 2, 3, 3, 4, 5, 6, 9, 14, 20, 28, 40, 57, 80])), 2 * bw)
        rec[0, :min(k, bw)] = level
        rec[bh - 1, :max(k - bw, 0)] = level
        return rec + err * (rec == level), rec
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def pictures(w, h):
    """[(source, reconstruction, cu_depth)] of one geometry: frames planar 4:2:0 uint8, read-only; cu_depth [h/8][w/8]"""
    wl, hl = (w + 63) // 64, (h + 63) // 64
    out = []
    for i in range(PICTURES):
        rng = np.random.default_rng(7000 * w + 70 * h + i)
        src = [np.zeros((h >> (c > 0), w >> (c > 0)), np.int64) for c in range(3)]
        rec = [p.copy() for p in src]
        for ly in range(hl):
            for lx in range(wl):
                joint = KINDS[int(rng.integers(0, len(KINDS)))]  # the chroma planes share a kind two times out of three
                copy = rng.random() < 0.3
                for c in range(3):
                    n = 32 if c else 64
                    x0, y0 = lx * n, ly * n
                    x1, y1 = min(x0 + n, w >> (c > 0)), min(y0 + n, h >> (c > 0))
                    kind = KINDS[int(rng.integers(0, len(KINDS)))] if (c == 0 or rng.random() < 0.33) else joint
                    if i == 3 and c == 0 and rng.random() < 0.7:  # a picture of luma blocks where edge and band SAO cost the same at some QP
                        kind = "tie"
                    if i % 3 == 1 and rng.random() < 0.75:  # calm pictures: LCUs without an error next to each other, where all the costs of a decision meet
                        kind = "exact"
                    s, r = _block(kind, y1 - y0, x1 - x0, rng)
                    if i % 3 == 2 and kind not in ("sat", "flatbig", "exact", "tie"):  # steps on the 8x8 grid: what deblocking smooths, so that R, V and D differ
                        by, bx = np.mgrid[0:y1 - y0, 0:x1 - x0]
                        r = r + rng.integers(-3, 4, (8, 8))[(by >> 3) & 7, (bx >> 3) & 7]
                    src[c][y0:y1, x0:x1], rec[c][y0:y1, x0:x1] = s, r
                if copy:  # a byte copy of a neighbour of the same size, all three planes
                    left_ok, up_ok = lx > 0 and min(w - lx * 64, 64) == 64, ly > 0 and min(h - ly * 64, 64) == 64
                    from_left = left_ok and (not up_ok or rng.random() < 0.5)
                    if left_ok or up_ok:
                        for c in range(3):
                            n = 32 if c else 64
                            x0, y0 = lx * n, ly * n
                            x1, y1 = min(x0 + n, w >> (c > 0)), min(y0 + n, h >> (c > 0))
                            dx, dy = (n, 0) if from_left else (0, n)
                            for p in (src[c], rec[c]):
                                p[y0:y1, x0:x1] = p[y0 - dy:y1 - dy, x0 - dx:x1 - dx]
        frames = [np.concatenate([np.clip(p, 0, 255).reshape(-1) for p in planes]).astype(np.uint8) for planes in (src, rec)]
        depth = np.full((h // 8, w // 8), 3, np.uint8) if i % 2 == 0 else dc.random_depth_map(w, h, rng)
        for a in frames + [depth]:
            a.setflags(write=False)
        out.append((frames[0], frames[1], depth))
    return out
