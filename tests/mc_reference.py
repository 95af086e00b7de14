"""A plain model of HEVC 4:2:0 motion-compensated interpolation with the semantics of kvazaar's generic strategies (ipol-generic.c:134-211, 681-758,
picture-generic.c:553-668), in int64 numpy: the checker the interpolation kernels are compared with, itself pinned against the oracle and the compiled
reference by tests/test_mc_reference.py.  TEST INFRASTRUCTURE -- never imported by the product.

  * the window around the block is edge-clamped (get_extended_block, ipol-generic.c:761-814);
  * the horizontal pass is stored as int16 (the reference's intermediate buffer);
  * the vertical sum is kept whole and shifted >> 6: the 14-bit sample v;
  * one list: clip((v + 32) >> 6), v NOT narrowed (kvz_sample_quarterpel_luma_generic clips the int32);
  * two lists: each operand int16(v) (wrapped, as kvz_sample_quarterpel_luma_hi_generic stores it), then clip((a + b + 64) >> 7).

The only phase where v leaves int16 is the luma half-pel position in both directions, mv & 3 == (2, 2): a sign-matched 0 / 255 window drives v to
(88 * 22440 + 24 * 6120) >> 6 = 33150 (extreme_window below)."""
import numpy as np

LUMA_FILTER = np.array([[0, 0, 0, 64, 0, 0, 0, 0], [-1, 4, -10, 58, 17, -5, 1, 0], [-1, 4, -11, 40, 40, -11, 4, -1], [0, 1, -5, 17, 58, -10, 4, -1]], np.int64)  # filter.c:66-72
CHROMA_FILTER = np.array([[0, 64, 0, 0], [-2, 58, 10, -2], [-4, 54, 16, -2], [-6, 46, 28, -4], [-4, 36, 36, -4], [-4, 28, 46, -6], [-2, 16, 54, -4],
                          [-2, 10, 58, -2]], np.int64)  # filter.c:74-84


def filters(fx, fy, chroma):
    """(horizontal taps, vertical taps) of fractional phase (fx, fy): quarter-pel luma, eighth-pel chroma"""
    f = CHROMA_FILTER if chroma else LUMA_FILTER
    return f[fx], f[fy]


def clamped(plane, x0, y0, w, h):
    """the w x h window of a 2-D plane at (x0, y0), edge samples repeated outside the plane"""
    fh, fw = plane.shape
    return plane[np.ix_(np.clip(np.arange(y0, y0 + h), 0, fh - 1), np.clip(np.arange(x0, x0 + w), 0, fw - 1))]


def filter14(plane, x, y, w, h, mv, chroma):
    """the 14-bit samples v (int64, not narrowed) of the w x h block at (x, y) of a 2-D plane under motion vector mv (quarter luma samples;
    chroma planes take it as eighth chroma samples)"""
    taps, before, frac, ish = (4, 1, 7, 3) if chroma else (8, 3, 3, 2)
    hf, vf = filters(mv[0] & frac, mv[1] & frac, chroma)
    win = clamped(plane, x + (mv[0] >> ish) - before, y + (mv[1] >> ish) - before, w + taps - 1, h + taps - 1).astype(np.int64)
    g = sum(hf[k] * win[:, k:k + w] for k in range(taps)).astype(np.int16).astype(np.int64)
    return sum(vf[k] * g[k:k + h, :] for k in range(taps)) >> 6


def uni(v):
    """the finished sample of one list"""
    return np.clip((np.asarray(v, np.int64) + 32) >> 6, 0, 255).astype(np.uint8)


def hi(v):
    """the 14-bit operand of two-list prediction as the reference stores it: wrapped to int16"""
    return np.asarray(v, np.int64).astype(np.int16)


def bi(a, b):
    """kvz_bipred_average of two int16 operands"""
    return np.clip((np.asarray(a, np.int64) + np.asarray(b, np.int64) + 64) >> 7, 0, 255).astype(np.uint8)


def planes_of(frame, W, H):
    """(2-D plane, offset) of Y, U, V in a W x H 4:2:0 frame of bytes"""
    q = W * H // 4
    return ((frame[:W * H].reshape(H, W), 0), (frame[W * H:W * H + q].reshape(H // 2, W // 2), W * H), (frame[W * H + q:W * H + 2 * q].reshape(H // 2, W // 2), W * H + q))


def inter_pred(refs, W, H, pus):
    """the prediction picture of PU list pus = [(x, y, w, h, mv0, mv1, use0, use1)] from the reference frames refs[0], refs[1]"""
    pred = np.zeros(W * H * 3 // 2, np.uint8)
    out = planes_of(pred, W, H)
    for (x, y, w, h, mv0, mv1, u0, u1) in pus:
        for pi in range(3):
            sh = 1 if pi else 0
            vals = [filter14(planes_of(ref, W, H)[pi][0], x >> sh, y >> sh, w >> sh, h >> sh, mv, pi > 0) for use, mv, ref in ((u0, mv0, refs[0]), (u1, mv1, refs[1])) if use]
            out[pi][0][y >> sh:(y + h) >> sh, x >> sh:(x + w) >> sh] = uni(vals[0]) if len(vals) == 1 else bi(hi(vals[0]), hi(vals[1]))
    return pred


def extreme_window(fx, fy, chroma, maximise=True):
    """the taps x taps window of 0 / 255 samples that drives the sample of phase (fx, fy) to its largest (smallest) value: 255 where the product of the
    horizontal and vertical tap is positive (negative)"""
    hf, vf = filters(fx, fy, chroma)
    s = np.sign(vf)[:, None] * np.sign(hf)[None, :]
    return np.where(s > 0 if maximise else s < 0, 255, 0).astype(np.uint8)


def tiled(window, h, w, y0=0, x0=0):
    """an h x w plane of the window repeated, so that the window starts at rows y0 + k taps, columns x0 + k taps"""
    t = window.shape[0]
    return window[np.ix_((np.arange(h) - y0) % t, (np.arange(w) - x0) % t)].copy()


def extreme_sample(fx, fy, chroma, maximise=True):
    """v of phase (fx, fy) on its extreme window, from the taps alone"""
    hf, vf = filters(fx, fy, chroma)
    win = extreme_window(fx, fy, chroma, maximise).astype(np.int64)
    g = (win * hf[None, :]).sum(axis=1)
    return int((vf * g).sum() >> 6)


def extreme_frame(W, H, fx=2, fy=2, cfx=4, cfy=4, maximise=True):
    """a 4:2:0 frame whose luma is the luma (fx, fy) extreme window tiled from the origin, chroma the chroma (cfx, cfy) one"""
    y = tiled(extreme_window(fx, fy, False, maximise), H, W)
    c = tiled(extreme_window(cfx, cfy, True, maximise), H // 2, W // 2)
    return np.concatenate([y.reshape(-1), c.reshape(-1), c.reshape(-1)])
