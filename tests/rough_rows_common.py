"""What tests/test_satd_rows_table.py (host) and tests/test_rough_rows.py (device) share: the reference sets, and the oracle's intra prediction of modes 2..33 for
them -- kvz_intra_predict's choice of the filtered or unfiltered references (intra.c:262-281), intra_filter_reference (intra.c:176-204), the oracle's
kvz_angular_pred (cases.py cases_intra's function) and intra_post_process_angular (intra.c:207-219) -- cut into the 8x8 blocks the rough search scores: computed
once per CU size and left unchanged."""
import numpy as np

import flatapi

PAD = 8  # bytes behind a reference row (cases_intra gives kvz_angular_pred the same room)
_SETS, _WANT = {}, {}


def ref_sets(log2w):
    """(top, left): [count][2 w + 1 + PAD] unfiltered references, the corner shared -- 50 random sets, all 0, all 255, and four that alternate 0 / 255 (in phase and
    out of phase along the two sides, from a 0 and from a 255 corner): next to the corner those take the edge samples of modes 10 / 26 into both ends of their clip"""
    if log2w not in _SETS:
        n = 2 * (1 << log2w) + 1
        rng = np.random.default_rng(1000 + log2w)
        top = rng.integers(0, 256, (50, n), dtype=np.uint8)
        left = rng.integers(0, 256, (50, n), dtype=np.uint8)
        alt = (255 * (np.arange(n) & 1)).astype(np.uint8)
        out_of_phase = 255 - alt
        out_of_phase[0] = alt[0]
        special_top = [np.zeros(n, np.uint8), np.full(n, 255, np.uint8), alt, 255 - alt, alt, 255 - alt]
        special_left = [np.zeros(n, np.uint8), np.full(n, 255, np.uint8), alt, 255 - alt, out_of_phase, 255 - out_of_phase]
        top = np.concatenate([top, np.array(special_top)])
        left = np.concatenate([left, np.array(special_left)])
        left[:, 0] = top[:, 0]
        pad = np.zeros((len(top), PAD), np.uint8)
        _SETS[log2w] = (np.ascontiguousarray(np.hstack([top, pad])), np.ascontiguousarray(np.hstack([left, pad])))
    return _SETS[log2w]


def reads_filtered(log2w, mode):
    return min(abs(mode - 26), abs(mode - 10)) > {3: 7, 4: 1}[log2w]


def filtered(top, left, n):
    """intra.c:176-204 on one reference set"""
    t, l = top[:n].astype(np.int32), left[:n].astype(np.int32)
    ft, fl = t.copy(), l.copy()
    ft[1:n - 1] = (t[:n - 2] + 2 * t[1:n - 1] + t[2:n] + 2) // 4
    fl[1:n - 1] = (l[:n - 2] + 2 * l[1:n - 1] + l[2:n] + 2) // 4
    ft[0] = fl[0] = (l[1] + 2 * l[0] + t[1] + 2) // 4
    pad = np.zeros(PAD, np.uint8)
    return np.concatenate([ft.astype(np.uint8), pad]), np.concatenate([fl.astype(np.uint8), pad])


def oracle_blocks(oracle, log2w):
    """[count][32 modes][(w / 8)^2 blocks, raster][64]: the layout of kvz_hip_dev_rough_rows' output"""
    if log2w not in _WANT:
        w, n = 1 << log2w, 2 * (1 << log2w) + 1
        tops, lefts = ref_sets(log2w)
        nb = w // 8
        want = np.empty((len(tops), 32, nb * nb, 64), np.uint8)
        dst = np.zeros(w * w, np.uint8)
        for i in range(len(tops)):
            ft, fl = filtered(tops[i], lefts[i], n)
            for mode in range(2, 34):
                t, l = (ft, fl) if reads_filtered(log2w, mode) else (tops[i], lefts[i])
                oracle.angular_pred(log2w, mode, flatapi.ptr(t), flatapi.ptr(l), flatapi.ptr(dst))
                pred = dst.reshape(w, w).astype(np.int32)
                if mode == 10:
                    pred[0, :] = np.clip(pred[0, :] + ((t[1:w + 1].astype(np.int32) - int(t[0])) >> 1), 0, 255)
                if mode == 26:
                    pred[:, 0] = np.clip(pred[:, 0] + ((l[1:w + 1].astype(np.int32) - int(l[0])) >> 1), 0, 255)
                want[i, mode - 2] = pred.astype(np.uint8).reshape(nb, 8, nb, 8).transpose(0, 2, 1, 3).reshape(nb * nb, 64)
        want.setflags(write=False)
        _WANT[log2w] = want
    return _WANT[log2w]
