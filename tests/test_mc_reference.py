"""tests/mc_reference.py -- the int64 model of motion-compensated interpolation the device kernels are checked with -- pinned against the oracle and the
compiled reference (oracle/_ref, generic and AVX2 strategies) where kernels go wrong: every luma (16) and chroma (64) phase, on the sign-matched 0 / 255
windows that drive each phase's sample to its largest and smallest value and on random content, PU sizes 8..64 including 2:1 shapes, windows off every
picture edge.  The one place where the reference disagrees with itself is written down explicitly: at the luma (2, 2) phase the 14-bit operand of
two-list prediction leaves int16, generic wraps it and AVX2 saturates it; the project follows generic."""
import numpy as np
import pytest

import flatapi
import mc_reference as mc
from flatapi import A, ptr

LUMA_SIZES = [(8, 8), (16, 16), (32, 32), (64, 64), (16, 8), (8, 16), (32, 16), (64, 32), (24, 32)]
CHROMA_SIZES = [(4, 4), (8, 8), (16, 16), (32, 32), (8, 4), (4, 8), (16, 8), (32, 16)]
S = 96      # side of the plane the blocks are cut from; the block sits at (ORG, ORG): every window stays inside it
ORG = 16


@pytest.fixture(scope="module", params=["oracle", "ref-generic", "ref-avx2"])
def impl(request):
    """(name, flat library) -- the compiled reference's strategies are process globals: select before every use"""
    import os
    if request.param == "oracle":
        return request.param, flatapi.load_oracle()
    if not os.path.exists(flatapi.refshim_path()):
        pytest.skip("oracle/_ref not built")
    return request.param, flatapi.load_ref(0 if request.param == "ref-generic" else 1)


def _select(name, lib):
    if name.startswith("ref"):
        flatapi.load_ref(0 if name == "ref-generic" else 1)
    return lib


def test_only_the_luma_half_half_phase_leaves_int16():
    """the extremes of every phase from its taps: the largest sample of luma (2, 2) is 33150, every other luma and chroma phase stays within 29580"""
    ext = {}
    for chroma, n in ((False, 4), (True, 8)):
        for fx in range(n):
            for fy in range(n):
                hi_, lo_ = mc.extreme_sample(fx, fy, chroma, True), mc.extreme_sample(fx, fy, chroma, False)
                ext[(chroma, fx, fy)] = (lo_, hi_)
    assert ext[(False, 2, 2)] == (-16830, 33150)
    others = [v for k, v in ext.items() if k != (False, 2, 2)]
    assert max(h for _, h in others) == 29580 and min(l for l, _ in others) >= -16830
    assert ext[(False, 0, 0)] == (0, 255 * 64) and ext[(True, 0, 0)] == (0, 255 * 64)


def _phase_planes(fx, fy, chroma, rng):
    """(label, S x S plane): the phase's maximising and minimising windows tiled so that a window starts at every taps-th sample from the block's first
    window, and random content"""
    taps, before = (4, 1) if chroma else (8, 3)
    out = []
    for maximise in (True, False):
        out.append(("max" if maximise else "min", mc.tiled(mc.extreme_window(fx, fy, chroma, maximise), S, S, ORG - before, ORG - before)))
    out.append(("random", rng.integers(0, 256, (S, S), dtype=np.uint8)))
    return out


@pytest.mark.parametrize("chroma", [False, True], ids=["luma", "chroma"])
def test_model_equals_implementation_on_every_phase(impl, chroma):
    name, lib = impl
    rng = np.random.default_rng(40 + chroma)
    n, sizes = (8, CHROMA_SIZES) if chroma else (4, LUMA_SIZES)
    fn, fn_hi = ("sample_octpel_chroma", "sample_octpel_chroma_hi") if chroma else ("sample_quarterpel_luma", "sample_quarterpel_luma_hi")
    bad, extremes = [], 0
    for fx in range(n):
        for fy in range(n):
            for label, plane in _phase_planes(fx, fy, chroma, rng):
                src = A(plane.reshape(-1))
                for (w, h) in sizes:
                    v = mc.filter14(plane, ORG, ORG, w, h, (fx, fy), chroma)
                    if label != "random":
                        # the tiling puts the extreme window under the block's first sample: the content really reaches the phase's extreme
                        assert v[0, 0] == mc.extreme_sample(fx, fy, chroma, label == "max"), (fx, fy, label)
                        extremes += 1
                    mv = A(np.array([fx, fy], np.int16))
                    d8 = A(np.zeros(64 * 64 + 64, np.uint8))
                    _select(name, lib)
                    getattr(lib, fn)(ptr(src, offset=ORG * S + ORG), S, w, h, ptr(d8), 64, 1, 1, ptr(mv))
                    if not np.array_equal(d8[:64 * h].reshape(h, 64)[:, :w], mc.uni(v)):
                        bad.append((fx, fy, label, w, h, "uni"))
                    if name == "ref-avx2":
                        continue  # AVX2 saturates the 14-bit operand where generic wraps it: test_avx2_hi_saturates_where_generic_wraps
                    d16 = A(np.zeros(64 * 64 + 64, np.int16))
                    getattr(lib, fn_hi)(ptr(src, offset=ORG * S + ORG), S, w, h, ptr(d16), 64, 1, 1, ptr(mv))
                    if not np.array_equal(d16[:64 * h].reshape(h, 64)[:, :w], mc.hi(v)):
                        bad.append((fx, fy, label, w, h, "hi"))
    assert not bad, f"{len(bad)} blocks differ: {bad[:10]}"
    assert extremes == n * n * 2 * len(sizes)


def test_avx2_hi_saturates_where_generic_wraps():
    """the reference's two strategies disagree on the two-list operand at the luma (2, 2) phase: generic (and the oracle, and the model, and the device)
    wraps 33150 to -32386, AVX2 saturates it to 32767 (_mm256_packs_epi32).  The one-list sample is 255 in both."""
    import os
    oracle = flatapi.load_oracle()
    plane = mc.tiled(mc.extreme_window(2, 2, False), S, S, ORG - 3, ORG - 3)
    src = A(plane.reshape(-1))
    v = mc.filter14(plane, ORG, ORG, 16, 16, (2, 2), False)
    assert v[0, 0] == 33150 and mc.hi(v)[0, 0] == -32386 and mc.uni(v)[0, 0] == 255
    over = v > 32767
    assert over.sum() >= 4

    def run(lib):
        mv = A(np.array([2, 2], np.int16))
        d16, d8 = A(np.zeros(64 * 16, np.int16)), A(np.zeros(64 * 16, np.uint8))
        lib.sample_quarterpel_luma_hi(ptr(src, offset=ORG * S + ORG), S, 16, 16, ptr(d16), 64, 1, 1, ptr(mv))
        lib.sample_quarterpel_luma(ptr(src, offset=ORG * S + ORG), S, 16, 16, ptr(d8), 64, 1, 1, ptr(mv))
        return d16.reshape(16, 64)[:, :16].copy(), d8.reshape(16, 64)[:, :16].copy()
    o16, o8 = run(oracle)
    assert np.array_equal(o16, mc.hi(v)) and np.array_equal(o8, mc.uni(v))
    if not os.path.exists(flatapi.refshim_path()):
        pytest.skip("oracle/_ref not built: the oracle side is checked above")
    g16, g8 = run(flatapi.load_ref(0))
    a16, a8 = run(flatapi.load_ref(1))
    assert np.array_equal(g16, mc.hi(v)) and np.array_equal(g8, mc.uni(v)) and np.array_equal(a8, g8)
    assert (a16[over] == 32767).all() and (g16[over] < 0).all()
    assert np.array_equal(a16[~over], g16[~over])


def edge_pus(W, H):
    """PUs 8..64 (square and 2:1) at the picture's corners and centre, vectors that put the window over every edge (a few samples, half the block,
    far outside), fractional phases including luma (2, 2) and chroma phases 0..7"""
    phases = [(2, 2), (1, 3), (3, 1), (0, 2), (2, 0), (0, 0), (2, 1), (3, 3)]
    pus, k = [], 0
    for (w, h) in [(8, 8), (16, 8), (8, 16), (16, 16), (32, 16), (16, 32), (32, 32), (64, 32), (64, 64)]:
        for (x, y) in [(0, 0), (W - w, 0), (0, H - h), (W - w, H - h), ((W - w) // 2 & ~7, (H - h) // 2 & ~7)]:
            for d in (2, w // 2 + 3, 300):
                dx = -d if x == 0 else (d if x == W - w else (d if k % 2 else -d))
                dy = -d if y == 0 else (d if y == H - h else (d if k % 3 else -d))
                fx, fy = phases[k % len(phases)]
                mv = (4 * dx + fx + (4 if k % 4 == 1 else 0), 4 * dy + fy)   # k % 4 == 1: an odd integer part, a half chroma sample
                mv2 = (4 * (-dx // 2) + phases[(k + 3) % len(phases)][0], 4 * (dy // 3) + phases[(k + 3) % len(phases)][1])
                use = ((1, 0), (0, 1), (1, 1))[k % 3]
                pus.append((x, y, w, h, mv, mv2, use[0], use[1]))
                k += 1
    return pus


@pytest.mark.parametrize("content", ["extreme", "extreme-min", "random"])
def test_model_equals_reference_branches_off_every_edge(impl, content):
    """whole PUs through the reference's own branches (copy or filter, get_extended_block at the edge, pixel or 14-bit bipred operands: tests/test_gpu_fme.py
    oracle_inter_pred) against the model, PU by PU"""
    from test_gpu_fme import oracle_inter_pred
    name, lib = impl
    W, H = 136, 104
    rng = np.random.default_rng(3)
    if content == "random":
        refs = [A(rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8)), A(rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8))]
    else:
        e = A(mc.extreme_frame(W, H, maximise=content == "extreme"))
        refs = [e, A(np.where(rng.integers(0, 3, W * H * 3 // 2) > 0, 255, 0).astype(np.uint8))]
    bad, n = [], 0
    for pu in edge_pus(W, H):
        if name == "ref-avx2" and pu[6] and pu[7] and content != "random":
            continue  # two lists on extreme content: AVX2 saturates (test_avx2_hi_saturates_where_generic_wraps)
        n += 1
        _select(name, lib)
        if not np.array_equal(oracle_inter_pred(lib, refs, W, H, [pu]), mc.inter_pred(refs, W, H, [pu])):
            bad.append(pu)
    assert not bad, f"{len(bad)}/{n} PUs differ: {bad[:6]}"
    assert n >= 90


def test_edge_pus_reach_the_overflow():
    """the extreme frame under a (2, 2) vector: the model's 14-bit samples leave int16, the one-list samples are 255 there and the wrapped operand negative"""
    W, H = 136, 104
    e = mc.extreme_frame(W, H)
    yv = mc.filter14(e[:W * H].reshape(H, W), 0, 0, 64, 64, (2, 2), False)
    assert (yv > 32767).sum() >= 64 and (mc.uni(yv)[yv > 32767] == 255).all() and (mc.hi(yv)[yv > 32767] < 0).all()
    assert any(pu[4][0] & 3 == 2 and pu[4][1] & 3 == 2 and pu[6] and not pu[7] for pu in edge_pus(W, H))
