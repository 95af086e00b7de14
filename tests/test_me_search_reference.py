"""The integer motion searches of the inter CTU pass (kvz_inter_ctu_pix.inc me_integer under KVZ_ICTU_ME: hexbs with a step limit, dia, tz, the full searches, the
three early-termination settings) PU by PU against a plain-Python statement of the reference's searches (tests/me_search_reference.py), without a GPU: the device
sources run in host simulation (tests/hostsim/hostsim_inter_me.cpp kvz_hostsim_me_integer_pu) on pictures with real motion, random candidates, PUs at the frame's
corners and the MV constraint of --owf on.  Vector, cost and bits must be equal, the cost to the last bit: both sides add the same doubles in the same order."""
import ctypes as C

import numpy as np
import pytest

import inter_common as ic
import inter_lists_common as ilc
import inter_me_common as mec
import inter_mixed_common as imc
import me_search_reference as ref

W, H = 136, 72


@pytest.fixture(scope="module")
def sim():
    return mec.load_sim()


@pytest.fixture(scope="module")
def planes():
    """two pictures a fast pan apart (tests/inter_common.py clip): the searches have somewhere to go"""
    frames = ic.clip(W, H, 2, 5, 1.5, (11, -6))
    for f in frames:
        f.setflags(write=False)
    return frames[1], frames[0]  # source, reference


def cdiv(a, b):
    """C's integer division"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def golomb_bits(s):
    """get_ep_ex_golomb_bitcost (search_inter.c:250-268)"""
    bins = 0
    for shift, add in ((8, 16), (4, 8), (2, 4)):
        if s >= 1 << shift:
            bins += add
            s >>= shift
    return bins + (2 if s >= 2 else 0)


def mvd_bits(dx, dy):
    """get_mvd_coding_cost (search_inter.c:329-344)"""
    ax, ay = abs(dx), abs(dy)
    return 4 + (ax == 1) + (ay == 1) + golomb_bits(ax) + golomb_bits(ay)


class Pu:
    """one PU's cost function, in Python: the clamped SAD (image.c kvz_image_calc_sad), the MVD bits of the cheaper predictor (calc_mvd_cost / select_mv_cand with
    cost_out), fracmv_within_tile under --owf (search_inter.c:94-147; mv_constraint none otherwise)"""

    def __init__(self, src, refp, x, y, w, mv_cand, mv_constraint, sao, deblock):
        self.x, self.y, self.w, self.mv_cand, self.constraint, self.sao, self.deblock = x, y, w, mv_cand, mv_constraint, sao, deblock
        self.ref = refp[:W * H].reshape(H, W).astype(np.int32)
        self.block = src[:W * H].reshape(H, W)[y:y + w, x:x + w].astype(np.int32)

    def allowed(self, qx, qy):
        if not self.constraint:
            return True
        margin = 4 if (qx % 4 or qy % 4) else (2 if (qx % 8 or qy % 8) else 0)
        margin += 10 if self.sao else (8 if self.deblock else 0)
        lx = cdiv((self.x + self.w + margin) * 4 + qx, 256) - self.x // 64
        ly = cdiv((self.y + self.w + margin) * 4 + qy, 256) - self.y // 64
        return not (ly > 1) and not (lx + ly > 2)

    def probe(self, x, y):
        if not self.allowed(x * 4, y * 4):
            return None
        ys = np.clip(np.arange(self.y + y, self.y + y + self.w), 0, H - 1)
        xs = np.clip(np.arange(self.x + x, self.x + x + self.w), 0, W - 1)
        sad = int(np.abs(self.block - self.ref[np.ix_(ys, xs)]).sum())
        return sad, min(mvd_bits(x * 4 - c[0], y * 4 - c[1]) for c in self.mv_cand)


def sim_pu(sim, src, refp, pu, merge, start, qp, fields):
    from kvazaar_amd.inter import InterParams, me_search_fields
    prm = InterParams(qp=qp, poc=1, mv_constraint=int(pu.constraint), sao=int(pu.sao), deblock=int(pu.deblock), fme_level=2, pu_depth_inter_max=3, no_wpp=0, fast_residual_cost=28,
                      **me_search_fields(**fields))
    fb, wts = imc.model_constants()
    cand = np.array(pu.mv_cand, np.int16).reshape(-1)
    mrg = np.array([[mx, my, mx, my, d] if d != 3 else [mx, my, -mx, my + 4, 3] for mx, my, d in merge], np.int16).reshape(-1) if merge else np.zeros(5, np.int16)
    mv, cost, bits = (C.c_int32 * 2)(), C.c_double(), C.c_double()
    f = sim.kvz_hostsim_me_integer_pu
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 3
    rc = f(W, H, C.addressof(prm), wts.ctypes.data, fb.ctypes.data, src.ctypes.data, refp.ctypes.data, pu.x, pu.y, pu.w, cand.ctypes.data, mrg.ctypes.data, len(merge),
           int(start is not None), start[0] if start else 0, start[1] if start else 0, mv, C.byref(cost), C.byref(bits))
    assert rc == 0
    return (mv[0], mv[1]), cost.value, bits.value


# (x, y, size), aligned to the size as the PUs of a CTU are: the corners of the picture, a PU of every size inside it, PUs whose windows leave the frame at one side only
PUS = [(0, 0, 8), (W - 8, 0, 8), (0, H - 8, 8), (W - 8, H - 8, 8), (64, 32, 16), (32, 0, 32), (96, 32, 32), (16, 48, 16), (112, 16, 16), (72, 64, 8)]
SETTINGS = [dict(me=m, me_early_termination=t) for m in ("hexbs", "dia", "tz", "full8", "full16") for t in ("sensitive", "on", "off")] + \
           [dict(me=m, me_steps=s, me_early_termination="off") for m in ("hexbs", "dia") for s in (1, 2, 3)] + \
           [dict(me="full32", me_early_termination="off"), dict(me="full", me_early_termination="off"), dict(me="full64", me_early_termination="off")]


@pytest.mark.parametrize("fields", SETTINGS, ids=lambda f: "-".join(str(v) for v in f.values()))
def test_search_of_one_pu_equals_the_python_statement(sim, planes, fields):
    src, refp = planes
    big = fields["me"] in ("full32", "full", "full64")
    rng = np.random.default_rng(sum(map(ord, str(sorted(fields.items())))))
    ilc.mul24_violations(sim, reset=True)
    moved = probes = 0
    for n, (x, y, w) in enumerate(PUS if not big else [p for p in PUS if p[2] == 8]):
        for constraint in (0, 1):
            # candidates around the true motion (11, -6), one of both lists, sometimes a repeat and sometimes zero; a co-located vector that may not be allowed
            merge = [(int(rng.integers(-70, 70)), int(rng.integers(-50, 50)), int(rng.choice((1, 1, 2, 3)))) for _ in range(int(rng.integers(0, 6)))]
            if merge and n % 3 == 0:
                merge[-1] = (merge[0][0] + 1, merge[0][1], 1)  # the same integer position as the first
            if len(merge) > 2 and n % 4 == 1:
                merge[1] = (1, -1, 2)  # rounds to zero
            mv_cand = [(int(rng.integers(-60, 60)), int(rng.integers(-40, 40))) for _ in range(2)]
            if n % 5 == 2:
                mv_cand[1] = mv_cand[0]
            start = None if n % 4 == 3 else (int(rng.integers(-64, 64)), int(rng.integers(-48, 48)))
            pu = Pu(src, refp, x, y, w, mv_cand, constraint, sao=n % 2, deblock=1)
            qp = (22, 27, 37)[n % 3]
            got = sim_pu(sim, src, refp, pu, merge, start, qp, fields)
            mv, cost, bits, made = ref.me_integer(pu.probe, pu.allowed, ic.lambda_sqrt(qp), merge, start, **fields)
            assert got == (mv, cost, bits), (fields, (x, y, w), constraint, merge, mv_cand, start, got, (mv, cost, bits))
            moved += mv != (0, 0)
            probes += made
    assert ilc.mul24_violations(sim) == 0
    assert moved > 0 and probes > 0


def test_zero_members_are_the_default_search(sim, planes):
    """me_algorithm = me_max_steps = me_early_termination = 0 runs the program's default text (KVZ_ICTU_ME 0): hexbs, no step limit, sensitive"""
    src, refp = planes
    for x, y, w in PUS:
        pu = Pu(src, refp, x, y, w, [(40, -20), (0, 0)], 0, 1, 1)
        merge = [(44, -24, 1), (8, 8, 3)]
        got = sim_pu(sim, src, refp, pu, merge, (40, -28), 27, {})
        mv, cost, bits, _ = ref.me_integer(pu.probe, pu.allowed, ic.lambda_sqrt(27), merge, (40, -28))
        assert got == (mv, cost, bits), (x, y, w)
