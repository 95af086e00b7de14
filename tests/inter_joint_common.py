"""Joint launches of the inter CTU pass (kvz_hip_dev_inter_ctu_pass_groups: groups of B pictures of different sizes in one launch), as tests/test_inter_joint_sim.py
(host simulation) and tests/test_gpu_inter_joint.py (device) build them.  Pictures come from tests/inter_mixed_common.py: B pictures of low-delay sequences the oracle
encoded ALONE (the oracle pinned to the reference encoder), so every picture's expected outputs are those of its own sequence's encode; nothing here is computed by
the code under test."""
import ctypes as C
import functools

import numpy as np

import inter_common as ic
import inter_mixed_common as mx

# the smallest sizes that cover the ways geometry can go wrong: 1x1 CTUs (no neighbour at all), 2x1 (width 8 mod 16, one row), 3x2 (partial CTUs right and bottom),
# 5x3 (the above-right wait, the context inheritance after the second CTU of a row)
SIZES = ((40, 24), (72, 40), (136, 72), (264, 136))
COUNTS = (2, 2, 3, 1)


def grid(w, h):
    return (w + 63) // 64, (h + 63) // 64


@functools.lru_cache(maxsize=None)
def sequence(qp, preset="veryfast", seed=0, w=136, h=72, n=4, no_wpp=False, mv_constraint=True, parts=True):
    """inter_mixed_common.sequence for every size of SIZES.  That function draws its content from inter_common.clip, whose moving rectangles need a picture beyond
    40 samples a side; the two small sizes take the content the inter fuzz gives pictures that small (inter_common.hard_clip: a panned sine texture over the whole
    sample range).  Same dictionary, same oracle encode, shared and never modified."""
    if w > 40 and h > 40:
        return mx.sequence(qp, preset=preset, seed=seed, w=w, h=h, n=n, no_wpp=no_wpp, mv_constraint=mv_constraint, parts=parts)
    import flatapi
    oracle = flatapi.load_oracle()
    frames = ic.hard_clip("smooth", w, h, n, 100 + seed, (1.25, -0.5))
    kw = dict(preset=preset, deblock=True, sao=True, mv_constraint=mv_constraint, no_wpp=no_wpp)
    rs, rf, cu, qps = ic.oracle_encode(oracle, w, h, frames, qp, **kw)
    s = dict(frames=frames, rs=rs, rf=rf, cu=cu, qps=[int(q) for q in qps], w=w, h=h, preset=preset)
    if parts:
        s["parts"] = ic.oracle_encode_parts(oracle, w, h, frames, qp, **kw)
        s["bits"] = ic.oracle_encode_bits(oracle, w, h, frames, qp, **kw)
        assert [int(q) for q in s["parts"]["qps"]] == s["qps"]
    for v in (rs, rf, cu):
        v.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def veryfast_groups():
    """the four sizes with 2, 2, 3 and 1 pictures, `veryfast` with the loop-filter switches on: sequences at --qp 22, 32, 27, 37, picture QPs on both sides of
    fast-residual-cost 28 (the 136x72 group alone has both), POC 1, 2 and 3 -> ((w, h, (pictures ...)) ...)"""
    plan = ((22, (1, 2)), (32, (2, 3)), (27, (1, 2, 3)), (37, (3,)))
    groups = []
    for i, ((w, h), (qp, ks)) in enumerate(zip(SIZES, plan)):
        s = sequence(qp, seed=40 + i, w=w, h=h, n=4)
        groups.append((w, h, tuple(mx.picture(s, k) for k in ks)))
    qps, pocs = [p["qp"] for g in groups for p in g[2]], [p["poc"] for g in groups for p in g[2]]
    assert min(qps) < 28 <= max(qps) and {1, 2, 3} <= set(pocs) and tuple(len(g[2]) for g in groups) == COUNTS, (qps, pocs)
    return tuple(groups)


@functools.lru_cache(maxsize=None)
def no_wpp_groups():
    """the same sizes and counts for a launch with no_wpp = 1, mv_constraint = 0: POC 1 pictures of --no-wpp sequences at --qp 22 and 32, each of its own sequence"""
    groups, seed = [], 60
    for (w, h), n in zip(SIZES, COUNTS):
        pics = []
        for _ in range(n):
            pics.append(mx.picture(sequence((22, 32)[seed & 1], seed=seed, w=w, h=h, n=2, no_wpp=True, mv_constraint=False, parts=False), 1))
            seed += 1
        groups.append((w, h, tuple(pics)))
    qps = [p["qp"] for g in groups for p in g[2]]
    assert min(qps) < 28 <= max(qps), qps
    return tuple(groups)


@functools.lru_cache(maxsize=None)
def faster_groups():
    """`faster` (fast-residual-cost 0: every picture on the residual coder; quarter-sample search): 136x72 and 72x40, two pictures each"""
    groups = []
    for i, ((w, h), qp, ks) in enumerate((((136, 72), 24, (1, 2)), ((72, 40), 33, (2, 1)))):
        s = sequence(qp, preset="faster", seed=80 + i, w=w, h=h, n=3)
        groups.append((w, h, tuple(mx.picture(s, k) for k in ks)))
    return tuple(groups)


def table_of(pics):
    from kvazaar_amd.inter import InterPictureParams
    return InterPictureParams([p["qp"] for p in pics], [p["poc"] for p in pics])


def group_array(n):
    from kvazaar_amd.inter import InterGroupStruct
    return (InterGroupStruct * n)()


class HostLaunch:
    """the groups of a launch as host arrays in the pass's layouts, and their kvz_hip_inter_group array.  with_coeff: per group, False = coeff NULL; tables: per
    group an InterPictureParams, None = the group's own QPs and POCs, False = pictures NULL.  Outputs start as `fill`"""

    def __init__(self, groups, with_coeff=None, tables=None, fill=0):
        from kvazaar_amd.inter import InterGroupStruct
        self.groups = groups
        n = len(groups)
        with_coeff = [True] * n if with_coeff is None else with_coeff
        tables = [None] * n if tables is None else tables
        self.src, self.ref, self.ref_cu, self.rec, self.cu, self.coeff, self.tables = [], [], [], [], [], [], []
        self.structs = group_array(n)
        for g, (w, h, pics), wc, t in zip(self.structs, groups, with_coeff, tables):
            m, fs, cells, ctus = len(pics), w * h * 3 // 2, (w // 4) * (h // 4), grid(w, h)[0] * grid(w, h)[1]
            self.src.append(mx.stacked(pics, "src"))
            self.ref.append(mx.stacked(pics, "ref"))
            self.ref_cu.append(np.concatenate([np.ascontiguousarray(p["ref_cu"]).reshape(-1) for p in pics]))
            self.rec.append(np.full(m * fs, fill, np.uint8))
            self.cu.append(np.frombuffer(bytes([fill]) * (m * cells * ic.CU_DTYPE.itemsize), ic.CU_DTYPE).copy())
            self.coeff.append(np.full(m * ctus * 6144, fill * 257, np.int16) if wc else None)
            self.tables.append(None if t is False else (table_of(pics) if t is None else t))
            g.struct_size, g.width, g.height, g.n_pictures = C.sizeof(InterGroupStruct), w, h, m
            g.src, g.ref, g.ref_cu, g.rec, g.cu = (a[-1].ctypes.data for a in (self.src, self.ref, self.ref_cu, self.rec, self.cu))
            g.coeff = self.coeff[-1].ctypes.data if wc else None
            g.pictures = self.tables[-1].ptr if self.tables[-1] is not None else None

    def run(self, sim, params, n_groups=None):
        fb, wts = mx.model_constants()
        f = sim.kvz_hostsim_inter_pass_groups
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        return f(C.addressof(self.structs), len(self.groups) if n_groups is None else n_groups, C.addressof(params), wts.ctypes.data, fb.ctypes.data)

    def outputs(self, i):
        """(rec [n, fs], cu [n, h/4, w/4], coeff [n, ctus * 6144] or None) of group i"""
        w, h, pics = self.groups[i]
        m = len(pics)
        return self.rec[i].reshape(m, -1), self.cu[i].reshape(m, h // 4, w // 4), None if self.coeff[i] is None else self.coeff[i].reshape(m, -1)

    def untouched(self, fill):
        return all((r == fill).all() for r in self.rec) and all((c.view(np.uint8) == fill).all() for c in self.cu) and all(c is None or (c == fill * 257).all() for c in self.coeff)


def assert_groups_equal_the_oracle(launch):
    for i, (w, h, pics) in enumerate(launch.groups):
        rec, cu, _ = launch.outputs(i)
        mx.assert_pictures_equal_the_oracle(pics, rec, cu)


def device_members(lib, groups, with_levels=None):
    """an InterPictures per group with the group's pictures uploaded"""
    from kvazaar_amd import inter
    with_levels = [True] * len(groups) if with_levels is None else with_levels
    members = []
    for (w, h, pics), lv in zip(groups, with_levels):
        ip = inter.InterPictures(lib, w, h, len(pics), with_levels=lv)
        for i, p in enumerate(pics):
            ip.upload(i, p["src"], p["ref"], np.ascontiguousarray(p["ref_cu"]).reshape(-1))
        members.append(ip)
    return members


def assert_member_equals_the_oracle(ip, pics):
    for i, p in enumerate(pics):
        rec, cu = ip.download(i)
        where = (ip.w, ip.h, i, p["qp"], p["poc"])
        assert ic.first_difference(cu[None], np.asarray(p["cu"])[None]) is None, where
        assert np.array_equal(rec, p["rec"]), where
