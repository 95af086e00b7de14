"""Host side of the inter CTU pass (include/kvz_hip_dev.h kvz_hip_dev_inter_ctu_pass): the CU record layout, the per-picture parameters and a thin wrapper that
keeps the pictures of many independent sequences on the device.  The product path: no oracle, no CPU fallback -- the library call fails if the HIP kernels are missing."""
import ctypes as C
import os
import hashlib

import numpy as np

CU_DTYPE = np.dtype([("type", "u1"), ("depth", "u1"), ("mode", "u1"), ("tr_depth", "u1"), ("cbf", "<u2"), ("skipped", "u1"), ("merged", "u1"), ("merge_idx", "u1"),
                     ("mv_dir", "u1"), ("mv_ref", "u1", (2,)), ("mv_cand", "u1", (2,)), ("mv", "<i2", (2, 2))], align=True)  # kvz_hip_cu_info
assert CU_DTYPE.itemsize == 22


class InterParams(C.Structure):  # kvz_hip_inter_params
    _fields_ = [("struct_size", C.c_uint32)] + [(n, C.c_int32) for n in ("qp", "poc", "mv_constraint", "sao", "deblock", "fme_level", "pu_depth_inter_max", "no_wpp", "fast_residual_cost",
                                                "ref_width", "ref_height", "tile_x", "tile_y", "no_tmvp",  # ref_width .. tile_y: tiles (include/kvz_hip_dev.h), zero = the picture is the frame
                                                "me_algorithm", "me_max_steps", "me_early_termination")]  # the integer motion search (me_search_fields), zero = hexbs, no step limit, sensitive


    def __init__(self, **kw):
        super().__init__(**kw)
        if "struct_size" not in kw:
            self.struct_size = C.sizeof(InterParams)  # the version of the struct this binding was written against (include/kvz_hip_dev.h)


ME_ALGORITHMS = {"hexbs": 0, "tz": 1, "full": 2, "full8": 3, "full16": 4, "full32": 5, "full64": 6, "dia": 7}  # kvazaar's enum kvz_ime_algorithm
ME_EARLY_TERMINATION = {"sensitive": 0, "on": 1, "off": 2}  # kvz_hip_inter_params' own order: zero is what every preset up to `fast` runs


def me_search_fields(me="hexbs", me_steps=-1, me_early_termination="sensitive"):
    """kvazaar's --me, --me-steps and --me-early-termination as the three members of kvz_hip_inter_params: InterParams(..., **me_search_fields(me="tz")).
    me_steps: -1 (kvazaar's default, no limit) or a count >= 1"""
    if me not in ME_ALGORITHMS:
        raise ValueError(f"--me {me}: one of {', '.join(ME_ALGORITHMS)}")
    if me_early_termination not in ME_EARLY_TERMINATION:
        raise ValueError(f"--me-early-termination {me_early_termination}: one of {', '.join(ME_EARLY_TERMINATION)}")
    if me_steps != -1 and me_steps < 1:
        raise ValueError(f"--me-steps {me_steps}: -1 (no limit) or a count of at least 1")
    return dict(me_algorithm=ME_ALGORITHMS[me], me_max_steps=0 if me_steps == -1 else int(me_steps), me_early_termination=ME_EARLY_TERMINATION[me_early_termination])


SLICE_TYPES = {"B": 0, "P": 1, "I": 2}  # KVZ_HIP_SLICE_* (include/kvz_hip_types.h), kvazaar's enum kvz_slices


def slice_type_value(slice_type):
    """"B" / "P" / "I" (or the KVZ_HIP_SLICE_* number itself, which the library checks) -> the argument of the kvz_hip_dev_*_slices entry points"""
    if isinstance(slice_type, str):
        if slice_type not in SLICE_TYPES:
            raise ValueError(f"slice type {slice_type!r}: one of {', '.join(SLICE_TYPES)}")
        return SLICE_TYPES[slice_type]
    return int(slice_type)


class InterPicturesStruct(C.Structure):  # kvz_hip_inter_pictures
    _fields_ = [("struct_size", C.c_uint32), ("n_pictures", C.c_int32), ("qp", C.c_void_p), ("poc", C.c_void_p)]


class InterPictureParams:
    """a QP and a POC per picture of one launch (kvz_hip_inter_pictures): the `pictures=` of InterPictures.run / .loop_filters / .entropy_code.  Everything else --
    preset, switches, geometry -- stays the launch's InterParams, whose qp and poc are then ignored"""

    def __init__(self, qps, pocs, references=None):
        """references (InterReferences): the pictures are P pictures with reference lists over the object's pool -- InterPictures.run / .loop_filters /
        .entropy_code then go through the kvz_hip_dev_*_refs entry points (slice_type="P"); the lists travel with the POCs they are checked against"""
        self.qps, self.pocs = np.ascontiguousarray(qps, np.int32).reshape(-1), np.ascontiguousarray(pocs, np.int32).reshape(-1)
        if self.qps.size != self.pocs.size:
            raise ValueError(f"{self.qps.size} QPs for {self.pocs.size} POCs")
        if references is not None and len(references) != self.qps.size:
            raise ValueError(f"{len(references)} reference lists for {self.qps.size} pictures")
        self.references = references
        self.struct = InterPicturesStruct(struct_size=C.sizeof(InterPicturesStruct), n_pictures=self.qps.size, qp=self.qps.ctypes.data, poc=self.pocs.ctypes.data)  # (the arrays live as long as self)

    def __len__(self):
        return int(self.qps.size)

    @property
    def ptr(self):
        return C.addressof(self.struct)


MAX_REFS = 4  # KVZ_HIP_MAX_REFS


class InterRefsStruct(C.Structure):  # kvz_hip_inter_refs
    _fields_ = [("struct_size", C.c_uint32), ("n_pictures", C.c_int32), ("n_frames", C.c_int32)] + [(n, C.c_void_p) for n in ("frame_poc", "frame_ref_poc", "n_refs", "ref_frame")]


class InterReferences:
    """the reference picture lists of the P pictures of one launch over a pool of reference frames (kvz_hip_inter_refs): the `references=` of InterPictureParams,
    which InterPictures.run / .loop_filters / .entropy_code take as `pictures`.  frame_pocs [n_frames]: the POC of every frame of the pool; frame_ref_pocs [n_frames][<= 4]: the POCs that frame's own list
    named when it was coded (an I frame: anything); n_refs [n_pictures]: the length of every picture's list; ref_frames [n_pictures][<= 4]: the pool indices of
    its entries in list order.  The library checks the table when a launch is made"""

    def __init__(self, frame_pocs, frame_ref_pocs, n_refs, ref_frames):
        def rows(a, n):
            out = np.zeros((n, MAX_REFS), np.int32)
            for i, row in enumerate(a):
                row = [int(v) for v in row][:MAX_REFS]
                out[i, :len(row)] = row
            return out
        self.frame_pocs = np.ascontiguousarray(frame_pocs, np.int32).reshape(-1)
        self.n_refs = np.ascontiguousarray(n_refs, np.int32).reshape(-1)
        if len(frame_ref_pocs) != self.frame_pocs.size or len(ref_frames) != self.n_refs.size:
            raise ValueError(f"{len(frame_ref_pocs)} rows of reference POCs for {self.frame_pocs.size} frames, {len(ref_frames)} lists for {self.n_refs.size} pictures")
        self.frame_ref_pocs, self.ref_frames = rows(frame_ref_pocs, self.frame_pocs.size), rows(ref_frames, self.n_refs.size)
        self.struct = InterRefsStruct(struct_size=C.sizeof(InterRefsStruct), n_pictures=self.n_refs.size, n_frames=self.frame_pocs.size, frame_poc=self.frame_pocs.ctypes.data,
                                      frame_ref_poc=self.frame_ref_pocs.ctypes.data, n_refs=self.n_refs.ctypes.data, ref_frame=self.ref_frames.ctypes.data)  # (the arrays live as long as self)

    def __len__(self):
        return int(self.n_refs.size)

    @property
    def ptr(self):
        return C.addressof(self.struct)


def lowdelay_ref_distances(g, ref, gop_len):
    """the POC distances picture g (1 .. gop_len) of `--gop lp-g<gop_len>d<..>t1 --ref <ref>` asks for (cfg.c:1468-1507 with t = 1): the previous picture, then the
    previous key pictures -- g, g + gop_len, ... back, skipping a distance the entry before already has"""
    neg = [1]
    keyframe = g
    for i in range(1, ref):
        while keyframe == neg[i - 1]:
            keyframe += gop_len
        neg.append(keyframe)
    return neg


def reference_pocs(poc, ref, gop="lp-g4d3t1"):
    """the POCs of picture `poc`'s list L0, in list order, under kvazaar's `--gop <gop> --ref <ref>` with one I picture at POC 0: `gop` "0" -- the previous `ref`
    pictures, as far as they exist --, or "lp-g<len>d<depth>t1" -- the pictures at lowdelay_ref_distances that are still in the decoded picture buffer, which drops
    every picture the current one does not ask for (encoderstate.c:1139-1182).  L0 is ordered by descending POC (encoderstate.c:1040-1115)"""
    if poc < 1:
        return []
    if gop == "0":
        return [poc - d for d in range(1, ref + 1) if poc - d >= 0]
    if not (gop.startswith("lp-g") and gop.endswith("t1") and "d" in gop):
        raise ValueError(f"--gop {gop}: \"0\" or lp-g<len>d<depth>t1")
    gop_len = int(gop[4:gop.index("d")])
    dpb = [0]
    for p in range(1, poc + 1):
        wanted = [p - d for d in lowdelay_ref_distances((p - 1) % gop_len + 1, ref, gop_len)]
        dpb = [q for q in dpb if q in wanted]
        if p == poc:
            return sorted(dpb, reverse=True)
        dpb.append(p)


def veryfast_params(qp, poc, mv_constraint=True):
    """`--preset veryfast` (cfg.c:541-568) for a B picture of the low-delay GOP"""
    p = InterParams(qp=qp, poc=poc, mv_constraint=int(mv_constraint), sao=1, deblock=1, fme_level=2, pu_depth_inter_max=3, no_wpp=0, fast_residual_cost=28)
    import os
    for k in os.environ.get("KVZ_DEBUG_INTER_PARAMS", "").split(","):  # developer: timing experiments (e.g. no_tmvp=1,mv_constraint=0); the results no longer verify
        if "=" in k:
            setattr(p, k.split("=")[0], int(k.split("=")[1]))
    return p


def lowdelay_picture_qp(qp, frame, gop_len=4, gop_depth=3, intra_period=0, preset_given=True):
    """the picture QP kvazaar runs picture `frame` of `--gop lp-g<len>d<depth>t1 -q <qp>` at, without rate control: intra_qp_offset for the I picture
    (encoder.c:180-183), the GOP layer for the others (cfg.c:1455-1463) plus -- when a preset was given, whose "gop 8" leaves the random-access GOP's QP model in
    the entries kvz_config_process_lp_gop does not rewrite (cfg.c:485-760, gop.h:94-200) -- CLIP(0, 3, qp * scale + offset) of rate_control.c:1040-1056"""
    ra8_offset = (0.0, -6.25, -6.25, -7.0, -7.0, -6.25, -7.0, -7.0)
    ra8_scale = (0.0, 0.25, 0.25, 0.245, 0.245, 0.25, 0.245, 0.245)
    pos = frame % intra_period if intra_period else frame
    if pos == 0:
        l2 = 0
        while (1 << l2) < gop_len:
            l2 += 1
        q = qp + (max(-l2 + 1, -3) if gop_len > 1 else 0)
    else:
        k = (pos + gop_len - 1) % gop_len
        g = k + 1
        modulo = [0] * 8
        for d in range(gop_depth):
            modulo[gop_depth - 1 - d] = 1 << d
        modulo[0] = gop_len
        layer = 1
        while layer < gop_depth and g % modulo[layer - 1]:
            layer += 1
        dq = float(qp + layer)
        if preset_given and k < 8:
            dq += min(3.0, max(0.0, dq * ra8_scale[k] + ra8_offset[k]))
        q = int(dq + 0.5)
    return min(51, max(0, q))


def intra_picture_cu_info(width, height):
    """the CU info of an I picture as far as the next picture's search reads it (no motion: no temporal candidates, no co-located starting point)"""
    cu = np.zeros((height // 4, width // 4), CU_DTYPE)
    cu["type"] = 1
    cu["mv_ref"] = 255
    return cu


def cu_decision_bytes(cu):
    """the decisions of one picture as bytes, motion and flags only where they mean something (the digests of tests/golden/inter_recon.json are taken over these)"""
    inter = cu["type"] == 2
    coded = inter & (cu["merged"] == 0) & (cu["skipped"] == 0)
    parts = [cu["type"], cu["depth"], np.where(cu["type"] == 1, cu["mode"], 0), np.where(inter, cu["skipped"], 0), np.where(inter, cu["merged"], 0),
             np.where(inter & ((cu["merged"] | cu["skipped"]) > 0), cu["merge_idx"], 0), np.where(inter, cu["mv_dir"], 0)]
    for l in range(2):
        used = inter & ((cu["mv_dir"] >> l) & 1 > 0)
        parts += [np.where(used, cu["mv"][..., l, 0], 0).astype("<i2"), np.where(used, cu["mv"][..., l, 1], 0).astype("<i2"), np.where(coded & used, cu["mv_cand"][..., l], 0)]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def cu_digest(cu):
    return hashlib.sha256(cu_decision_bytes(cu)).hexdigest()[:24]


class InterPictures:
    """picture k of `n` independent sequences, resident on the device: sources, references (+ their CU info), and the pass's outputs"""

    def __init__(self, lib, width, height, n, with_levels=False, pool=1):
        """pool: reference frames kept per picture slot (P pictures with reference lists: kvz_hip_dev_*_refs).  The reference buffers then hold pool * n frames,
        frame s * n + i = slot s of sequence i; with pool == 1 they are what they have always been"""
        from .dev import Dev
        self.lib, self.dev, self.w, self.h, self.n, self.pool = lib, Dev(lib), width, height, n, int(pool)
        if self.pool < 1:
            raise ValueError(f"pool {pool}: at least one reference frame per picture")
        self.fs, self.cells = width * height * 3 // 2, (width // 4) * (height // 4)
        lib.kvz_hip_dev_inter_ctu_pass.restype = C.c_int
        lib.kvz_hip_dev_inter_ctu_pass.argtypes = [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_void_p]
        lib.kvz_hip_dev_cu_dbk_from_info.restype = None
        lib.kvz_hip_dev_cu_dbk_from_info.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.kvz_hip_dev_loop_filters_inter.restype = C.c_int
        lib.kvz_hip_dev_loop_filters_inter.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 3
        lib.kvz_hip_dev_inter_ctu_pass_pictures.restype = C.c_int
        lib.kvz_hip_dev_inter_ctu_pass_pictures.argtypes = [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        lib.kvz_hip_dev_loop_filters_inter_pictures.restype = C.c_int
        lib.kvz_hip_dev_loop_filters_inter_pictures.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 3
        lib.kvz_hip_dev_entropy_code_inter_pictures.restype = C.c_long
        lib.kvz_hip_dev_entropy_code_inter_pictures.argtypes = [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        if hasattr(lib, "kvz_hip_dev_inter_ctu_pass_lists"):  # (a library from before the entry point still loads: tools/bench_inter_scaling_lists.py times one)
            lib.kvz_hip_dev_inter_ctu_pass_lists.restype = C.c_int
            lib.kvz_hip_dev_inter_ctu_pass_lists.argtypes = [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        if hasattr(lib, "kvz_hip_dev_inter_ctu_pass_slices"):  # (likewise: tools/bench_inter_p.py times the library of the parent commit)
            lib.kvz_hip_dev_inter_ctu_pass_slices.restype = C.c_int
            lib.kvz_hip_dev_inter_ctu_pass_slices.argtypes = [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
            lib.kvz_hip_dev_loop_filters_inter_slices.restype = C.c_int
            lib.kvz_hip_dev_loop_filters_inter_slices.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 3
            lib.kvz_hip_dev_entropy_code_inter_slices.restype = C.c_long
            lib.kvz_hip_dev_entropy_code_inter_slices.argtypes = [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
        self.d_dbk = None
        lib.kvz_hip_dev_entropy_code_inter.restype = C.c_long
        lib.kvz_hip_dev_entropy_code_inter.argtypes = [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        e = self.dev.empty
        self.d_src, self.d_ref, self.d_rec = e(n * self.fs), e(self.pool * n * self.fs), e(n * self.fs)
        self.d_ref_cu, self.d_cu = e(self.pool * n * self.cells * CU_DTYPE.itemsize), e(n * self.cells * CU_DTYPE.itemsize)
        if hasattr(lib, "kvz_hip_dev_inter_ctu_pass_refs"):  # (a library from before the entry points still loads: tools/bench_inter_refs.py times the parent commit's)
            lib.kvz_hip_dev_inter_ctu_pass_refs.restype = C.c_int
            lib.kvz_hip_dev_inter_ctu_pass_refs.argtypes = [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
            lib.kvz_hip_dev_loop_filters_inter_refs.restype = C.c_int
            lib.kvz_hip_dev_loop_filters_inter_refs.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 4
            lib.kvz_hip_dev_entropy_code_inter_refs.restype = C.c_long
            lib.kvz_hip_dev_entropy_code_inter_refs.argtypes = [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
            lib.kvz_hip_dev_copy.restype = None
            lib.kvz_hip_dev_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        self.ctus = ((width + 63) // 64) * ((height + 63) // 64)
        self.d_coeff = e(n * self.ctus * 6144 * 2) if with_levels else None  # KVZ_HIP_CTU_COEFFS int16 per CTU: what the entropy coder reads
        self._entropy_out = None
        self._list_sets, self._list_index, self._n_list_sets = None, None, 0  # set_scaling_lists

    def upload(self, i, src, ref, ref_cu):
        up = self.lib.kvz_hip_dev_upload
        for base, a, size in ((self.d_src, src, self.fs), (self.d_ref, ref, self.fs), (self.d_ref_cu, ref_cu, self.cells * CU_DTYPE.itemsize)):
            a = np.ascontiguousarray(a)
            assert a.nbytes == size
            up(base + i * size, a.ctypes.data, size)

    FLAT = 0xffff  # set_of_picture: the picture stays without lists

    def set_scaling_lists(self, sets, set_of_picture=None):
        """Later run() calls quantise picture i under sets[set_of_picture[i]] (InterPictures.FLAT: flat; None: every picture under sets[0]) through
        kvz_hip_dev_inter_ctu_pass_lists.  sets: a sequence of batch.ScalingLists, the conventions of HipBatch.set_scaling_lists; an empty sequence clears.  State of
        the object until changed or cleared.  The library checks the sets when a launch is made: run() raises when it refuses them (see stderr)"""
        from .batch import ScalingListsStruct
        sets = list(sets)
        if not sets:
            self._list_sets, self._list_index, self._n_list_sets = None, None, 0
            return
        index = None
        if set_of_picture is not None:
            if len(set_of_picture) != self.n:
                raise ValueError(f"set_of_picture of {len(set_of_picture)} pictures for {self.n}")
            index = (C.c_uint16 * self.n)(*[int(v) for v in set_of_picture])
        self._list_sets, self._list_index, self._n_list_sets = (ScalingListsStruct * len(sets))(*[s.struct for s in sets]), index, len(sets)

    def clear_scaling_lists(self):
        """the object is again what it was before the first set_scaling_lists"""
        self.set_scaling_lists([])

    def upload_pool(self, slot, i, ref, ref_cu):
        """slot `slot` of sequence i's reference pool: a reference frame (after its loop filters) and its CU records"""
        if not 0 <= slot < self.pool:
            raise ValueError(f"slot {slot} of a pool of {self.pool}")
        for base, a, size in ((self.d_ref, ref, self.fs), (self.d_ref_cu, ref_cu, self.cells * CU_DTYPE.itemsize)):
            a = np.ascontiguousarray(a)
            assert a.nbytes == size
            self.lib.kvz_hip_dev_upload(base + (slot * self.n + i) * size, a.ctypes.data, size)

    def pool_frame(self, slot, i):
        """the index into the pool (InterReferences ref_frames) of slot `slot` of sequence i"""
        return slot * self.n + i

    def advance_pool(self, keep):
        """the pictures just encoded (after their loop filters) and their CU records move into slot `keep` of every sequence's pool, on the device: the next
        pictures' lists can name them"""
        if not 0 <= keep < self.pool:
            raise ValueError(f"slot {keep} of a pool of {self.pool}")
        self.lib.kvz_hip_dev_copy(self.d_ref + keep * self.n * self.fs, self.d_rec, self.n * self.fs)
        self.lib.kvz_hip_dev_copy(self.d_ref_cu + keep * self.n * self.cells * CU_DTYPE.itemsize, self.d_cu, self.n * self.cells * CU_DTYPE.itemsize)

    def run(self, params, pictures=None, slice_type="B"):
        """the CTU pass of the n pictures; pictures (InterPictureParams): every picture at its own QP and POC instead of params.qp / params.poc.  While the object
        holds scaling lists (set_scaling_lists) the launch is kvz_hip_dev_inter_ctu_pass_lists.
        slice_type: "B" (the default: the calls this method has always made) or "P" -- kvazaar's --no-bipred -- through kvz_hip_dev_inter_ctu_pass_slices, as is
        every slice type given as a KVZ_HIP_SLICE_* number.  P pictures take no scaling lists"""
        references = getattr(pictures, "references", None)
        if references is not None:  # P pictures with reference lists over the pool (InterPictureParams(..., references=InterReferences)): kvz_hip_dev_inter_ctu_pass_refs
            if self._n_list_sets:
                raise ValueError("scaling lists are set: kvz_hip_dev_inter_ctu_pass_lists has no reference lists (clear_scaling_lists())")
            rc = self.lib.kvz_hip_dev_inter_ctu_pass_refs(self.d_src, self.d_ref, self.d_ref_cu, self.d_rec, self.d_cu, self.d_coeff, self.w, self.h, self.n, C.addressof(params), None, 0,
                                                          pictures.ptr if pictures is not None else None, slice_type_value(slice_type), references.ptr)
            if rc != 0:
                raise RuntimeError(f"kvz_hip_dev_inter_ctu_pass_refs returned {rc}")
            return
        if slice_type != "B":
            if self._n_list_sets:
                raise ValueError("scaling lists are set: kvz_hip_dev_inter_ctu_pass_lists has no slice type, its pictures are B (clear_scaling_lists())")
            rc = self.lib.kvz_hip_dev_inter_ctu_pass_slices(self.d_src, self.d_ref, self.d_ref_cu, self.d_rec, self.d_cu, self.d_coeff, self.w, self.h, self.n, C.addressof(params), None, 0,
                                                            pictures.ptr if pictures is not None else None, slice_type_value(slice_type))
            if rc != 0:
                raise RuntimeError(f"kvz_hip_dev_inter_ctu_pass_slices returned {rc}")
            return
        if self._n_list_sets:
            rc = self.lib.kvz_hip_dev_inter_ctu_pass_lists(self.d_src, self.d_ref, self.d_ref_cu, self.d_rec, self.d_cu, self.d_coeff, self.w, self.h, self.n, C.addressof(params), None, 0,
                                                           pictures.ptr if pictures is not None else None, C.addressof(self._list_sets), self._n_list_sets,
                                                           C.addressof(self._list_index) if self._list_index is not None else None)
            if rc != 0:
                raise RuntimeError(f"kvz_hip_dev_inter_ctu_pass_lists returned {rc}")
            return
        if pictures is not None:
            rc = self.lib.kvz_hip_dev_inter_ctu_pass_pictures(self.d_src, self.d_ref, self.d_ref_cu, self.d_rec, self.d_cu, self.d_coeff, self.w, self.h, self.n, C.addressof(params), None, 0,
                                                              pictures.ptr)
            if rc != 0:
                raise RuntimeError(f"kvz_hip_dev_inter_ctu_pass_pictures returned {rc}")
            return
        rc = self.lib.kvz_hip_dev_inter_ctu_pass(self.d_src, self.d_ref, self.d_ref_cu, self.d_rec, self.d_cu, self.d_coeff, self.w, self.h, self.n, C.addressof(params))
        if rc != 0:
            raise RuntimeError(f"kvz_hip_dev_inter_ctu_pass returned {rc}")

    def upload_source(self, i, src):
        a = np.ascontiguousarray(src)
        assert a.nbytes == self.fs
        self.lib.kvz_hip_dev_upload(self.d_src + i * self.fs, a.ctypes.data, self.fs)

    def new_source_set(self):
        """another resident set of n source pictures (the next picture of every sequence); returns the handle use_source_set() takes"""
        self._source_sets = getattr(self, "_source_sets", [self.d_src])
        self._source_sets.append(self.dev.empty(self.n * self.fs))
        return len(self._source_sets) - 1

    def use_source_set(self, k):
        self._source_sets = getattr(self, "_source_sets", [self.d_src])
        self.d_src = self._source_sets[k]

    def loop_filters(self, params, slice_is_b=True, pictures=None, slice_type=None):
        """deblocking and SAO of the pictures the pass just produced, in place (kvz_hip_dev_loop_filters_inter): d_rec becomes what the next picture predicts from.
        pictures (InterPictureParams): every picture at its own QP (kvz_hip_dev_loop_filters_inter_pictures).
        slice_type: None (slice_is_b says it, as it always has: B, or the I slice's rules) or "B" / "P" / "I" through kvz_hip_dev_loop_filters_inter_slices"""
        if self.d_dbk is None:
            self.d_dbk = self.dev.empty(self.n * self.cells * 20)  # kvz_hip_cu_dbk
        self.lib.kvz_hip_dev_cu_dbk_from_info(self.d_cu, self.n * self.cells, self.d_dbk)
        references = getattr(pictures, "references", None)
        if references is not None:  # kvz_hip_dev_loop_filters_inter_refs: the table is checked, the filters are the slice type's
            if pictures is not None and len(pictures) != self.n:
                raise ValueError(f"{len(pictures)} picture QPs for {self.n} pictures")
            rc = self.lib.kvz_hip_dev_loop_filters_inter_refs(self.d_src, self.d_rec, self.w, self.h, self.n, self.d_dbk, params.qp, pictures.qps.ctypes.data if pictures is not None else None,
                                                              slice_type_value("P" if slice_type is None else slice_type), params.deblock, 0, 0, params.sao, params.no_wpp, None, None, None, references.ptr)
            if rc != 0:
                raise RuntimeError(f"kvz_hip_dev_loop_filters_inter_refs returned {rc}")
            return
        if slice_type is not None:
            if pictures is not None and len(pictures) != self.n:
                raise ValueError(f"{len(pictures)} picture QPs for {self.n} pictures")
            rc = self.lib.kvz_hip_dev_loop_filters_inter_slices(self.d_src, self.d_rec, self.w, self.h, self.n, self.d_dbk, params.qp, pictures.qps.ctypes.data if pictures is not None else None,
                                                                slice_type_value(slice_type), params.deblock, 0, 0, params.sao, params.no_wpp, None, None, None)
            if rc != 0:
                raise RuntimeError(f"kvz_hip_dev_loop_filters_inter_slices returned {rc}")
            return
        if pictures is not None:
            if len(pictures) != self.n:
                raise ValueError(f"{len(pictures)} picture QPs for {self.n} pictures")
            rc = self.lib.kvz_hip_dev_loop_filters_inter_pictures(self.d_src, self.d_rec, self.w, self.h, self.n, self.d_dbk, pictures.qps.ctypes.data, int(slice_is_b), params.deblock, 0, 0,
                                                                  params.sao, params.no_wpp, None, None, None)
            if rc != 0:
                raise RuntimeError(f"kvz_hip_dev_loop_filters_inter_pictures returned {rc}")
            return
        rc = self.lib.kvz_hip_dev_loop_filters_inter(self.d_src, self.d_rec, self.w, self.h, self.n, self.d_dbk, params.qp, int(slice_is_b), params.deblock, 0, 0, params.sao,
                                                     params.no_wpp, None, None, None)
        if rc != 0:
            raise RuntimeError(f"kvz_hip_dev_loop_filters_inter returned {rc}")

    def entropy_code(self, params, pictures=None, slice_type="B"):
        """kvz_hip_dev_entropy_code_inter: the slice data of the pictures the pass just produced (after loop_filters when params.sao: their SAO decisions are coded).
        pictures (InterPictureParams): every picture at its own QP and POC (kvz_hip_dev_entropy_code_inter_pictures).
        slice_type: "B" (the default: the calls this method has always made) or "P" through kvz_hip_dev_entropy_code_inter_slices.
        -> (bytes of all substreams back to back, sizes [sequence][substream])"""
        if self.d_coeff is None:
            raise RuntimeError("InterPictures(..., with_levels=True) keeps the levels the entropy coder needs")
        rows = 1 if params.no_wpp else (self.h + 63) // 64
        from .batch import entropy_capacity
        capacity = entropy_capacity(self.n, self.w, self.h)
        if self._entropy_out is None:
            from .batch import pinned_bytes
            self._entropy_ptr, self._entropy_out = pinned_bytes(self.lib, capacity)  # pinned: the call downloads the slice data straight into it
        sizes = np.zeros((self.n, rows), np.uint32)
        references = getattr(pictures, "references", None)
        if references is not None:  # the pool's records are the reference records: the co-located picture of a picture is the frame of its list's first entry
            total = self.lib.kvz_hip_dev_entropy_code_inter_refs(self.d_cu, self.d_ref_cu, self.d_coeff, self.w, self.h, self.n, C.addressof(params), self._entropy_out.ctypes.data,
                                                                 capacity, sizes.ctypes.data, pictures.ptr if pictures is not None else None, slice_type_value(slice_type), references.ptr)
        elif slice_type != "B":
            total = self.lib.kvz_hip_dev_entropy_code_inter_slices(self.d_cu, self.d_ref_cu, self.d_coeff, self.w, self.h, self.n, C.addressof(params), self._entropy_out.ctypes.data,
                                                                   capacity, sizes.ctypes.data, pictures.ptr if pictures is not None else None, slice_type_value(slice_type))
        elif pictures is not None:
            total = self.lib.kvz_hip_dev_entropy_code_inter_pictures(self.d_cu, self.d_ref_cu, self.d_coeff, self.w, self.h, self.n, C.addressof(params), self._entropy_out.ctypes.data,
                                                                     capacity, sizes.ctypes.data, pictures.ptr)
        else:
            total = self.lib.kvz_hip_dev_entropy_code_inter(self.d_cu, self.d_ref_cu, self.d_coeff, self.w, self.h, self.n, C.addressof(params), self._entropy_out.ctypes.data,
                                                            capacity, sizes.ctypes.data)
        if total < 0:
            raise RuntimeError("kvz_hip_dev_entropy_code_inter failed")
        return self._entropy_out[:total], sizes

    def sse(self):
        """-> uint64 array [n][3]: the exact sum of squared differences of the current source set against d_rec as it stands, Y, U, V (kvz_hip_dev_picture_sse).
        After loop_filters() it is the distortion of the final picture, the one kvazaar's PSNR is of; call it before advance(), which swaps d_rec away"""
        f = self.lib.kvz_hip_dev_picture_sse
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        d_out = self.dev.empty(self.n * 24)
        try:
            if f(self.d_src, self.d_rec, self.w, self.h, self.n, d_out) != 0:
                raise RuntimeError("kvz_hip_dev_picture_sse: bad argument")
            return self.dev.get(d_out, (self.n, 3), np.uint64)
        finally:
            self.dev.free(d_out)

    def psnr(self):
        """-> float64 array [n][3]: PSNR Y, U, V of the pictures just encoded as kvazaar computes it"""
        from .batch import psnr_of_planes
        return psnr_of_planes(self.lib, self.sse(), self.w, self.h)

    def advance(self):
        """the pictures just encoded (after their loop filters) and their CU records become the references of the next picture"""
        self.d_ref, self.d_rec = self.d_rec, self.d_ref
        self.d_ref_cu, self.d_cu = self.d_cu, self.d_ref_cu

    def sync(self):
        self.lib.kvz_hip_dev_sync()

    def download(self, i):
        rec, cu = np.empty(self.fs, np.uint8), np.empty((self.h // 4, self.w // 4), CU_DTYPE)
        self.lib.kvz_hip_dev_download(rec.ctypes.data, self.d_rec + i * self.fs, self.fs)
        self.lib.kvz_hip_dev_download(cu.ctypes.data, self.d_cu + i * self.cells * CU_DTYPE.itemsize, cu.nbytes)
        return rec, cu

    def close(self):
        self.dev.free(self.d_ref, self.d_rec, self.d_ref_cu, self.d_cu, *getattr(self, "_source_sets", [self.d_src]))
        if self.d_dbk is not None:
            self.dev.free(self.d_dbk)
        if self.d_coeff is not None:
            self.dev.free(self.d_coeff)
        if getattr(self, "_entropy_ptr", None):
            from .batch import pinned_free
            pinned_free(self.lib, self._entropy_ptr)
            self._entropy_ptr = self._entropy_out = None


class InterGroupStruct(C.Structure):  # kvz_hip_inter_group
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("n_pictures", C.c_int32)] + [(n, C.c_void_p) for n in ("src", "ref", "ref_cu", "rec", "cu", "coeff", "pictures")]


class InterGroup:
    """InterPictures objects of different sizes whose CTU passes run as ONE launch (kvz_hip_dev_inter_ctu_pass_groups): the persistent workgroups draw the CTUs of all
    members, instead of one partly empty launch per size.  The members stay what they are: after run() each member's rec / cu / coeff hold what member.run(...)
    would have made them, and its loop_filters, entropy_code, sse, advance and download work unchanged.  Scaling lists are not part of joint launches."""

    def __init__(self, lib, members):
        self.lib, self.members = lib, list(members)
        if not self.members:
            raise ValueError("an InterGroup needs at least one InterPictures member")
        lib.kvz_hip_dev_inter_ctu_pass_groups.restype = C.c_int
        lib.kvz_hip_dev_inter_ctu_pass_groups.argtypes = [C.c_void_p, C.c_int, C.c_void_p]

    def structs(self, pictures=None):
        """the kvz_hip_inter_group array of the members as they stand now (their buffers swap on advance() / use_source_set())"""
        pictures = [None] * len(self.members) if pictures is None else list(pictures)
        if len(pictures) != len(self.members):
            raise ValueError(f"{len(pictures)} picture tables for {len(self.members)} members")
        arr = (InterGroupStruct * len(self.members))()
        for g, m, t in zip(arr, self.members, pictures):
            g.struct_size, g.width, g.height, g.n_pictures = C.sizeof(InterGroupStruct), m.w, m.h, m.n
            g.src, g.ref, g.ref_cu, g.rec, g.cu, g.coeff = m.d_src, m.d_ref, m.d_ref_cu, m.d_rec, m.d_cu, m.d_coeff
            g.pictures = t.ptr if t is not None else None
        return arr

    def run(self, params, pictures=None):
        """the CTU pass of every member's pictures in one launch.  pictures: one InterPictureParams, or None (params.qp / params.poc), per member.  Returns the
        pass's code: 0, -1 for a refused launch (see stderr; nothing was queued), -2 for a hand-off time-out"""
        for i, m in enumerate(self.members):
            if m._n_list_sets:
                raise ValueError(f"member {i} has scaling lists set: they are not part of joint launches (clear_scaling_lists(), or run the member on its own)")
        arr = self.structs(pictures)  # (pictures' arrays live as long as the caller's objects; arr as long as this call)
        return int(self.lib.kvz_hip_dev_inter_ctu_pass_groups(C.addressof(arr), len(self.members), C.addressof(params)))

    def close(self):
        """forgets the members; they stay open"""
        self.members = []


class TiledInterSequences:
    """BASELINE config 4 sharded by tile: picture k of `n` independent sequences of a width x height frame cut into kvazaar's uniform --tiles grid.  This rank's
    tiles are resident as pictures of their own (source, reconstruction, CU records: the tile is an independent sub-picture for prediction, neighbours, contexts and loop
    filters); the REFERENCE frames and their CU records are whole frames on every rank -- motion vectors leave the tile --, rebuilt after every picture by THE collective of the
    configuration: one all-gather of the ranks' filtered tiles (RCCL over xGMI when world > 1) and a paste, and the same for the CU records.
    Buffers are torch tensors (the collective is torch.distributed's); the passes run through the C ABI on the library's stream of this thread."""

    def __init__(self, lib, width, height, cols, rows, n, rank=0, world=1, dist=None, device="cuda"):
        import torch
        from . import sharding
        self.lib, self.w, self.h, self.n, self.rank, self.world, self.dist, self.torch = lib, width, height, n, rank, world, dist, torch
        self.plan = sharding.exchange_plan(width, height, cols, rows, world)
        self.tiles = self.plan["tiles"]
        self.mine = sharding.tiles_of_rank(len(self.tiles), rank, world)
        self.per_rank = self.plan["slots_per_rank"]
        self.fs, self.cells = width * height * 3 // 2, (width // 4) * (height // 4)
        self.rec_item = CU_DTYPE.itemsize
        dev = torch.device(device)
        e = lambda nbytes: torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.ref, self.ref_cu = e(n * self.fs), e(n * self.cells * self.rec_item)
        self.slot_px = max(t[2] * t[3] * 3 // 2 for t in self.tiles)
        self.slot_cu = max((t[2] // 4) * (t[3] // 4) for t in self.tiles) * self.rec_item
        # send / receive buffers of the two all-gathers: [slot of the rank][sequence][bytes of the largest tile]
        self.send_px, self.send_cu = torch.zeros(self.per_rank * n * self.slot_px, dtype=torch.uint8, device=dev), torch.zeros(self.per_rank * n * self.slot_cu, dtype=torch.uint8, device=dev)
        self.recv_px = e(world * self.per_rank * n * self.slot_px) if world > 1 else self.send_px
        self.recv_cu = e(world * self.per_rank * n * self.slot_cu) if world > 1 else self.send_cu
        # this rank's tiles grouped by size: one launch of the pass (and of the loop filters) per group, picture j * n + i = tile j of the group, sequence i
        self.groups = {}
        for ti in self.mine:
            self.groups.setdefault((self.tiles[ti][2], self.tiles[ti][3]), []).append(ti)
        self.src, self.rec, self.cu, self.dbk, self.xy = {}, {}, {}, {}, {}
        for (tw, th), members in self.groups.items():
            m = len(members) * n
            self.src[(tw, th)], self.rec[(tw, th)] = e(m * tw * th * 3 // 2), e(m * tw * th * 3 // 2)
            self.cu[(tw, th)], self.dbk[(tw, th)] = e(m * (tw // 4) * (th // 4) * self.rec_item), e(m * (tw // 4) * (th // 4) * 20)
            xy = np.array([[self.tiles[ti][0], self.tiles[ti][1]] for ti in members for _ in range(n)], np.int32)
            self.xy[(tw, th)] = torch.from_numpy(xy).to(dev)
        lib.kvz_hip_dev_inter_ctu_pass_tiles.restype = C.c_int
        lib.kvz_hip_dev_inter_ctu_pass_tiles.argtypes = [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p, C.c_int]
        lib.kvz_hip_dev_cu_dbk_from_info.restype = None
        lib.kvz_hip_dev_cu_dbk_from_info.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.kvz_hip_dev_loop_filters_inter.restype = C.c_int
        lib.kvz_hip_dev_loop_filters_inter.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 3
        self.ctus = sum(((self.tiles[ti][2] + 63) // 64) * ((self.tiles[ti][3] + 63) // 64) for ti in self.mine)  # of this rank, per sequence
        self.pass_ms = 0.0

    def group_params(self, base):
        return InterParams(qp=base.qp, poc=base.poc, mv_constraint=0, sao=base.sao, deblock=base.deblock, fme_level=base.fme_level, pu_depth_inter_max=base.pu_depth_inter_max,
                           no_wpp=1, fast_residual_cost=base.fast_residual_cost, ref_width=self.w, ref_height=self.h, tile_x=0, tile_y=0, no_tmvp=1)  # tiles: --no-wpp, no TMVP (cfg.c:920-975)

    def upload_sources(self, frames_of_sequence):
        """frames_of_sequence(i) -> the planar frame of sequence i for the picture about to be encoded; every tile of this rank gets its part"""
        from . import sharding
        torch = self.torch
        for (tw, th), members in self.groups.items():
            ts = tw * th * 3 // 2
            host = np.empty((len(members), self.n, ts), np.uint8)
            for j, ti in enumerate(members):
                cache = {}
                for i in range(self.n):
                    f = frames_of_sequence(i)
                    k = id(f)
                    if k not in cache:
                        cache[k] = sharding.crop_tile(f, self.w, self.h, self.tiles[ti])
                    host[j, i] = cache[k]
            self.src[(tw, th)].copy_(torch.from_numpy(host).reshape(-1))

    def set_reference(self, frames, cu):
        """whole reference frames [n, fs] and their CU records [n, h/4, w/4] (host arrays): the start of a chain"""
        torch = self.torch
        self.ref.copy_(torch.from_numpy(np.ascontiguousarray(frames).reshape(-1)))
        self.ref_cu.copy_(torch.from_numpy(np.ascontiguousarray(cu).view(np.uint8).reshape(-1)))

    def save_reference(self):
        """keep a device copy of the reference frames and their CU records as they are now (restore_reference puts them back: a bench step that codes the same picture again)"""
        self._saved = (self.ref.clone(), self.ref_cu.clone())

    def restore_reference(self):
        self.ref.copy_(self._saved[0])
        self.ref_cu.copy_(self._saved[1])

    def run_picture(self, base):
        """one B picture of every sequence: the CTU pass of this rank's tiles, their loop filters, then the exchange that turns the result into the next picture's reference"""
        torch = self.torch
        torch.cuda.synchronize()
        self.lib.kvz_hip_dev_inter_kernel_ms.restype = C.c_float
        prm = self.group_params(base)

        def group_pass(g, members, parts=1):
            tw, th = g
            m = len(members) * self.n
            self.lib.kvz_hip_dev_inter_set_share(parts)  # per calling thread: this pass's share of the workgroup slots (the pool's threads stay alive)
            rc = self.lib.kvz_hip_dev_inter_ctu_pass_tiles(self.src[g].data_ptr(), self.ref.data_ptr(), self.ref_cu.data_ptr(), self.rec[g].data_ptr(), self.cu[g].data_ptr(), None, tw, th,
                                                           m, C.addressof(prm), self.xy[g].data_ptr(), self.n)
            if rc != 0:
                raise RuntimeError(f"kvz_hip_dev_inter_ctu_pass_tiles returned {rc}")
            ms = float(self.lib.kvz_hip_dev_inter_kernel_ms())
            self.lib.kvz_hip_dev_cu_dbk_from_info(self.cu[g].data_ptr(), m * (tw // 4) * (th // 4), self.dbk[g].data_ptr())
            rc = self.lib.kvz_hip_dev_loop_filters_inter(self.src[g].data_ptr(), self.rec[g].data_ptr(), tw, th, m, self.dbk[g].data_ptr(), prm.qp, 1, prm.deblock, 0, 0, prm.sao, 1, None, None, None)
            if rc != 0:
                raise RuntimeError(f"kvz_hip_dev_loop_filters_inter returned {rc}")
            self.lib.kvz_hip_dev_sync()  # this thread's stream of the library
            return ms
        groups = list(self.groups.items())
        if len(groups) > 1:
            # kvazaar's uniform grid gives this rank tiles of two sizes: their passes are two persistent launches, and the first one launched fills the device while
            # each holds fewer serial tile chains than the device has workgroup slots.  So: side by side, each on its share of the slots (kvz_hip_dev_inter_set_share), from
            # two host threads -- a thread has its own stream and scratch in the library, and the blocking calls release the GIL.
            if getattr(self, "_pool", None) is None:
                from concurrent.futures import ThreadPoolExecutor
                self._pool = ThreadPoolExecutor(max_workers=len(groups))
            self.pass_ms = max(f.result() for f in [self._pool.submit(group_pass, g, mem, len(groups)) for g, mem in groups])
        else:
            self.pass_ms = sum(group_pass(g, mem) for g, mem in groups)
        self.exchange()

    def slots_per_cu(self):
        """workgroups of the inter pass's kernel that fit a CU (kvz_hip_dev_inter_slots_per_cu: its occupancy; 12 with the round-4 build)"""
        self.lib.kvz_hip_dev_inter_slots_per_cu.restype = C.c_int
        return int(self.lib.kvz_hip_dev_inter_slots_per_cu())

    def exchange(self):
        """all-gather of the tiles' pictures and CU records, pasted into every rank's reference frames"""
        torch = self.torch
        n = self.n
        slot_of = {ti: k for k, ti in enumerate(self.mine)}
        for (tw, th), members in self.groups.items():
            ts, tc = tw * th * 3 // 2, (tw // 4) * (th // 4) * self.rec_item
            for j, ti in enumerate(members):
                self.send_px.view(self.per_rank, n, self.slot_px)[slot_of[ti], :, :ts] = self.rec[(tw, th)].view(len(members), n, ts)[j]
                self.send_cu.view(self.per_rank, n, self.slot_cu)[slot_of[ti], :, :tc] = self.cu[(tw, th)].view(len(members), n, tc)[j]
        if self.world > 1:
            self.dist.all_gather_into_tensor(self.recv_px, self.send_px)
            self.dist.all_gather_into_tensor(self.recv_cu, self.send_cu)
        from . import sharding
        ys, cs = self.w * self.h, (self.w // 2) * (self.h // 2)
        fr = self.ref.view(n, self.fs)
        Y, U, V = fr[:, :ys].view(n, self.h, self.w), fr[:, ys:ys + cs].view(n, self.h // 2, self.w // 2), fr[:, ys + cs:].view(n, self.h // 2, self.w // 2)
        CU = self.ref_cu.view(n, self.h // 4, self.w // 4, self.rec_item)
        px, cu = self.recv_px.view(self.world, self.per_rank, n, self.slot_px), self.recv_cu.view(self.world, self.per_rank, n, self.slot_cu)
        for r in range(self.world):
            for k, ti in enumerate(sharding.tiles_of_rank(len(self.tiles), r, self.world)):
                x, y, tw, th = self.tiles[ti]
                c = (tw // 2) * (th // 2)
                t = px[r, k]
                Y[:, y:y + th, x:x + tw] = t[:, :tw * th].view(n, th, tw)
                U[:, y // 2:(y + th) // 2, x // 2:(x + tw) // 2] = t[:, tw * th:tw * th + c].view(n, th // 2, tw // 2)
                V[:, y // 2:(y + th) // 2, x // 2:(x + tw) // 2] = t[:, tw * th + c:tw * th + 2 * c].view(n, th // 2, tw // 2)
                CU[:, y // 4:(y + th) // 4, x // 4:(x + tw) // 4] = cu[r, k][:, :(tw // 4) * (th // 4) * self.rec_item].view(n, th // 4, tw // 4, self.rec_item)
        torch.cuda.synchronize()

    def download_reference(self, i):
        """the assembled frame and CU records of sequence i after the last exchange"""
        frame = self.ref.view(self.n, self.fs)[i].cpu().numpy().copy()
        cu = self.ref_cu.view(self.n, self.cells * self.rec_item)[i].cpu().numpy().copy().view(CU_DTYPE).reshape(self.h // 4, self.w // 4)
        return frame, cu
