"""ctypes view of include/kvz_hip_batch.h: the batched, device-resident all-intra CTU pass (kvz_hip_intra_frames) and what follows
it per picture (deblocking, picture hashes).  Used by bench.py, __graft_entry__.smoke(), tools/ and the GPU tests; no checker code
in here (the oracle runners are in tests/ctu_common.py)."""
import ctypes as C

import numpy as np

from .capi import i16p, ptr, u8p


class CostModel(C.Structure):
    """kvz_hip_intra_cost_model (include/kvz_hip_types.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("lambda_", C.c_double), ("lambda_sqrt", C.c_double), ("split_flag", (C.c_float * 2) * 3),
                ("part_size", C.c_float * 2), ("intra_mode", C.c_float * 2), ("chroma_mode", C.c_float * 2),
                ("cbf_luma", (C.c_float * 2) * 2), ("cbf_chroma", (C.c_float * 2) * 2), ("coeff_weights", C.c_uint64),
                ("qp", C.c_int32), ("adaptive", C.c_int32), ("coeff_cabac", C.c_int32), ("no_wpp", C.c_int32), ("search_32x32", C.c_int32), ("rdoq", C.c_int32), ("search_nxn", C.c_int32), ("ctx_init", C.c_uint8 * 160),
                ("entropy_fbits", C.c_float * 128), ("signhide", C.c_int32)]

    def key(self):
        return bytes(self)


def default_coeff_weights(lib, qp):
    """kvz_fast_coeff_get_weights of kvazaar's built-in table (kvz_hip_default_coeff_weights)"""
    lib.kvz_hip_default_coeff_weights.restype = C.c_uint64
    lib.kvz_hip_default_coeff_weights.argtypes = [C.c_int]
    return int(lib.kvz_hip_default_coeff_weights(qp))


def cost_model(lib, qp, weights=None):
    """kvz_hip_intra_cost_model_init: the model of an I slice at `qp` as `kvazaar --preset ultrafast` sets it up"""
    m = CostModel()
    lib.kvz_hip_intra_cost_model_init.argtypes = [C.c_int, C.c_uint64, C.POINTER(CostModel)]
    lib.kvz_hip_intra_cost_model_init.restype = None
    lib.kvz_hip_intra_cost_model_init(qp, default_coeff_weights(lib, qp) if weights is None else weights, C.byref(m))
    return m


class PictureModelsStruct(C.Structure):
    """kvz_hip_picture_models (include/kvz_hip_types.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("n_models", C.c_int32), ("models", C.POINTER(CostModel)), ("model_of_picture", C.POINTER(C.c_uint16))]


class PictureModels:
    """A cost model per picture of a batch (kvz_hip_picture_models): pictures of streams at different QPs in one launch.  qps: the QP of every picture of the batch, in
    order; the table holds one model per distinct QP.  weights: fast-coefficient-cost weights for every QP (an int), per QP (a dict or a callable), or None for kvazaar's
    built-in table.  switches: CostModel fields set on every model (adaptive, no_wpp, search_32x32, rdoq, search_nxn, coeff_cabac, signhide) -- the first five must be the
    same for all models of a table, which this guarantees.  signhide may also be a sequence with a value per picture (sign data hiding for some streams of the batch):
    the table then holds a model per distinct (QP, signhide).  HipBatch.launch / run / loop_filters / entropy_code take it wherever they take a CostModel.  The object owns the ctypes
    arrays the struct points into: keep it alive while a call uses it."""

    def __init__(self, lib, qps, weights=None, extra_qps=(), **switches):
        """extra_qps: QPs the table also gets a row for although no picture runs at them (CtuModels: the QPs of CTUs)"""
        qps = [int(q) for q in qps]
        if not qps:
            raise ValueError("PictureModels: no pictures")
        self.qps = qps
        hide = switches.pop("signhide", 0)
        hide = [int(bool(v)) for v in hide] if isinstance(hide, (list, tuple, np.ndarray)) else [int(bool(hide))] * len(qps)
        if len(hide) != len(qps):
            raise ValueError("PictureModels: signhide per picture needs a value for every picture")
        self.signhide = hide
        distinct = sorted(set(zip(qps, hide)) | {(int(q), 0) for q in extra_qps})
        row = self.row = {k: i for i, k in enumerate(distinct)}
        self.models = (CostModel * len(distinct))()
        for i, (q, sh) in enumerate(distinct):
            w = weights(q) if callable(weights) else (weights[q] if isinstance(weights, dict) else weights)
            m = cost_model(lib, q, w)
            for k, v in switches.items():
                if k not in ("adaptive", "no_wpp", "search_32x32", "rdoq", "search_nxn", "coeff_cabac"):
                    raise TypeError(f"PictureModels: {k} is not a switch of the cost model")
                setattr(m, k, int(v))
            m.signhide = sh
            self.models[i] = m
        self.index = (C.c_uint16 * len(qps))(*[row[k] for k in zip(qps, hide)])
        self.struct = PictureModelsStruct(C.sizeof(PictureModelsStruct), len(distinct), self.models, self.index)

    def model_of(self, picture):
        """the CostModel picture `picture` runs under"""
        return self.models[self.index[picture]]

    # what HipBatch reads of a model, table or not
    @property
    def no_wpp(self):
        return self.models[0].no_wpp

    def __len__(self):
        return len(self.qps)


class CtuModelsStruct(C.Structure):
    """kvz_hip_ctu_models (include/kvz_hip_types.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("pictures", C.POINTER(PictureModelsStruct)), ("model_of_ctu", C.POINTER(C.c_uint16))]


class CtuModels:
    """A cost model per CTU of a batch (kvz_hip_ctu_models): a QP per CTU inside a picture, HEVC's cu_qp_delta with one quantisation group per CTU -- what kvazaar's
    --roi / --vaq / rate control set per LCU.  picture_qps: the slice QP of every picture of the batch; ctu_qps: per picture the QP of every CTU in raster order (CTU
    rows x CTU columns).  The table (`pictures`, a PictureModels) holds one model per distinct QP; weights and switches as PictureModels takes them, without signhide,
    rdoq and search_nxn.  The slice QP and the CTU QPs of one picture may span at most 25.  HipBatch.launch / run / loop_filters / entropy_code take it wherever they take a
    PictureModels.  The object owns the ctypes arrays the struct points into: keep it alive while a call uses it."""

    def __init__(self, lib, picture_qps, ctu_qps, weights=None, **switches):
        for k in ("signhide", "rdoq", "search_nxn"):
            if switches.get(k):
                raise TypeError(f"CtuModels: {k} is not supported with a model per CTU")
        ctu_qps = [[int(q) for q in np.asarray(p).reshape(-1)] for p in ctu_qps]
        if len(ctu_qps) != len(picture_qps) or len({len(p) for p in ctu_qps}) > 1:
            raise ValueError("CtuModels: ctu_qps needs the QP of every CTU of every picture")
        self.ctu_qps = ctu_qps
        self.pictures = PictureModels(lib, picture_qps, weights, extra_qps={q for p in ctu_qps for q in p}, **switches)
        flat = [self.pictures.row[(q, 0)] for p in ctu_qps for q in p]
        self.index = (C.c_uint16 * max(len(flat), 1))(*flat)
        self.struct = CtuModelsStruct(C.sizeof(CtuModelsStruct), C.pointer(self.pictures.struct), self.index)

    @property
    def no_wpp(self):
        return self.pictures.no_wpp

    def __len__(self):
        return len(self.pictures)


class ScalingListsStruct(C.Structure):
    """kvz_hip_scaling_lists (include/kvz_hip_types.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("coeff", ((C.c_int32 * 64) * 6) * 4), ("dc", (C.c_int32 * 6) * 4)]


class ScalingLists:
    """One set of per-coefficient scaling lists (kvz_hip_scaling_lists; kvazaar's --scaling-list / --cqmfile): coeff [4][6][64] as the encoder holds
    scaling_list_coeff[size_id][list_id] (16 entries at 4x4, 64 above, raster order, 13 .. 255), dc [4][6] (0 = 16).  HipBatch.set_scaling_lists takes a sequence of them."""

    def __init__(self, coeff, dc=None):
        self.struct = ScalingListsStruct()
        self.struct.struct_size = C.sizeof(ScalingListsStruct)
        self.coeff = np.ascontiguousarray(coeff, np.int32).reshape(4, 6, 64)
        self.dc = np.zeros((4, 6), np.int32) if dc is None else np.ascontiguousarray(dc, np.int32).reshape(4, 6)
        C.memmove(self.struct.coeff, self.coeff.ctypes.data, self.coeff.nbytes)
        C.memmove(self.struct.dc, self.dc.ctypes.data, self.dc.nbytes)

    @classmethod
    def default(cls, lib):
        """--scaling-list default (kvz_hip_scaling_lists_default): H.265 tables 7-5 / 7-6, DC 16"""
        st = ScalingListsStruct()
        lib.kvz_hip_scaling_lists_default.argtypes = [C.POINTER(ScalingListsStruct)]
        lib.kvz_hip_scaling_lists_default.restype = None
        lib.kvz_hip_scaling_lists_default(C.byref(st))
        return cls(np.ctypeslib.as_array(st.coeff), np.ctypeslib.as_array(st.dc))


def _is_table(model):
    return isinstance(model, PictureModels)


def _is_ctu_map(model):
    return isinstance(model, CtuModels)


def outputs(width, height):
    """host arrays of one picture's results: reconstruction Y|U|V, coefficients, CU depth / intra mode per 8x8, CTU costs"""
    nctu = ((width + 63) // 64) * ((height + 63) // 64)
    ncu = (width // 8) * (height // 8)
    return dict(rec=np.zeros(width * height * 3 // 2, np.uint8), coeff=np.zeros(nctu * 6144, np.int16),
                depth=np.zeros(ncu, np.uint8), mode=np.zeros(ncu, np.uint8), cost=np.zeros(nctu, np.float64))


class BatchError(RuntimeError):
    """a pass of the batch was invalid (kvz_hip_batch_sync returned -1)"""


class HipBatch:
    """kvz_hip_batch_* through ctypes"""

    def __init__(self, lib, width, height, n_frames, device=-1):
        """device: kvz_hip_batch_create_on -- -1 = the calling thread's current device (the process default unless the thread chose another)"""
        self.lib, self.w, self.h, self.n = lib, width, height, n_frames
        vp, ci = C.c_void_p, C.c_int
        lib.kvz_hip_batch_create.restype = vp
        lib.kvz_hip_batch_create.argtypes = [ci, ci, ci]
        lib.kvz_hip_batch_destroy.argtypes = [vp]
        lib.kvz_hip_batch_destroy.restype = None
        lib.kvz_hip_batch_upload.argtypes = [vp, ci, u8p, u8p, u8p]
        lib.kvz_hip_batch_upload.restype = None
        lib.kvz_hip_batch_download.argtypes = [vp, ci, u8p, u8p, u8p, i16p, u8p, u8p, C.POINTER(C.c_double)]
        lib.kvz_hip_batch_download.restype = ci
        lib.kvz_hip_intra_frames.argtypes = [vp, C.POINTER(CostModel)]
        lib.kvz_hip_intra_frames.restype = ci
        lib.kvz_hip_batch_sync.argtypes = [vp]
        lib.kvz_hip_batch_sync.restype = ci
        lib.kvz_hip_batch_reset.argtypes = [vp]
        lib.kvz_hip_batch_reset.restype = ci
        lib.kvz_hip_batch_last_kernel_ms.argtypes = [vp]
        lib.kvz_hip_batch_last_kernel_ms.restype = C.c_float
        lib.kvz_hip_batch_ctus_per_frame.argtypes = [vp]
        lib.kvz_hip_batch_ctus_per_frame.restype = ci
        lib.kvz_hip_batch_deblock.argtypes = [vp, ci, ci, ci]
        lib.kvz_hip_batch_deblock.restype = None
        lib.kvz_hip_batch_checksums.argtypes = [vp, vp]
        lib.kvz_hip_batch_checksums.restype = ci
        lib.kvz_hip_batch_create_on.restype = vp
        lib.kvz_hip_batch_create_on.argtypes = [ci, ci, ci, ci]
        self.handle = lib.kvz_hip_batch_create_on(device, width, height, n_frames)
        if not self.handle:
            raise RuntimeError(f"kvz_hip_batch_create_on({device}, {width}, {height}, {n_frames}) failed")
        self.ctus_per_frame = lib.kvz_hip_batch_ctus_per_frame(self.handle)

    def upload(self, frame, yuv):
        ys, cs = self.w * self.h, self.w * self.h // 4
        self.lib.kvz_hip_batch_upload(self.handle, frame, ptr(yuv), ptr(yuv, offset=ys), ptr(yuv, offset=ys + cs))

    def upload_all_async(self, src_ptr):
        """kvz_hip_batch_upload_all_async: all n pictures (back to back, Y | U | V each) from host memory at address `src_ptr` -- pinned_bytes() -- on the batch's upload
        queue; starts when the batch's last pass has ended, the next launch waits for it"""
        self.lib.kvz_hip_batch_upload_all_async.argtypes = [C.c_void_p, C.c_void_p]
        self.lib.kvz_hip_batch_upload_all_async.restype = None
        self.lib.kvz_hip_batch_upload_all_async(self.handle, src_ptr)

    def _check_table(self, models):
        if len(models) != self.n:
            raise ValueError(f"PictureModels of {len(models)} pictures for a batch of {self.n}")

    def launch(self, model):
        """asynchronous on the batch's stream; returns the number of kernel launches.  model: a CostModel for every picture, or a PictureModels table
        (kvz_hip_intra_frames_models), or a CtuModels map (kvz_hip_intra_frames_ctu_models: the pass, and behind it the QP of every CU)"""
        if _is_ctu_map(model):
            self._check_table(model)
            f = self.lib.kvz_hip_intra_frames_ctu_models
            f.argtypes = [C.c_void_p, C.POINTER(CtuModelsStruct)]
            f.restype = C.c_int
            return f(self.handle, C.byref(model.struct))
        if _is_table(model):
            self._check_table(model)
            f = self.lib.kvz_hip_intra_frames_models
            f.argtypes = [C.c_void_p, C.POINTER(PictureModelsStruct)]
            f.restype = C.c_int
            return f(self.handle, C.byref(model.struct))
        return self.lib.kvz_hip_intra_frames(self.handle, C.byref(model))

    def order_after(self, other):
        """later work of this batch starts after everything queued on `other` so far (kvz_hip_batch_order_after)"""
        self.lib.kvz_hip_batch_order_after.argtypes = [C.c_void_p, C.c_void_p]
        self.lib.kvz_hip_batch_order_after.restype = None
        self.lib.kvz_hip_batch_order_after(self.handle, other.handle)

    def set_device_share(self, num, den):
        """this batch's persistent pass takes num / den of the device's workgroup slots (kvz_hip_batch_set_device_share): batches of different geometry side by side"""
        self.lib.kvz_hip_batch_set_device_share.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self.lib.kvz_hip_batch_set_device_share.restype = None
        self.lib.kvz_hip_batch_set_device_share(self.handle, num, den)

    FLAT = 0xffff  # set_of_picture: the picture stays without lists

    def set_scaling_lists(self, sets, set_of_picture=None):
        """kvz_hip_batch_set_scaling_lists: the batch's later passes quantise picture i under sets[set_of_picture[i]] (HipBatch.FLAT: flat; None: every picture under
        sets[0]).  sets: a sequence of ScalingLists.  State of the batch until changed or cleared; raises BatchError when the library refuses (see stderr), and the
        previous state stays"""
        sets = list(sets)
        arr = (ScalingListsStruct * max(len(sets), 1))(*[s.struct for s in sets])
        index = None
        if set_of_picture is not None:
            if len(set_of_picture) != self.n:
                raise ValueError(f"set_of_picture of {len(set_of_picture)} pictures for a batch of {self.n}")
            index = (C.c_uint16 * self.n)(*[int(v) for v in set_of_picture])
        f = self.lib.kvz_hip_batch_set_scaling_lists
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        f.restype = C.c_int
        if f(self.handle, C.addressof(arr) if sets else None, len(sets), C.addressof(index) if index is not None else None) != 0:
            raise BatchError("kvz_hip_batch_set_scaling_lists: refused (see stderr)")

    def clear_scaling_lists(self):
        """the batch is again what it was before the first set_scaling_lists"""
        self.set_scaling_lists([])

    def sync(self):
        if self.lib.kvz_hip_batch_sync(self.handle) != 0:
            raise BatchError("kvz_hip_batch_sync: a CTU hand-off wait timed out; results invalid")

    def reset(self):
        """after a BatchError: drains the batch's stream and clears the (sticky) error word -- the batch can run again (kvz_hip_batch_reset)"""
        self.lib.kvz_hip_batch_reset(self.handle)

    def run(self, model):
        n = self.launch(model)
        if n < 0:
            raise BatchError("kvz_hip_intra_frames: the batch cannot run this model (see stderr)")
        self.sync()
        return n

    def deblock(self, qp, beta_offset_div2=0, tc_offset_div2=0, wait=True):
        self.lib.kvz_hip_batch_deblock(self.handle, qp, beta_offset_div2, tc_offset_div2)
        if wait:
            self.sync()

    def loop_filters(self, model, deblock=True, sao=True, beta_offset_div2=0, tc_offset_div2=0, wait=True):
        """kvz_hip_batch_loop_filters: deblocking + SAO decision + SAO reconstruction on the batch's stream (a PictureModels table: kvz_hip_batch_loop_filters_models,
        every picture with its own QP, lambda and SAO contexts; with sao=False that is the deblocking of a mixed batch; a CtuModels map, after a launch with it:
        kvz_hip_batch_loop_filters_ctu_models, every edge at the QPs of the CUs on its two sides and every CTU's SAO decision under its own lambda)"""
        if _is_ctu_map(model):
            self._check_table(model)
            f = self.lib.kvz_hip_batch_loop_filters_ctu_models
            f.argtypes = [C.c_void_p, C.POINTER(CtuModelsStruct), C.c_int, C.c_int, C.c_int, C.c_int]
            f.restype = C.c_int
            if f(self.handle, C.byref(model.struct), int(deblock), beta_offset_div2, tc_offset_div2, int(sao)) != 0:
                raise BatchError("kvz_hip_batch_loop_filters_ctu_models: the batch cannot run this map (see stderr)")
            if wait:
                self.sync()
            return
        if _is_table(model):
            self._check_table(model)
            f = self.lib.kvz_hip_batch_loop_filters_models
            f.argtypes = [C.c_void_p, C.POINTER(PictureModelsStruct), C.c_int, C.c_int, C.c_int, C.c_int]
            f.restype = C.c_int
            if f(self.handle, C.byref(model.struct), int(deblock), beta_offset_div2, tc_offset_div2, int(sao)) != 0:
                raise BatchError("kvz_hip_batch_loop_filters_models: the batch cannot run this table (see stderr)")
            if wait:
                self.sync()
            return
        f = self.lib.kvz_hip_batch_loop_filters
        f.argtypes = [C.c_void_p, C.POINTER(CostModel), C.c_int, C.c_int, C.c_int, C.c_int]
        f.restype = None
        f(self.handle, C.byref(model), int(deblock), beta_offset_div2, tc_offset_div2, int(sao))
        if wait:
            self.sync()

    def entropy_code(self, model, sao=False, capacity=None, not_last=None, then=None):
        """kvz_hip_batch_entropy_code: the slice data of every picture of the batch, coded on the device from the results of the last launch (and, with sao, of the
        last loop_filters(sao=True)).  -> (bytes of all substreams back to back, sizes as an array [frame][substream]).  then = (batch, model): that batch's pass is
        started once this coder's first stage is through (kvz_hip_batch_entropy_code_then).  With a PictureModels table as `model` every picture's substreams start
        from its own initial contexts (kvz_hip_batch_entropy_code_then_models); `then` then names a batch with a table of its own"""
        if _is_ctu_map(model):  # kvz_hip_batch_entropy_code_ctu_models: after a launch with the same map; every CTU with a coefficient codes its cu_qp_delta
            self._check_table(model)
            if then or not_last is not None:
                raise TypeError("entropy_code with a CtuModels map: no `then`, no tiles")
            f = self.lib.kvz_hip_batch_entropy_code_ctu_models
            f.argtypes = [C.c_void_p, C.POINTER(CtuModelsStruct), C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
            f.restype = C.c_long
            capacity = capacity or entropy_capacity(self.n, self.w, self.h)
            if getattr(self, "_entropy_out", None) is None or self._entropy_out.nbytes < capacity:
                pinned_free(self.lib, getattr(self, "_entropy_ptr", None))
                self._entropy_ptr, self._entropy_out = pinned_bytes(self.lib, capacity)
            sizes = np.zeros((self.n, 1 if model.no_wpp else (self.h + 63) // 64), np.uint32)
            total = f(self.handle, C.byref(model.struct), int(sao), None, self._entropy_out.ctypes.data, capacity, sizes.ctypes.data)
            if total < 0:
                raise BatchError(f"kvz_hip_batch_entropy_code_ctu_models failed ({total}; see stderr)")
            return self._entropy_out[:total], sizes
        table = _is_table(model)
        if table:
            self._check_table(model)
            if then and not _is_table(then[1]):
                raise TypeError("entropy_code with a PictureModels table: then = (batch, PictureModels)")
            then = (then[0], then[1].struct) if then else None
        elif then and _is_table(then[1]):
            raise TypeError("entropy_code with a CostModel: then = (batch, CostModel)")
        f = self.lib.kvz_hip_batch_entropy_code_then_models if table else self.lib.kvz_hip_batch_entropy_code_then
        f.argtypes = [C.c_void_p, C.POINTER(PictureModelsStruct if table else CostModel), C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        f.restype = C.c_long
        flags = None if not_last is None else np.ascontiguousarray(not_last, np.uint8)  # tiles: 1 = other tiles of the slice follow
        assert flags is None or flags.size == self.n
        rows = 1 if model.no_wpp else (self.h + 63) // 64
        capacity = capacity or entropy_capacity(self.n, self.w, self.h)
        if getattr(self, "_entropy_out", None) is None or self._entropy_out.nbytes < capacity:
            pinned_free(self.lib, getattr(self, "_entropy_ptr", None))
            self._entropy_ptr, self._entropy_out = pinned_bytes(self.lib, capacity)  # the slice data is downloaded by the call: a pinned destination, no staging copy
        sizes = np.zeros((self.n, rows), np.uint32)
        total = f(self.handle, C.byref(model.struct if table else model), int(sao), flags.ctypes.data if flags is not None else None, self._entropy_out.ctypes.data, capacity, sizes.ctypes.data,
                  then[0].handle if then else None, C.addressof(then[1]) if then else None)
        if total < 0:
            # -1 the coder, -2 the next batch's launch (in both cases that pass is queued and wants a sync), -3 bad next model (nothing queued)
            raise BatchError(f"kvz_hip_batch_entropy_code failed ({total})")
        return self._entropy_out[:total], sizes

    def entropy_defer_download(self, on=True):
        """kvz_hip_batch_entropy_defer_download: entropy_code returns with the slice data's download queued; sync() before reading the bytes"""
        self.lib.kvz_hip_batch_entropy_defer_download.argtypes = [C.c_void_p, C.c_int]
        self.lib.kvz_hip_batch_entropy_defer_download.restype = None
        self.lib.kvz_hip_batch_entropy_defer_download(self.handle, int(bool(on)))

    def sao_params(self, frame):
        """-> (luma records, chroma records, merge flags) of one frame, one entry per LCU in raster order"""
        from .capi import SaoParams
        n = self.ctus_per_frame
        luma, chroma, merge = (SaoParams * n)(), (SaoParams * n)(), np.zeros(n, np.uint8)
        f = self.lib.kvz_hip_batch_sao_params
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        f.restype = C.c_int
        if f(self.handle, frame, luma, chroma, merge.ctypes.data) != 0:
            raise BatchError("kvz_hip_batch_sao_params failed")
        return luma, chroma, merge

    def checksums(self):
        out = np.zeros((self.n, 3), np.uint32)
        if self.lib.kvz_hip_batch_checksums(self.handle, out.ctypes.data) != 0:
            raise BatchError("kvz_hip_batch_checksums: the batch's last pass was invalid")
        return out

    def md5(self):
        """-> uint8 array [frames][3][16]: kvz_image_md5 of every frame's current reconstruction (--hash md5)"""
        out = np.zeros((self.n, 3, 16), np.uint8)
        self.lib.kvz_hip_batch_md5.argtypes = [C.c_void_p, C.c_void_p]
        self.lib.kvz_hip_batch_md5.restype = C.c_int
        if self.lib.kvz_hip_batch_md5(self.handle, out.ctypes.data) != 0:
            raise BatchError("kvz_hip_batch_md5: the batch's last pass was invalid")
        return out

    def sse(self):
        """-> uint64 array [frames][3]: the exact sum of squared differences of every frame's source against its current reconstruction (after deblock /
        loop_filters if they ran), Y, U, V (kvz_hip_batch_sse)"""
        out = np.zeros((self.n, 3), np.uint64)
        self.lib.kvz_hip_batch_sse.argtypes = [C.c_void_p, C.c_void_p]
        self.lib.kvz_hip_batch_sse.restype = C.c_int
        if self.lib.kvz_hip_batch_sse(self.handle, out.ctypes.data) != 0:
            raise BatchError("kvz_hip_batch_sse: the batch's last pass was invalid")
        return out

    def sse_async(self, out_ptr):
        """kvz_hip_batch_sse_async: the same queued on the batch's stream; the n x 3 uint64 at address `out_ptr` -- pinned_bytes() -- are valid after sync().  A sum queued
        before upload_all_async sees the old pictures, one queued after it the new ones"""
        self.lib.kvz_hip_batch_sse_async.argtypes = [C.c_void_p, C.c_void_p]
        self.lib.kvz_hip_batch_sse_async.restype = C.c_int
        if self.lib.kvz_hip_batch_sse_async(self.handle, out_ptr) != 0:
            raise BatchError("kvz_hip_batch_sse_async: bad argument")

    def psnr(self):
        """-> float64 array [frames][3]: PSNR Y, U, V of every frame as kvazaar computes it (kvz_hip_psnr of sse())"""
        return psnr_of_planes(self.lib, self.sse(), self.w, self.h)

    def kernel_ms(self):
        return self.lib.kvz_hip_batch_last_kernel_ms(self.handle)

    def download(self, frame):
        o = outputs(self.w, self.h)
        ys, cs = self.w * self.h, self.w * self.h // 4
        rc = self.lib.kvz_hip_batch_download(self.handle, frame, ptr(o["rec"]), ptr(o["rec"], offset=ys), ptr(o["rec"], offset=ys + cs),
                                             ptr(o["coeff"]), ptr(o["depth"]), ptr(o["mode"]), o["cost"].ctypes.data_as(C.POINTER(C.c_double)))
        if rc != 0:
            raise BatchError("kvz_hip_batch_download: the batch's last pass was invalid")
        return o

    def download_cu_qps(self, frame):
        """after a launch with a CtuModels map (kvz_hip_batch_download_cu_qps): (the QP of every 8x8 unit, per CTU pred | Q << 8 | coded << 16 | first << 24)"""
        cu_qp, ctu_qp = np.zeros((self.h // 8) * (self.w // 8), np.uint8), np.zeros(self.ctus_per_frame, np.uint32)
        f = self.lib.kvz_hip_batch_download_cu_qps
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        f.restype = C.c_int
        if f(self.handle, frame, cu_qp.ctypes.data, ctu_qp.ctypes.data) != 0:
            raise BatchError("kvz_hip_batch_download_cu_qps: invalid pass, or the batch's last pass had no CtuModels map")
        return cu_qp, ctu_qp

    def download_partitions(self, frame):
        """after a pass with model.search_nxn: (NxN flag per 8x8 CU, luma mode per 4x4 unit)"""
        part, mode4 = np.zeros((self.h // 8) * (self.w // 8), np.uint8), np.zeros((self.h // 4) * (self.w // 4), np.uint8)
        self.lib.kvz_hip_batch_download_partitions.argtypes = [C.c_void_p, C.c_int, u8p, u8p]
        self.lib.kvz_hip_batch_download_partitions.restype = C.c_int
        if self.lib.kvz_hip_batch_download_partitions(self.handle, frame, ptr(part), ptr(mode4)) != 0:
            raise BatchError("kvz_hip_batch_download_partitions: invalid pass, or no pass with search_nxn has run")
        return part, mode4

    def close(self):
        if self.handle:
            self.lib.kvz_hip_batch_destroy(self.handle)
            self.handle = None
        pinned_free(self.lib, getattr(self, "_entropy_ptr", None))
        self._entropy_ptr = self._entropy_out = None


class BatchGroup:
    """kvz_hip_batch_group: the CTU passes of several HipBatch objects -- any picture sizes -- as ONE persistent launch.  Everything else (uploads, loop filters, entropy
    coder, downloads, hashes) is called on the batches as before; a batch stays usable alone between joint launches.  The batches must outlive the group: close()
    the group first."""

    def __init__(self, lib, batches):
        batches = list(batches)
        if any(b.handle is None for b in batches):
            raise ValueError("BatchGroup: a batch of the group has been closed")
        self.lib, self.batches = lib, batches
        lib.kvz_hip_batch_group_create.restype = C.c_void_p
        lib.kvz_hip_batch_group_create.argtypes = [C.c_void_p, C.c_int]
        lib.kvz_hip_batch_group_destroy.restype = None
        lib.kvz_hip_batch_group_destroy.argtypes = [C.c_void_p]
        lib.kvz_hip_batch_group_intra_frames.restype = C.c_int
        lib.kvz_hip_batch_group_intra_frames.argtypes = [C.c_void_p, C.c_void_p]
        lib.kvz_hip_batch_group_last_kernel_ms.restype = C.c_float
        lib.kvz_hip_batch_group_last_kernel_ms.argtypes = [C.c_void_p]
        handles = (C.c_void_p * max(len(batches), 1))(*[b.handle for b in batches])
        self.handle = lib.kvz_hip_batch_group_create(handles, len(batches))
        if not self.handle:
            raise RuntimeError(f"kvz_hip_batch_group_create({len(batches)} batches) failed (see stderr)")

    def _tables(self, models):
        """one entry per batch: a PictureModels, or a CostModel for all of that batch's pictures (wrapped into a table of one model)"""
        models = list(models)
        if len(models) != len(self.batches):
            raise ValueError(f"BatchGroup: {len(models)} models for {len(self.batches)} batches")
        tables = []
        for b, m in zip(self.batches, models):
            if b.handle is None:
                raise ValueError("BatchGroup: a batch of the group has been closed")
            if _is_table(m):
                b._check_table(m)
                tables.append((m, m.struct))
            else:
                one = (CostModel * 1)(m)
                index = (C.c_uint16 * b.n)()
                tables.append(((one, index), PictureModelsStruct(C.sizeof(PictureModelsStruct), 1, one, index)))
        return tables

    def launch(self, models):
        """kvz_hip_batch_group_intra_frames: asynchronous; 1, or -1 when the library refuses (see stderr; nothing is queued on any batch then)"""
        tables = self._tables(models)
        ptrs = (C.c_void_p * len(tables))(*[C.addressof(t[1]) for t in tables])
        return self.lib.kvz_hip_batch_group_intra_frames(self.handle, ptrs)

    def run(self, models):
        if self.launch(models) < 0:
            raise BatchError("kvz_hip_batch_group_intra_frames: the group cannot run these models (see stderr)")
        bad = [i for i, b in enumerate(self.batches) if self.lib.kvz_hip_batch_sync(b.handle) != 0]  # every batch is synced, whatever the first one says
        if bad:
            raise BatchError(f"kvz_hip_batch_sync: a CTU hand-off wait of the joint pass timed out; the results of batches {bad} are invalid")

    def kernel_ms(self):
        """device time of the last joint launch; after the batches were synced"""
        return float(self.lib.kvz_hip_batch_group_last_kernel_ms(self.handle))

    def close(self):
        if self.handle:
            self.lib.kvz_hip_batch_group_destroy(self.handle)
            self.handle = None


def psnr(lib, sse, num_pixels):
    """kvz_hip_psnr: compute_psnr's last step (encmain.c:138-143) -- 999.99 for sse == 0, else 10 log10(num_pixels * 255^2 / sse); on the host, no device involved"""
    lib.kvz_hip_psnr.argtypes = [C.c_uint64, C.c_long]
    lib.kvz_hip_psnr.restype = C.c_double
    return float(lib.kvz_hip_psnr(int(sse), int(num_pixels)))


def psnr_of_planes(lib, sse, width, height):
    """[..., 3] sums of squared differences of width x height 4:2:0 pictures -> float64 [..., 3] PSNR Y, U, V"""
    sse = np.asarray(sse, np.uint64)
    px = (width * height, width * height // 4, width * height // 4)
    return np.array([psnr(lib, v, px[i % 3]) for i, v in enumerate(sse.reshape(-1))], np.float64).reshape(sse.shape)


def psnr_text(psnr3):
    """the PSNR part of kvazaar's per-picture log line (cli.c:735)"""
    return " PSNR Y %2.4f U %2.4f V %2.4f" % tuple(float(v) for v in psnr3)


def entropy_capacity(n, w, h):
    """room for the slice data of n pictures: generous for small batches (noise at a low QP codes to more than the pictures' own bytes), half the pictures' bytes for big
    ones (pinned memory; the call fails with a message when a batch outgrows it and the caller can pass its own capacity)"""
    full = n * w * h * 2 + 65536
    return full if full <= (256 << 20) else n * w * h * 3 // 4 + 65536


def pinned_bytes(lib, nbytes):
    """kvz_hip_host_alloc'ed (hipHostMalloc) byte buffer -> (pointer, numpy view)"""
    lib.kvz_hip_host_alloc.restype = C.c_void_p
    lib.kvz_hip_host_alloc.argtypes = [C.c_size_t]
    p = lib.kvz_hip_host_alloc(nbytes)
    if not p:
        raise MemoryError(f"kvz_hip_host_alloc({nbytes})")
    return p, np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(p))


def pinned_free(lib, p):
    if p:
        lib.kvz_hip_host_free.argtypes = [C.c_void_p]
        lib.kvz_hip_host_free(p)


class PinnedResults:
    """pinned host buffers for kvz_hip_batch_download_all_async: everything the host entropy coder needs of every frame of a batch"""

    def __init__(self, batch):
        lib, w, h, n = batch.lib, batch.w, batch.h, batch.n
        lib.kvz_hip_host_alloc.restype = C.c_void_p
        lib.kvz_hip_host_alloc.argtypes = [C.c_size_t]
        lib.kvz_hip_host_free.restype = None
        lib.kvz_hip_host_free.argtypes = [C.c_void_p]
        lib.kvz_hip_batch_download_all_async.restype = None
        lib.kvz_hip_batch_download_all_async.argtypes = [C.c_void_p] * 5
        self.lib, self.batch = lib, batch
        self.sizes = dict(rec=w * h * 3 // 2 * n, coeff=batch.ctus_per_frame * 6144 * 2 * n, depth=(w // 8) * (h // 8) * n, mode=(w // 8) * (h // 8) * n)
        self.ptrs = {k: lib.kvz_hip_host_alloc(v) for k, v in self.sizes.items()}
        self.bytes = sum(self.sizes.values())

    def download_async(self):
        self.lib.kvz_hip_batch_download_all_async(self.batch.handle, self.ptrs["rec"], self.ptrs["coeff"], self.ptrs["depth"], self.ptrs["mode"])

    def array(self, name, dtype=np.uint8):
        buf = (C.c_uint8 * self.sizes[name]).from_address(self.ptrs[name])
        return np.frombuffer(buf, dtype=dtype)

    def close(self):
        for p in self.ptrs.values():
            self.lib.kvz_hip_host_free(p)
        self.ptrs = {}
