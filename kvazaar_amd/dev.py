"""ctypes view of include/kvz_hip_dev.h (device-resident batch entry points) for the GPU tests and bench_kernels.py."""
import ctypes as C

import numpy as np

TRANSFORM_KINDS = {"dct4": 0, "dct8": 1, "dct16": 2, "dct32": 3, "dst4": 4, "idct4": 5, "idct8": 6, "idct16": 7, "idct32": 8, "idst4": 9}
TRANSFORM_SIZE = {0: 4, 1: 8, 2: 16, 3: 32, 4: 4, 5: 4, 6: 8, 7: 16, 8: 32, 9: 4}


class Dev:
    def __init__(self, cdll):
        self.lib = l = cdll
        vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
        l.kvz_hip_dev_alloc.restype = vp; l.kvz_hip_dev_alloc.argtypes = [sz]
        l.kvz_hip_dev_free.restype = None; l.kvz_hip_dev_free.argtypes = [vp]
        l.kvz_hip_dev_upload.restype = None; l.kvz_hip_dev_upload.argtypes = [vp, vp, sz]
        l.kvz_hip_dev_download.restype = None; l.kvz_hip_dev_download.argtypes = [vp, vp, sz]
        l.kvz_hip_dev_sync.restype = None; l.kvz_hip_dev_sync.argtypes = []
        l.kvz_hip_dev_timer_start.restype = None; l.kvz_hip_dev_timer_start.argtypes = []
        l.kvz_hip_dev_timer_stop.restype = C.c_float; l.kvz_hip_dev_timer_stop.argtypes = []
        for f in (l.kvz_hip_dev_sad_nxn, l.kvz_hip_dev_satd_nxn):
            f.restype = None; f.argtypes = [ci, vp, vp, ci, vp]
        l.kvz_hip_dev_transform.restype = None; l.kvz_hip_dev_transform.argtypes = [ci, vp, vp, vp, ci, ci]
        l.kvz_hip_dev_angular_pred.restype = None; l.kvz_hip_dev_angular_pred.argtypes = [ci, ci, vp, vp, ci, vp]
        l.kvz_hip_dev_intra_select.restype = ci; l.kvz_hip_dev_intra_select.argtypes = [ci, ci, vp, vp, vp, ci, vp]
        l.kvz_hip_dev_cu8_units.restype = ci; l.kvz_hip_dev_cu8_units.argtypes = [ci, ci, vp, vp, vp, vp, vp]
        l.kvz_hip_dev_satd8_blocks.restype = ci; l.kvz_hip_dev_satd8_blocks.argtypes = [vp, vp, ci, vp]
        if hasattr(l, "kvz_hip_dev_rough_rows"):  # (an earlier build's library, given through KVZ_HIP_LIB for a comparison run, does not have it)
            l.kvz_hip_dev_rough_rows.restype = ci; l.kvz_hip_dev_rough_rows.argtypes = [ci, vp, vp, ci, vp]
        if hasattr(l, "kvz_hip_dev_cu16_predict"):
            l.kvz_hip_dev_cu16_predict.restype = ci; l.kvz_hip_dev_cu16_predict.argtypes = [vp, vp, vp, ci, vp]

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.lib.kvz_hip_dev_alloc(a.nbytes)
        self.lib.kvz_hip_dev_upload(p, a.ctypes.data, a.nbytes)
        return p

    def copy_in(self, p, a):
        a = np.ascontiguousarray(a)
        self.lib.kvz_hip_dev_upload(p, a.ctypes.data, a.nbytes)

    def empty(self, nbytes):
        return self.lib.kvz_hip_dev_alloc(nbytes)

    def get(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        self.lib.kvz_hip_dev_download(out.ctypes.data, p, out.nbytes)
        return out

    def free(self, *ps):
        for p in ps:
            self.lib.kvz_hip_dev_free(p)

    def entropy_code_intra(self, width, height, model, cu_depth, cu_mode, coeff, cu_part=None, cu_mode4=None, not_last=None, sao=None, capacity=None):
        """kvz_hip_dev_entropy_code_intra on host arrays: the results of n I pictures back to back (cu_depth / cu_mode / cu_part per 8x8 unit, cu_mode4 per 4x4 unit,
        coeff 6144 int16 per CTU; n from cu_depth), uploaded here and freed again.  model: a kvz_hip_intra_cost_model (batch.CostModel); not_last: a flag per
        picture or None; sao: (luma, chroma, merge) -- kvz_hip_sao_params records of every CTU of every picture as bytes or int32 words, merge 0 / 1 / 2 -- or None.
        -> (bytes of all substreams back to back, sizes as an array [picture][substream])"""
        f = self.lib.kvz_hip_dev_entropy_code_intra
        f.restype = C.c_long
        f.argtypes = [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p] * 6 + [C.c_size_t, C.c_void_p]
        n = np.asarray(cu_depth).size // ((width // 8) * (height // 8))
        host = [None if a is None else np.ascontiguousarray(a) for a in (not_last,) + (tuple(sao) if sao else (None, None, None))]
        if host[0] is not None:
            host[0] = host[0].astype(np.uint8)
        capacity = capacity or n * width * height * 12 + 65536  # dense blocks of 16-bit levels cost 5 bytes per sample and more
        out, sizes = np.zeros(capacity, np.uint8), np.zeros((n, 1 if model.no_wpp else (height + 63) // 64), np.uint32)
        dev = [None if a is None else self.put(a) for a in (cu_depth, cu_mode, cu_part, cu_mode4, coeff)]
        try:
            total = f(*dev, width, height, n, C.addressof(model), *[None if a is None else a.ctypes.data for a in host], out.ctypes.data, capacity, sizes.ctypes.data)
        finally:
            self.free(*[p for p in dev if p is not None])
        if total < 0:
            raise RuntimeError(f"kvz_hip_dev_entropy_code_intra failed ({total}; see stderr)")
        return out[:total].tobytes(), sizes
