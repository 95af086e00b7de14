"""The tiled inter chain (BASELINE config 4 sharded by tile) as the tests run it: I -> B -> B .. of a clip cut into kvazaar's --tiles grid, every picture through
CTU pass -> loop filters -> exchange -> next picture.  The pass of a B picture's tile is pluggable (host simulation of the device sources / the device); the I picture's pass and
the loop filters are test infrastructure (host simulation, oracle).  Shared by tests/test_dist_cpu.py (two gloo ranks) and tests/test_gpu_inter_ctu.py."""
import ctypes as C

import numpy as np

import ctu_common as cc
import flatapi
import inter_common as ic
from kvazaar_amd import inter, sharding


def tile_sub(frame, x, y, tw, th, W, H):
    """tile (x, y, tw, th) of a planar W x H frame as a planar picture of its own"""
    Y = frame[:W * H].reshape(H, W)[y:y + th, x:x + tw]
    U = frame[W * H:W * H * 5 // 4].reshape(H // 2, W // 2)[y // 2:(y + th) // 2, x // 2:(x + tw) // 2]
    V = frame[W * H * 5 // 4:].reshape(H // 2, W // 2)[y // 2:(y + th) // 2, x // 2:(x + tw) // 2]
    return np.ascontiguousarray(np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)]))


def load_hostsim():
    sim = C.CDLL(flatapi.hostsim_path())
    ft = sim.kvz_hostsim_inter_tile
    ft.restype = None
    ft.argtypes = [C.c_int] * 4 + [C.c_uint64, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 5 + [C.c_int] * 5
    return sim


def hostsim_tile_pass(sim):
    """the inter CTU pass of one tile by the device sources in host simulation (kvz_hostsim_inter_tile): `veryfast`, tiles => --no-wpp, no TMVP (cfg.c:920-975)"""
    mc = cc.model_constants()
    fb = np.array(mc["entropy_fbits"], np.float32)

    def run(tw, th, pq, k, src, ref_frame, ref_cu, w, h, tx, ty):
        rec = np.zeros(tw * th * 3 // 2, np.uint8)
        cu = np.zeros((th // 4, tw // 4), ic.CU_DTYPE)
        sim.kvz_hostsim_inter_tile(tw, th, pq, k, int(mc["coeff_weights"][str(pq)]), fb.ctypes.data, 0, 1, 1, 2, 3, 1, 28, src.ctypes.data, ref_frame.ctypes.data, ref_cu.ctypes.data,
                                   rec.ctypes.data, cu.ctypes.data, w, h, tx, ty, 1)
        return rec, cu
    return run


def tiled_inter_chain(clip, rank, world, dist, tile_pass, sim):
    """-> (final pictures [n, fs], CU records [n, h/4, w/4]) as every rank holds them after the last exchange"""
    import torch
    from flatapi import SaoParams, ptr
    from test_encoder_parity import oracle_model
    name, w, h, n, qp, tiles, seed, noise, pan = clip
    oracle = flatapi.load_oracle()
    frames = ic.clip(w, h, n, seed, noise, pan)
    cols, rows = (int(v) for v in tiles.split("x"))
    plan = sharding.exchange_plan(w, h, cols, rows, world)
    ex = sharding.ReferenceExchange(dist, plan, rank, world, w, h, torch.device("cpu"))
    mine = sharding.tiles_of_rank(len(plan["tiles"]), rank, world)
    ref_frame, ref_cu = None, None
    pictures, records = [], []
    for k in range(n):
        pq = inter.lowdelay_picture_qp(qp, k)
        model = oracle_model(oracle, pq)
        model.no_wpp = 1  # tiles imply --no-wpp (cfg.c:925-978)
        local_cu = {}
        for slot, ti in enumerate(mine):
            tx, ty, tw, th = plan["tiles"][ti]
            src = tile_sub(frames[k], tx, ty, tw, th, w, h)
            nl = ((tw + 63) // 64) * ((th + 63) // 64)
            luma, chroma, merge = (SaoParams * nl)(), (SaoParams * nl)(), np.zeros(nl, np.uint8)
            if k == 0:
                o = cc.run_hostsim(sim, model, tw, th, src)
                rec = o["rec"].copy()
                cu = inter.intra_picture_cu_info(tw, th).reshape(th // 4, tw // 4).copy()
                cu["depth"] = np.repeat(np.repeat(o["depth"].reshape(th // 8, tw // 8), 2, 0), 2, 1)
                cu["mode"] = np.repeat(np.repeat(o["mode"].reshape(th // 8, tw // 8), 2, 0), 2, 1)
                cu["tr_depth"] = np.maximum(cu["depth"], 1)
                f = oracle.lib.kvz_oracle_sao_search_frame
                f.restype = None
                f(C.byref(model), tw, th, ptr(src), ptr(rec), ptr(o["depth"]), 1, 0, 0, luma, chroma, ptr(merge))
            else:
                rec, cu = tile_pass(tw, th, pq, k, src, ref_frame, ref_cu, w, h, tx, ty)
                init = ic.b_slice_context_states(oracle, pq)
                model.ctx_init[148], model.ctx_init[149] = int(init[148]), int(init[149])  # KVZ_HIP_CX_SAO_MERGE / _TYPE of a B slice
                dbk = ic.cu_dbk_records(cu)
                f = oracle.lib.kvz_oracle_sao_search_frame_inter
                f.restype = None
                f(C.byref(model), tw, th, ptr(src), ptr(rec), dbk.ctypes.data_as(C.c_void_p), 1, 1, 0, 0, luma, chroma, ptr(merge))
            final = rec.copy()
            g = oracle.lib.kvz_oracle_sao_frame
            g.restype = None
            g(tw, th, ptr(rec), ptr(final), luma, chroma)
            ex.send_slot(slot).copy_(torch.from_numpy(final))
            local_cu[ti] = cu
        ref_frame = ex.exchange().numpy().copy()  # THE collective of the sharded inter configuration: every rank ends up with the whole reference frame
        ref_cu = sharding.allgather_cu_records(dist, plan, rank, world, local_cu, w, h, ic.CU_DTYPE)
        pictures.append(ref_frame)
        records.append(ref_cu)
    return np.stack(pictures), np.stack(records)
