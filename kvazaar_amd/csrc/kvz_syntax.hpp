// kvz_syntax.hpp -- the small facts of H.265 / kvazaar syntax that more than one pass needs, each stated ONCE: the intra CTU pass (kvz_ctu.hpp), RDOQ (kvz_rdoq.hpp),
// the residual walker (kvz_residual.hpp) with the entropy coder (kvz_entropy.hpp) and the inter CTU pass (kvz_inter_ctu.hpp) behind it, and the host-side tables
// (kvz_tables.hpp) all call these.  Free functions without state, host and device.  (The oracle under oracle/ keeps its own copies on purpose: it is the independent
// restatement the tests compare against.)
#pragma once
#include "kvz_ops.hpp"
#include "../../include/kvz_hip_types.h"

namespace kvz {

// ---- scans.  HEVC scans are hierarchical: 4x4 coefficient groups in group order, the same sixteen positions inside every group -- both orders by arithmetic, no table
// in memory on the chain from one coefficient to the next.
// Position y * 4 + x of scan index k inside a group is nibble k of these constants -- diagonal, horizontal, vertical (tables.c kvz_g_sig_last_scan, 4x4 entries)
KVZ_HD unsigned long long scan_pattern16(int scan_mode) { return scan_mode == 0 ? 0xfbe7ad369c258140ull : (scan_mode == 1 ? 0xfedcba9876543210ull : 0xfb73ea62d951c840ull); }
KVZ_HD int scan_in_group(int scan_mode, int k) { return (int)((scan_pattern16(scan_mode) >> (4 * k)) & 15); }
// Raster index of the i-th group in group order (tables.h:45-89 g_sig_last_scan_cg).  diag8: the up-right diagonal order of an 8x8 grid (Tables::diag8), the group order
// of a 32x32 block -- an argument, because where it is read from is the caller's business (RDOQ instantiations stage it in LDS).
template <class PtrU8> KVZ_HD int scan_group(int log2w, int scan_mode, int i, PtrU8 diag8)
{
  if (log2w == 2) return 0;
  if (log2w == 3) return scan_mode == 1 ? i : ((0x3120 >> (4 * i)) & 3);
  if (log2w == 4) return scan_in_group(0, i);
  return diag8[i];
}
// encoderstate.c:1761-1775 kvz_get_scan_order for an intra CU (the chroma mode is the luma mode here); an inter CU scans diagonally
KVZ_HD int intra_scan_order(int mode, int depth)
{
  if (depth >= 3) {
    if (mode >= 6 && mode <= 14) return 2;
    if (mode >= 22 && mode <= 30) return 1;
  }
  return 0;
}

// ---- residual contexts
// context.c:366-399 kvz_context_get_sig_ctx_inc
KVZ_HD int sig_ctx_inc(int pattern_sig_ctx, int scan_idx, int pos_x, int pos_y, int log2_size, int type)
{
  if (pos_x + pos_y == 0) return 0;
  if (log2_size == 2) { const unsigned long long map = 0x8877886654325410ull; return (int)((map >> (4 * (4 * pos_y + pos_x))) & 15); }  // ctx_ind_map
  const int offset = log2_size == 3 ? (scan_idx == 0 ? 9 : 15) : (type == 0 ? 21 : 12);
  const int xs = pos_x & 3, ys = pos_y & 3;
  int cnt;
  if (pattern_sig_ctx == 0) cnt = xs + ys <= 2 ? (xs + ys == 0 ? 2 : 1) : 0;
  else if (pattern_sig_ctx == 1) cnt = ys <= 1 ? (ys == 0 ? 2 : 1) : 0;
  else if (pattern_sig_ctx == 2) cnt = xs <= 1 ? (xs == 0 ? 2 : 1) : 0;
  else cnt = 2;
  return ((type == 0 && ((pos_x >> 2) + (pos_y >> 2)) > 0) ? 3 : 0) + offset + cnt;
}
// g_group_idx (encoderstate.h:397, rdo.c:60): the prefix group of a last-position coordinate, v in [0, 31]
KVZ_HD int group_idx(int v)
{
  const unsigned long long lo = 0x7777666655443210ull;  // [0..15]; [16..23] = 8, [24..31] = 9
  return v < 16 ? (int)((lo >> (4 * v)) & 15) : (v < 24 ? 8 : 9);
}
// kvz_encode_last_significant_xy (encode_coding_tree.c:63-115): bin i of a coordinate's prefix uses context base_x / base_y + (i >> shift) (KVZ_HIP_CX_* numbering);
// the prefix of the last group, group_idx(width - 1), has no terminating zero.  type 0 luma, else chroma.
struct LastPosCtx { int base_x, base_y, shift; };
KVZ_HD LastPosCtx last_pos_ctx(int log2_size, int type)
{
  const int index = log2_size - 2, ctx_offset = type ? 0 : (index * 3 + (index + 1) / 4);
  LastPosCtx l;
  l.base_x = (type ? KVZ_HIP_CX_LAST_X_CHROMA : KVZ_HIP_CX_LAST_X_LUMA) + ctx_offset;
  l.base_y = (type ? KVZ_HIP_CX_LAST_Y_CHROMA : KVZ_HIP_CX_LAST_Y_LUMA) + ctx_offset;
  l.shift = type ? index : (index + 3) / 4;
  return l;
}

// ---- coding tree
// z-order offset of the 4x4 unit at (x, y) inside a 64x64 CTU's block of levels (cu.h:385-421): Morton index of the unit times 16
KVZ_HD unsigned ctu_zorder(int x, int y)
{
  unsigned r = 0;
  for (int b = 0; b < 4; b++) r |= (((unsigned)(x >> (2 + b)) & 1u) << (2 * b)) | (((unsigned)(y >> (2 + b)) & 1u) << (2 * b + 1));
  return r * 16;
}
// intra.c:84-126 kvz_intra_get_dir_luma_predictor, from the candidate modes of the left and above neighbours (DC = 1 where there is none: which neighbours count is
// the caller's knowledge)
template <class T> KVZ_HD void intra_mpm(int l, int a, T preds[3])
{
  if (l == a) {
    if (l > 1) { preds[0] = (T)l; preds[1] = (T)(((l + 29) % 32) + 2); preds[2] = (T)(((l - 1) % 32) + 2); }
    else { preds[0] = 0; preds[1] = 1; preds[2] = 26; }
  } else {
    preds[0] = (T)l; preds[1] = (T)a;
    if (l && a) preds[2] = 0; else preds[2] = (T)((l + a) < 2 ? 26 : 1);
  }
}

// ---- pictures of one launch under different cost models (kvz_hip_picture_models): the row of the launch's model table that a picture uses.  The CTU pass, the
// loop filters and the entropy coder all select through this; a null map is the single-model launch (row 0).
KVZ_HD int picture_model(const uint16_t *model_of_picture, long picture) { return model_of_picture ? (int)model_of_picture[picture] : 0; }

// ---- quantisation, flat scaling lists
// kvz_g_chroma_scale (transform.c:56-62, H.265 table 8-10): the chroma QP of a luma QP, clipped to the table
KVZ_HD int chroma_qp(int qp)
{
  const u8 chroma_scale[58] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 29, 30, 31, 32,
                                33, 33, 34, 34, 35, 35, 36, 36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51 };
  return chroma_scale[iclip(0, 57, qp)];
}
// kvz_g_quant_scales / kvz_g_inv_quant_scales (scalinglist.c:78-79) of qp % 6
KVZ_HD int quant_scale(int qp_rem) { const int t[6] = { 26214, 23302, 20560, 18396, 16384, 14564 }; return t[qp_rem]; }
KVZ_HD int inv_quant_scale(int qp_rem) { const int t[6] = { 40, 45, 51, 57, 64, 72 }; return t[qp_rem]; }

}  // namespace kvz
