// kvz_inter_host.hpp -- host side of the inter CTU pass (kvz_inter_ctu.hpp): the per-picture model (lambda, quantisation scalars, the B or P slice's context
// initialisation, kvz_init_contexts context.c:202-305 with row 0 of the tables :36-193 or -- P -- their row 1, typed here from H.265 9.3.2.2).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "kvz_inter_ctu.hpp"
#include "kvz_inter_pictures.hpp"
#include "kvz_inter_refs.hpp"
#include "kvz_scaling_lists.hpp"
#include "kvz_tables.hpp"

namespace kvz {

inline int inter_ctx_state(int qp, int init_value)  // context.c:202-213 kvz_ctx_init
{
  const int slope = (init_value >> 4) * 5 - 45, offset = ((init_value & 15) << 3) - 16;
  int st = ((slope * qp) >> 4) + offset;
  st = st < 1 ? 1 : (st > 126 ? 126 : st);
  return st >= 64 ? ((st - 64) << 1) + 1 : (63 - st) << 1;
}

// Row 0 (B slices) of the residual coder's initialisation tables (context.c:111-193: INIT_SIG_CG_FLAG, INIT_SIG_FLAG, INIT_LAST, INIT_ONE_FLAG, INIT_ABS_FLAG), entry
// KVZ_HIP_CX_x - KVZ_HIP_CX_SIG_CG for context KVZ_HIP_CX_x: the layout both the entropy coder's context set and the search contexts (ICtx from IX_RES on) keep
inline void b_slice_residual_init_values(uint8_t v[KVZ_HIP_CX_ABS_CHROMA + 2 - KVZ_HIP_CX_SIG_CG])
{
  static const uint8_t sig_cg[4] = { 121, 140, 61, 154 };
  static const uint8_t sig[42] = { 170, 154, 139, 153, 139, 123, 123, 63, 124, 166, 183, 140, 136, 153, 154, 166, 183, 140, 136, 153, 154, 166, 183, 140, 136, 153, 154,
                                   170, 153, 138, 138, 122, 121, 122, 121, 167, 151, 183, 140, 151, 183, 140 };
  static const uint8_t last[30] = { 125, 110, 124, 110, 95, 94, 125, 111, 111, 79, 125, 126, 111, 111, 79, 108, 123, 93, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154 };
  static const uint8_t one[24] = { 154, 196, 167, 167, 154, 152, 167, 182, 182, 134, 149, 136, 153, 121, 136, 122, 169, 208, 166, 167, 154, 152, 167, 182 };
  static const uint8_t absf[6] = { 107, 167, 91, 107, 107, 167 };
  const int b = KVZ_HIP_CX_SIG_CG;
  for (int i = 0; i < 4; i++) v[KVZ_HIP_CX_SIG_CG - b + i] = sig_cg[i];
  for (int i = 0; i < 27; i++) v[KVZ_HIP_CX_SIG_LUMA - b + i] = sig[i];
  for (int i = 0; i < 15; i++) {
    v[KVZ_HIP_CX_SIG_CHROMA - b + i] = sig[27 + i];
    v[KVZ_HIP_CX_LAST_Y_LUMA - b + i] = v[KVZ_HIP_CX_LAST_X_LUMA - b + i] = last[i];
    v[KVZ_HIP_CX_LAST_Y_CHROMA - b + i] = v[KVZ_HIP_CX_LAST_X_CHROMA - b + i] = last[15 + i];
  }
  for (int i = 0; i < 16; i++) v[KVZ_HIP_CX_ONE_LUMA - b + i] = one[i];
  for (int i = 0; i < 8; i++) v[KVZ_HIP_CX_ONE_CHROMA - b + i] = one[16 + i];
  for (int i = 0; i < 4; i++) v[KVZ_HIP_CX_ABS_LUMA - b + i] = absf[i];
  for (int i = 0; i < 2; i++) v[KVZ_HIP_CX_ABS_CHROMA - b + i] = absf[4 + i];
}

// ... and the P row of the same tables (H.265 9.3.2.2 Tables 9-26 to 9-31, initType 1: coded_sub_block_flag, sig_coeff_flag, last_sig_coeff_{x,y}_prefix,
// coeff_abs_level_greater1_flag, coeff_abs_level_greater2_flag), in the same layout
inline void p_slice_residual_init_values(uint8_t v[KVZ_HIP_CX_ABS_CHROMA + 2 - KVZ_HIP_CX_SIG_CG])
{
  static const uint8_t sig_cg[4] = { 121, 140, 61, 154 };
  static const uint8_t sig[42] = { 155, 154, 139, 153, 139, 123, 123, 63, 153, 166, 183, 140, 136, 153, 154, 166, 183, 140, 136, 153, 154, 166, 183, 140, 136, 153, 154,
                                   170, 153, 123, 123, 107, 121, 107, 121, 167, 151, 183, 140, 151, 183, 140 };
  static const uint8_t last[30] = { 125, 110, 94, 110, 95, 79, 125, 111, 110, 78, 110, 111, 111, 95, 94, 108, 123, 108, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154 };
  static const uint8_t one[24] = { 154, 196, 196, 167, 154, 152, 167, 182, 182, 134, 149, 136, 153, 121, 136, 137, 169, 194, 166, 167, 154, 167, 137, 182 };
  static const uint8_t absf[6] = { 107, 167, 91, 122, 107, 167 };
  const int b = KVZ_HIP_CX_SIG_CG;
  for (int i = 0; i < 4; i++) v[KVZ_HIP_CX_SIG_CG - b + i] = sig_cg[i];
  for (int i = 0; i < 27; i++) v[KVZ_HIP_CX_SIG_LUMA - b + i] = sig[i];
  for (int i = 0; i < 15; i++) {
    v[KVZ_HIP_CX_SIG_CHROMA - b + i] = sig[27 + i];
    v[KVZ_HIP_CX_LAST_Y_LUMA - b + i] = v[KVZ_HIP_CX_LAST_X_LUMA - b + i] = last[i];
    v[KVZ_HIP_CX_LAST_Y_CHROMA - b + i] = v[KVZ_HIP_CX_LAST_X_CHROMA - b + i] = last[15 + i];
  }
  for (int i = 0; i < 16; i++) v[KVZ_HIP_CX_ONE_LUMA - b + i] = one[i];
  for (int i = 0; i < 8; i++) v[KVZ_HIP_CX_ONE_CHROMA - b + i] = one[16 + i];
  for (int i = 0; i < 4; i++) v[KVZ_HIP_CX_ABS_LUMA - b + i] = absf[i];
  for (int i = 0; i < 2; i++) v[KVZ_HIP_CX_ABS_CHROMA - b + i] = absf[4 + i];
}

// The initial values of the syntax contexts an inter slice codes with, by name: the B row (initType 2) and the P row (initType 1) of H.265 Tables 9-5 to 9-25.
// What both the search contexts (inter_model_init, IX_*) and the entropy coder's set (kvz_slice_contexts.hpp, KVZ_HIP_CX_* / KVZ_EB_CX_*) are filled from.
// P differs from B in merge_flag, merge_idx, pred_mode_flag, abs_mvd_greater0_flag, prev_intra_luma_pred_flag, cbf_cb / cbf_cr at depth 1 and sao_type_idx.
struct SliceSyntaxInit {
  uint8_t split[3], skip[3], merge_flag, merge_idx, pred_mode, part, intra, chroma, cbf_luma[2], cbf_chroma[4], mvd[2], mvp_idx, inter_dir[5], root_cbf, sao_merge, sao_type;
  uint8_t ref_idx[2];  // ref_idx_l0 / ref_idx_l1 (Table 9-17): only a launch with reference lists (kvz_hip_inter_refs) has contexts for it
};
inline const SliceSyntaxInit &slice_syntax_init(int slice_type)
{
  static const SliceSyntaxInit b = { { 107, 139, 126 }, { 197, 185, 201 }, 154, 137, 134, 154, 183, 152, { 153, 111 }, { 149, 92, 167, 154 }, { 169, 198 }, 168, { 95, 79, 63, 31, 31 }, 79, 153, 160, { 153, 153 } };
  static const SliceSyntaxInit p = { { 107, 139, 126 }, { 197, 185, 201 }, 110, 122, 149, 154, 154, 152, { 153, 111 }, { 149, 107, 167, 154 }, { 140, 198 }, 168, { 95, 79, 63, 31, 31 }, 79, 153, 185, { 153, 153 } };
  return slice_type == KVZ_HIP_SLICE_P ? p : b;
}
inline void slice_residual_init_values(int slice_type, uint8_t v[KVZ_HIP_CX_ABS_CHROMA + 2 - KVZ_HIP_CX_SIG_CG])
{
  if (slice_type == KVZ_HIP_SLICE_P) p_slice_residual_init_values(v); else b_slice_residual_init_values(v);
}
// a slice type the inter pass and the inter coder cover: B or P.  false and a message otherwise
inline bool inter_slice_type_known(int slice_type, const char *who)
{
  if (slice_type == KVZ_HIP_SLICE_B || slice_type == KVZ_HIP_SLICE_P) return true;
  if (slice_type == KVZ_HIP_SLICE_I) fprintf(stderr, "%s: slice type I (%d): an I picture has no inter pass and no inter coder (kvz_hip_batch.h)\n", who, slice_type);
  else fprintf(stderr, "%s: slice type %d is none of KVZ_HIP_SLICE_B (0), KVZ_HIP_SLICE_P (1), KVZ_HIP_SLICE_I (2)\n", who, slice_type);
  return false;
}

// The geometry kvz_hip_dev_inter_ctu_pass[_tiles] covers: pictures of whole 8x8 blocks up to 255 CTUs a side (the ticket packs the CTU column and row into a byte each),
// and -- ref_w / ref_h non-zero: the pictures are tiles of that frame -- a tile that lies in its reference frame on the 8-sample grid.  The kernel addresses CU
// records with 24-bit multiplies, (cell index) * sizeof(CuInfo) in InterCtu::cell_at and cand_fetch: the signed 24-bit operand holds a cell index below 2^23, so a
// picture or a reference frame of 2^23 or more 4x4 cells is refused, as is a reference frame beyond the 64 * 255 samples a picture may have.  0 = covered
inline int inter_pass_geometry_refused(int width, int height, int n_pictures, int ref_w, int ref_h, int tile_x, int tile_y)
{
  const int max_side = 64 * 255;
  const long max_cells = 1l << 23;
  if (width <= 0 || height <= 0 || (width & 7) || (height & 7) || width > max_side || height > max_side || n_pictures > 65535) return 1;
  if ((long)(width / 4) * (height / 4) >= max_cells) return 1;
  if (ref_w || ref_h) {
    if (ref_w <= 0 || ref_h <= 0 || (ref_w & 7) || (ref_h & 7) || ref_w > max_side || ref_h > max_side) return 2;
    if (tile_x < 0 || tile_y < 0 || (tile_x & 7) || (tile_y & 7) || tile_x + width > ref_w || tile_y + height > ref_h) return 2;
    if ((long)(ref_w / 4) * (ref_h / 4) >= max_cells) return 2;
  }
  return 0;
}

// kvz_hip_inter_params grows at its end, and struct_size says which version the caller was built against.  Two are known: this library's, and the one before the
// three me_* members (everything in front of me_algorithm) -- a binding that was compiled before them keeps working and gets the default search, which is what it
// asked for.  *full: the caller's members in this library's struct, the rest zero.  Any other size is refused: false and a message.
inline bool inter_params_full(const kvz_hip_inter_params *p, kvz_hip_inter_params *full, const char *who)
{
  const size_t before_me = offsetof(kvz_hip_inter_params, me_algorithm);
  if (!p || (p->struct_size != sizeof(kvz_hip_inter_params) && p->struct_size != before_me)) {
    fprintf(stderr, "%s: kvz_hip_inter_params.struct_size %u is not this library's %zu (zero the struct, set struct_size = sizeof, build against the library's headers)\n", who, p ? p->struct_size : 0u, sizeof(kvz_hip_inter_params));
    return false;
  }
  memset(full, 0, sizeof *full);
  memcpy(full, p, p->struct_size);
  full->struct_size = (uint32_t)sizeof *full;
  return true;
}

// The launch's choice of the integer motion search (kvz_hip_inter_params me_algorithm / me_max_steps / me_early_termination): what every entry point of the pass
// refuses of it before anything is queued -- false and a message --, `excluded` naming what the call has that the ME builds do not cover ("tiles", "scaling lists",
// "a joint launch") or nullptr
inline bool inter_me_chosen(const kvz_hip_inter_params *p) { return p->me_algorithm != 0 || p->me_max_steps != 0 || p->me_early_termination != 0; }
inline bool inter_me_known(const kvz_hip_inter_params *p, const char *excluded, const char *who)
{
  if (p->me_algorithm < 0 || p->me_algorithm > 7) { fprintf(stderr, "%s: me_algorithm %d outside 0..7\n", who, p->me_algorithm); return false; }
  if (p->me_max_steps < 0) { fprintf(stderr, "%s: me_max_steps %d is negative (0: no limit)\n", who, p->me_max_steps); return false; }
  if (p->me_early_termination < 0 || p->me_early_termination > 2) { fprintf(stderr, "%s: me_early_termination %d outside 0..2\n", who, p->me_early_termination); return false; }
  if (excluded && inter_me_chosen(p)) {
    fprintf(stderr, "%s: me_algorithm / me_max_steps / me_early_termination (%d, %d, %d) are not covered together with %s\n", who, p->me_algorithm, p->me_max_steps, p->me_early_termination, excluded);
    return false;
  }
  return true;
}
// The slice type of a launch (kvz_hip_dev_inter_ctu_pass_slices, kvz_hip_dev_entropy_code_inter_slices): what those entry points refuse of it before anything is
// queued -- false and a message: a type that is neither B nor P, and P together with what the P builds do not cover (tiles; a chosen integer search)
inline bool inter_slice_launch_known(const kvz_hip_inter_params *p, bool has_tile_xy, int slice_type, const char *who)
{
  if (!inter_slice_type_known(slice_type, who)) return false;
  if (slice_type != KVZ_HIP_SLICE_P) return true;
  if (p->ref_width || p->ref_height || p->tile_x || p->tile_y || has_tile_xy) {
    fprintf(stderr, "%s: P pictures are not covered together with tiles (ref_width %d, ref_height %d, tile_x %d, tile_y %d%s)\n", who, p->ref_width, p->ref_height, p->tile_x, p->tile_y, has_tile_xy ? ", tile_xy" : "");
    return false;
  }
  if (inter_me_chosen(p)) {
    fprintf(stderr, "%s: P pictures are not covered together with me_algorithm / me_max_steps / me_early_termination (%d, %d, %d)\n", who, p->me_algorithm, p->me_max_steps, p->me_early_termination);
    return false;
  }
  return true;
}
// The reference lists of a launch (the kvz_hip_dev_*_refs entry points): what those entry points refuse of them before anything is queued, besides what
// inter_slice_launch_known refuses of the slice type -- false and a message: lists without a POC per picture, with a slice type other than P (which brings the
// refusal of tiles and of the me_* members with it), and whatever inter_refs_known refuses of the struct.  has_pictures / poc: the call's kvz_hip_inter_pictures
// (the loop filters have none and pass poc == nullptr with has_pictures true: their twin takes a QP array)
inline bool inter_refs_launch_known(const kvz_hip_inter_refs *refs, int n_pictures, bool has_pictures, const int32_t *poc, int slice_type, const char *who)
{
  if (!refs) return true;
  if (slice_type != KVZ_HIP_SLICE_P) { fprintf(stderr, "%s: reference lists (kvz_hip_inter_refs) are covered for KVZ_HIP_SLICE_P only, not slice type %d\n", who, slice_type); return false; }
  if (!has_pictures) { fprintf(stderr, "%s: reference lists (kvz_hip_inter_refs) need `pictures`: the POC of every picture comes from there\n", who); return false; }
  return inter_refs_known(refs, n_pictures, poc, who);
}
inline void inter_model_set_me(InterModel *m, const kvz_hip_inter_params *p) { m->me_algorithm = p->me_algorithm; m->me_max_steps = p->me_max_steps; m->me_early_termination = p->me_early_termination; }

inline void inter_model_init(InterModel *m, int qp, int poc, uint64_t coeff_weights, const float fbits[128], int mv_constraint, int sao, int deblock, int fme_level,
                             int pu_depth_inter_max, int no_wpp, int fast_residual_cost, int pic_w = 0, int pic_h = 0, int ref_w = 0, int ref_h = 0, int tile_x = 0, int tile_y = 0, int no_tmvp = 0,
                             int scaling_list = 0 /* a launch with scaling lists: the inverse scalars of the rule that takes a factor per position (quant-generic.c:309-333) */,
                             int slice_type = KVZ_HIP_SLICE_B /* or KVZ_HIP_SLICE_P: the row of the tables the initial context states come from */,
                             int refs = 0 /* a launch with reference lists: the search contexts hold ref_idx_l0's two (IX_REF_IDX) */)
{
  memset(m, 0, sizeof *m);
  m->qp = qp; m->poc = poc;
  m->lambda = 0.57 * pow(2.0, (qp - 12) / 3.0);  // rate_control.c:678-691
  m->lambda_sqrt = sqrt(m->lambda);
  m->coeff_weights = coeff_weights;
  m->coeff_cabac = inter_qp_prices_with_cabac(qp, fast_residual_cost);  // rdo.c:311-340: cfg.fast_residual_cost_limit (28 `ultrafast` .. `veryfast`, 0 `faster`), MAX_FAST_COEFF_COST_QP
  m->ref_w = ref_w > 0 ? ref_w : pic_w; m->ref_h = ref_h > 0 ? ref_h : pic_h; m->tile_x = ref_w > 0 ? tile_x : 0; m->tile_y = ref_h > 0 ? tile_y : 0;
  m->no_tmvp = no_tmvp;
  m->mv_constraint = mv_constraint; m->sao = sao; m->deblock = deblock; m->fme_level = fme_level; m->pu_depth_inter_max = pu_depth_inter_max; m->no_wpp = no_wpp;
  uint8_t init[IX_COUNT];
  memset(init, 154, sizeof init);
  const SliceSyntaxInit &v = slice_syntax_init(slice_type);
  for (int i = 0; i < 3; i++) { init[IX_SPLIT + i] = v.split[i]; init[IX_SKIP + i] = v.skip[i]; }
  init[IX_MERGE_FLAG] = v.merge_flag; init[IX_MERGE_IDX] = v.merge_idx; init[IX_PRED_MODE] = v.pred_mode; init[IX_PART] = v.part; init[IX_INTRA] = v.intra; init[IX_CHROMA] = v.chroma;
  init[IX_CBF_LUMA] = v.cbf_luma[0]; init[IX_CBF_LUMA + 1] = v.cbf_luma[1]; init[IX_CBF_CHROMA] = v.cbf_chroma[0]; init[IX_CBF_CHROMA + 1] = v.cbf_chroma[1];
  init[IX_MVD] = v.mvd[0]; init[IX_MVD + 1] = v.mvd[1]; init[IX_MVP_IDX] = v.mvp_idx;
  for (int i = 0; i < 5; i++) init[IX_INTER_DIR + i] = v.inter_dir[i];
  init[IX_ROOT_CBF] = v.root_cbf;
  if (refs) { init[IX_REF_IDX] = v.ref_idx[0]; init[IX_REF_IDX + 1] = v.ref_idx[1]; }
  slice_residual_init_values(slice_type, init + IX_RES);
  for (int i = 0; i < IX_COUNT; i++) m->ctx_init[i] = (uint8_t)inter_ctx_state(qp, init[i]);
  for (int l2 = 2; l2 <= 5; l2++)
    for (int c = 0; c < 2; c++) {
      m->qf[c][l2 - 2] = quant_scalars(qp, 8, 0 /* B and P slices: rounding 85, the non-intra one */, 0, 1 << l2, c ? 2 : 0);
      m->qi[c][l2 - 2] = quant_scalars(qp, 8, 0, scaling_list, 1 << l2, c ? 2 : 0);
    }
  memcpy(m->fbits, fbits, sizeof m->fbits);
}

// The ticket list of a launch (kvz_inter_kernels.hpp InterSched::items, picture << 16 | y << 8 | x): anti-diagonals x + 2 y ascending (raster order per picture
// without WPP), pictures interleaved -- consecutive tickets belong to different pictures
inline void inter_ticket_items(int wc, int hc, int n_pictures, int no_wpp, std::vector<uint32_t> &items)
{
  items.clear();
  items.reserve((size_t)wc * hc * n_pictures);
  if (no_wpp) {
    for (int y = 0; y < hc; y++) for (int x = 0; x < wc; x++) for (int f = 0; f < n_pictures; f++) items.push_back((uint32_t)f << 16 | (uint32_t)y << 8 | (uint32_t)x);
  } else {
    for (int d = 0; d <= (wc - 1) + 2 * (hc - 1); d++)
      for (int y = 0; y < hc; y++) { const int x = d - 2 * y; if (x < 0 || x >= wc) continue; for (int f = 0; f < n_pictures; f++) items.push_back((uint32_t)f << 16 | (uint32_t)y << 8 | (uint32_t)x); }
  }
}

// The table of a launch whose pictures have a QP and a POC of their own, as the device holds it (InterFrames::pictures): n InterPicture records, then one InterModel
// row per distinct QP.  init_row(m, qp): the launch's model at that QP (inter_model_init with the launch's parameters).  The caller copies `image` to the device as
// it is: the records address their rows relative to the image's first byte.
struct InterPictureTable {
  std::vector<uint64_t> image;
  int n_rows = 0;
  bool any_cabac = false;  // some picture prices coefficients with the residual coder: the launch takes the kernel build that holds its contexts
  size_t record_bytes = sizeof(InterPicture);  // (sizeof(InterPictureLists) in a launch with scaling lists; either record starts with model_at)
  size_t bytes() const { return image.size() * sizeof(uint64_t); }
  // the row of a picture in a copy of the image that starts at `base` (the device's, or the image itself)
  const InterModel *model_of_picture(const void *base, int picture) const { return (const InterModel *)((const uint8_t *)base + ((const InterPicture *)((const uint8_t *)image.data() + (size_t)picture * record_bytes))->model_at); }
};
template <class InitRow> inline InterPictureTable inter_picture_table(const int32_t *qp, const int32_t *poc, int n_pictures, const InitRow &init_row)
{
  static_assert(sizeof(InterPicture) == 8 && alignof(InterModel) <= 8 && sizeof(InterModel) % 8 == 0, "records and rows share a buffer of 8-byte words");
  InterPictureTable t;
  int row_of_qp[52], qp_of_row[52];
  t.n_rows = inter_qp_rows(qp, n_pictures, row_of_qp, qp_of_row);
  const size_t rows_at = (size_t)n_pictures * sizeof(InterPicture);
  t.image.assign((rows_at + (size_t)t.n_rows * sizeof(InterModel)) / sizeof(uint64_t), 0);
  uint8_t *base = (uint8_t *)t.image.data();
  for (int r = 0; r < t.n_rows; r++) {
    InterModel *m = (InterModel *)(base + rows_at) + r;
    init_row(m, qp_of_row[r]);
    t.any_cabac = t.any_cabac || m->coeff_cabac;
  }
  for (int i = 0; i < n_pictures; i++) ((InterPicture *)base)[i] = InterPicture{ (uint32_t)(rows_at + (size_t)row_of_qp[qp[i]] * sizeof(InterModel)), poc[i] };
  return t;
}

// ... and of a launch of P pictures with reference lists (kvz_hip_dev_inter_ctu_pass_refs; checked by inter_refs_launch_known): n InterPictureRefs records -- the
// picture's list as pool frames and the scales of every vector it can meet (kvz_inter_refs.hpp inter_refs_record) --, then the InterModel rows.  init_row must make
// its rows for a launch with lists of references (inter_model_init's refs).
template <class InitRow> inline InterPictureTable inter_picture_table_refs(const int32_t *qp, const int32_t *poc, int n_pictures, const InitRow &init_row, const kvz_hip_inter_refs *refs)
{
  static_assert(sizeof(InterPictureRefs) == 128, "records and rows share a buffer of 8-byte words");
  InterPictureTable t;
  t.record_bytes = sizeof(InterPictureRefs);
  int row_of_qp[52], qp_of_row[52];
  t.n_rows = inter_qp_rows(qp, n_pictures, row_of_qp, qp_of_row);
  const size_t rows_at = (size_t)n_pictures * sizeof(InterPictureRefs);
  t.image.assign((rows_at + (size_t)t.n_rows * sizeof(InterModel)) / sizeof(uint64_t), 0);
  uint8_t *base = (uint8_t *)t.image.data();
  for (int r = 0; r < t.n_rows; r++) {
    InterModel *m = (InterModel *)(base + rows_at) + r;
    init_row(m, qp_of_row[r]);
    t.any_cabac = t.any_cabac || m->coeff_cabac;
  }
  for (int i = 0; i < n_pictures; i++) ((InterPictureRefs *)base)[i] = InterPictureRefs{ (uint32_t)(rows_at + (size_t)row_of_qp[qp[i]] * sizeof(InterModel)), poc[i], inter_refs_record(refs, i, poc[i]), 0u };
  return t;
}

// ... and of a launch with scaling lists (kvz_hip_dev_inter_ctu_pass_lists; checked by scaling_list_sets_known): n InterPictureLists records, the InterModel rows, then
// the factor table -- six rows (qp % 6) of KVZ_LIST_ROW_INTER words per set, the sets in order, the flat list behind them (scaling_list_rows_inter) -- and every
// record's two rows of it: those of the picture's set, or of the flat list (set 0xffff), at its luma and its chroma QP (scaling_list_row; the byte offsets fit 32 bits for every n_sets the check accepts).
// set_of_picture == nullptr: set 0 for every picture.  init_row must make its rows for a launch with lists (inter_model_init's scaling_list).
template <class InitRow> inline InterPictureTable inter_picture_table_lists(const int32_t *qp, const int32_t *poc, int n_pictures, const InitRow &init_row,
                                                                            const kvz_hip_scaling_lists *sets, int n_sets, const uint16_t *set_of_picture)
{
  static_assert(sizeof(InterPictureLists) == 16, "records and rows share a buffer of 8-byte words");
  InterPictureTable t;
  t.record_bytes = sizeof(InterPictureLists);
  int row_of_qp[52], qp_of_row[52];
  t.n_rows = inter_qp_rows(qp, n_pictures, row_of_qp, qp_of_row);
  const size_t rows_at = (size_t)n_pictures * sizeof(InterPictureLists), lists_at = rows_at + (size_t)t.n_rows * sizeof(InterModel), row_bytes = KVZ_LIST_ROW_INTER * sizeof(uint32_t);
  t.image.assign((lists_at + (size_t)(n_sets + 1) * 6 * row_bytes) / sizeof(uint64_t), 0);
  uint8_t *base = (uint8_t *)t.image.data();
  for (int r = 0; r < t.n_rows; r++) {
    InterModel *m = (InterModel *)(base + rows_at) + r;
    init_row(m, qp_of_row[r]);
    t.any_cabac = t.any_cabac || m->coeff_cabac;
  }
  for (int k = 0; k <= n_sets; k++) scaling_list_rows_inter(k < n_sets ? &sets[k] : nullptr, (uint32_t *)(base + lists_at) + (size_t)k * 6 * KVZ_LIST_ROW_INTER);
  for (int i = 0; i < n_pictures; i++) {
    const int set = set_of_picture ? set_of_picture[i] : 0;
    const size_t row_y = scaling_list_row(set, n_sets, qp[i]), row_c = scaling_list_row(set, n_sets, scaled_qp(2, qp[i], 0));
    ((InterPictureLists *)base)[i] = InterPictureLists{ (uint32_t)(rows_at + (size_t)row_of_qp[qp[i]] * sizeof(InterModel)), poc[i], (uint32_t)(lists_at + row_y * row_bytes),
                                                        (uint32_t)(lists_at + row_c * row_bytes) };
  }
  return t;
}

}  // namespace kvz
