/*
 * kvz_oracle.h -- TEST INFRASTRUCTURE.  CPU restatement of kvazaar's strategy hot path.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library;
 * the product (kvazaar_amd/, libkvz_hip.so) never links, imports or calls it.
 *
 * Every function restates, in plain C, what the reference's *generic* strategy computes
 * (the files under src/strategies/generic/ of ultravideo/kvazaar v2.3.2); each definition in kvz_oracle.c cites
 * the file:line it follows.  Signatures mirror include/kvz_hip.h one-to-one (prefix kvz_oracle_
 * instead of kvz_hip_) so the parity tests can call oracle, reference build (oracle/_ref) and the
 * HIP library with identical arguments.
 *
 * Pinning: tests/test_oracle_*.py check this file against (a) the golden values of the
 * reference's own unit tests (tests/satd_tests.c, sad_tests.c, intra_sad_tests.c, dct_tests.c,
 * coeff_sum_tests.c) and (b) the compiled reference itself (oracle/_ref/libkvazaar_ref.so, generic
 * AND avx2 function pointers) on seeded random and adversarial inputs.
 */
#ifndef KVZ_ORACLE_H_
#define KVZ_ORACLE_H_

#include "../include/kvz_hip_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- tables (generated, verified against the reference's exported tables) ---- */
const int16_t *kvz_oracle_dct_matrix(int n);               /* n in {4,8,16,32}: row-major n*n */
const int16_t *kvz_oracle_dst_matrix(void);                /* 4x4 */
const uint32_t *kvz_oracle_scan_table(int scan_idx, int log2_size); /* scan 0 diag,1 hor,2 ver; log2 1..5 */

/* ---- picture ---- */
unsigned kvz_oracle_reg_sad(const uint8_t *d1, const uint8_t *d2, int w, int h, unsigned s1, unsigned s2);
unsigned kvz_oracle_sad_nxn(int n, const uint8_t *b1, const uint8_t *b2);
unsigned kvz_oracle_satd_nxn(int n, const uint8_t *b1, const uint8_t *b2);
void     kvz_oracle_sad_nxn_dual(int n, const uint8_t *preds /* 2 x 1024 */, const uint8_t *orig,
                                 unsigned num_modes, unsigned *costs_out);
void     kvz_oracle_satd_nxn_dual(int n, const uint8_t *preds /* 2 x 1024 */, const uint8_t *orig,
                                  unsigned num_modes, unsigned *costs_out);
unsigned kvz_oracle_satd_any_size(int w, int h, const uint8_t *b1, int s1, const uint8_t *b2, int s2);
void     kvz_oracle_satd_any_size_quad(int w, int h, const uint8_t *const *preds, int stride,
                                       const uint8_t *orig, int orig_stride, unsigned num_modes,
                                       unsigned *costs_out, int8_t *valid);
unsigned kvz_oracle_pixels_calc_ssd(const uint8_t *ref, const uint8_t *rec, int ref_stride, int rec_stride, int width);
uint32_t kvz_oracle_ver_sad(const uint8_t *pic, const uint8_t *ref, int32_t bw, int32_t bh, uint32_t pic_stride);
uint32_t kvz_oracle_hor_sad(const uint8_t *pic, const uint8_t *ref, int32_t w, int32_t h, uint32_t pic_stride,
                            uint32_t ref_stride, uint32_t left, uint32_t right);
double   kvz_oracle_pixel_var(const uint8_t *buf, uint32_t len);
/* One plane of bipred_average: exactly one of (px0, im0) and one of (px1, im1) is non-NULL. */
void     kvz_oracle_bipred_average_plane(uint8_t *dst, unsigned dst_stride, const uint8_t *px0, const int16_t *im0,
                                         const uint8_t *px1, const int16_t *im1, unsigned w, unsigned h);

/* Frame-edge SAD (image.c:407 kvz_image_calc_sad): SAD of the bw x bh block of `pic` at (pic_x,pic_y) against
 * `ref` at (ref_x,ref_y) with edge replication outside the ref_w x ref_h frame. */
unsigned kvz_oracle_image_calc_sad(const uint8_t *pic, int pic_stride, const uint8_t *ref, int ref_w, int ref_h,
                                   int ref_stride, int pic_x, int pic_y, int ref_x, int ref_y, int bw, int bh);

/* ---- dct ---- */
void kvz_oracle_transform(int kind, int8_t bitdepth, const int16_t *in, int16_t *out);

/* ---- quant ---- */
void kvz_oracle_quant(const kvz_hip_quant_params *p, const int16_t *coef, int16_t *q_coef, int32_t width,
                      int32_t height, int8_t type, int8_t scan_idx, int8_t block_type);
void kvz_oracle_dequant(const kvz_hip_quant_params *p, const int16_t *q_coef, int16_t *coef, int32_t width,
                        int32_t height, int8_t type, int8_t block_type);
int  kvz_oracle_quantize_residual(const kvz_hip_quant_params *p, int width, int color, int scan_order,
                                  int use_trskip, int in_stride, int out_stride, const uint8_t *ref_in,
                                  const uint8_t *pred_in, uint8_t *rec_out, int16_t *coeff_out, int early_skip);
void kvz_oracle_plane_md5(const uint8_t *data, int height, int width, int stride, uint8_t *out16);  /* nal-generic.c:41-55 (RFC 1321) */
uint32_t kvz_oracle_plane_checksum(const uint8_t *data, int height, int width, int stride);  /* nal-generic.c:57-82 */
uint32_t kvz_oracle_coeff_abs_sum(const int16_t *coeffs, size_t length);
double   kvz_oracle_fast_coeff_cost(const int16_t *coeff, int32_t width, uint64_t weights);
/* find_last_scanpos: returns through the same out-pointers as the reference; sig_coeff_inc_out is the
 * sh_rates->sig_coeff_inc array (int32 per coefficient), only the entry at the found blkpos is written. */
void kvz_oracle_find_last_scanpos(const int16_t *coef, int16_t *dest_coeff, int8_t type, int32_t q_bits,
                                  const int16_t *quant_coeff, int32_t *sig_coeff_inc_out, uint32_t cg_size,
                                  uint16_t *ctx_set, const uint32_t *scan, int32_t *cg_last_scanpos,
                                  int32_t *last_scanpos, uint32_t cg_num, int32_t *cg_scanpos, int32_t width,
                                  int8_t scan_mode);
int32_t kvz_oracle_get_scaled_qp(int8_t type, int8_t qp, int8_t qp_offset);

/* ---- intra ---- */
void kvz_oracle_angular_pred(int log2_width, int intra_mode, const uint8_t *ref_above, const uint8_t *ref_left, uint8_t *dst);
void kvz_oracle_intra_pred_planar(int log2_width, const uint8_t *ref_top, const uint8_t *ref_left, uint8_t *dst);
void kvz_oracle_intra_pred_filtered_dc(int log2_width, const uint8_t *ref_top, const uint8_t *ref_left, uint8_t *dst);

/* ---- ipol ---- */
void kvz_oracle_sample_quarterpel_luma(const uint8_t *src, int16_t src_stride, int w, int h, uint8_t *dst,
                                       int16_t dst_stride, int8_t hor_flag, int8_t ver_flag, const int16_t mv[2]);
void kvz_oracle_sample_quarterpel_luma_hi(const uint8_t *src, int16_t src_stride, int w, int h, int16_t *dst,
                                          int16_t dst_stride, int8_t hor_flag, int8_t ver_flag, const int16_t mv[2]);
void kvz_oracle_sample_octpel_chroma(const uint8_t *src, int16_t src_stride, int w, int h, uint8_t *dst,
                                     int16_t dst_stride, int8_t hor_flag, int8_t ver_flag, const int16_t mv[2]);
void kvz_oracle_sample_octpel_chroma_hi(const uint8_t *src, int16_t src_stride, int w, int h, int16_t *dst,
                                        int16_t dst_stride, int8_t hor_flag, int8_t ver_flag, const int16_t mv[2]);
/* The four FME block filters.  filtered = 4 planes of 64*64 u8 (stride 64); hor_intermediate = 5 planes of
 * KVZ_HIP_IPOL_IM_PLANE int16; hor_first_cols = 5 rows of KVZ_HIP_IPOL_COL_LEN int16.  State carried between
 * calls (hpel hor_ver -> hpel diag -> qpel hor_ver -> qpel diag) lives in those caller buffers exactly as in
 * the reference. */
#define KVZ_HIP_IPOL_IM_PLANE ((64 + 7 + 1) * 64 + 1)   /* KVZ_IPOL_MAX_IM_SIZE_LUMA_SIMD, strategies-ipol.h:54 */
#define KVZ_HIP_IPOL_COL_LEN  (64 + 7 + 1)              /* KVZ_EXT_BLOCK_W_LUMA + 1 */
void kvz_oracle_filter_hpel_blocks_hor_ver_luma(const uint8_t *src, int16_t src_stride, int w, int h, uint8_t *filtered,
                                                int16_t *hor_intermediate, int8_t fme_level, int16_t *hor_first_cols,
                                                int8_t hpel_off_x, int8_t hpel_off_y);
void kvz_oracle_filter_hpel_blocks_diag_luma(const uint8_t *src, int16_t src_stride, int w, int h, uint8_t *filtered,
                                             int16_t *hor_intermediate, int8_t fme_level, int16_t *hor_first_cols,
                                             int8_t hpel_off_x, int8_t hpel_off_y);
void kvz_oracle_filter_qpel_blocks_hor_ver_luma(const uint8_t *src, int16_t src_stride, int w, int h, uint8_t *filtered,
                                                int16_t *hor_intermediate, int8_t fme_level, int16_t *hor_first_cols,
                                                int8_t hpel_off_x, int8_t hpel_off_y);
void kvz_oracle_filter_qpel_blocks_diag_luma(const uint8_t *src, int16_t src_stride, int w, int h, uint8_t *filtered,
                                             int16_t *hor_intermediate, int8_t fme_level, int16_t *hor_first_cols,
                                             int8_t hpel_off_x, int8_t hpel_off_y);
/* get_extended_block: returns 1 and fills buf (stride = pad_l+blk_w+pad_r) when the window leaves the frame,
 * returns 0 when the reference would hand back a pointer into the frame. */
int kvz_oracle_get_extended_block(const kvz_hip_epol_params *a, const uint8_t *src, uint8_t *buf);

/* ---- sao ---- */
int  kvz_oracle_sao_edge_ddistortion(int bitdepth, const uint8_t *orig, const uint8_t *rec, int bw, int bh,
                                     int eo_class, const int offsets[5]);
void kvz_oracle_calc_sao_edge_dir(int bitdepth, const uint8_t *orig, const uint8_t *rec, int eo_class, int bw,
                                  int bh, int cat_sum_cnt[10] /* [2][5], accumulated */);
void kvz_oracle_sao_reconstruct_color(const kvz_hip_sao_params *sao, const uint8_t *rec /* may be read at -1 row/col */,
                                      uint8_t *new_rec, int stride, int new_stride, int bw, int bh, int color);
void kvz_oracle_sao_frame(int width, int height, const uint8_t *in, uint8_t *out, const kvz_hip_sao_params *luma,
                          const kvz_hip_sao_params *chroma);  /* sao.c:302-361 for every CTU and plane */
int  kvz_oracle_sao_band_ddistortion(int bitdepth, const uint8_t *orig, const uint8_t *rec, int bw, int bh,
                                     int band_pos, const int sao_bands[4]);

/* ---- batched all-intra CTU pass (kvz_oracle_ctu.c) ---- */
void kvz_oracle_intra_frame(const kvz_hip_intra_cost_model *m, int width, int height, const uint8_t *src_y, const uint8_t *src_u,
                            const uint8_t *src_v, uint8_t *rec_y, uint8_t *rec_u, uint8_t *rec_v, int16_t *coeff, uint8_t *cu_depth,
                            uint8_t *cu_mode, double *ctu_cost);
void kvz_oracle_intra_frame_nxn(const kvz_hip_intra_cost_model *m, int width, int height, const uint8_t *src_y, const uint8_t *src_u,
                            const uint8_t *src_v, uint8_t *rec_y, uint8_t *rec_u, uint8_t *rec_v, int16_t *coeff, uint8_t *cu_depth,
                            uint8_t *cu_mode, double *ctu_cost, uint8_t *cu_part, uint8_t *cu_mode4);
void kvz_oracle_intra_cost_model(int qp, const float entropy_fbits[128], uint64_t coeff_weights, kvz_hip_intra_cost_model *m);
double kvz_oracle_coeff_cabac_bits(const float entropy_fbits[128], const int16_t *coeff, int width, int type, int scan_mode, int update, uint8_t *ctx);
const uint8_t *kvz_oracle_next_state_table(int lps);  /* cabac.c:40-62, regenerated from H.265 Table 9-41 */

/* ---- rate-distortion optimised quantisation of one intra transform block (kvz_oracle_rdoq.c; rdo.c:661 kvz_rdoq) ----
 * ctx_states: uc_state of the contexts in KVZ_HIP_CX_* order (state->cabac.ctx of the encoder); entropy_fbits: kvz_f_entropy_bits; type 0 luma / 2 chroma */
void kvz_oracle_rdoq(int qp, double lambda, const uint8_t *ctx_states, const float *entropy_fbits, const int16_t *coef, int16_t *dest, int width, int type,
                     int scan_mode, int tr_depth);

/* ---- SAO parameter decision of a whole picture in the encoder's LCU order (kvz_oracle_sao.c; sao.c:671 kvz_sao_search_lcu) ----
 * src = the original picture, rec = the reconstruction BEFORE deblocking (Y|U|V tight), deblocked in place LCU by LCU when `deblock`
 * (the statistics see the partly deblocked picture the encoder has at that moment); on return rec is the deblocked, pre-SAO picture.
 * luma_out / chroma_out / merge_out: one record per LCU in raster order; merge: 0 none, 1 left, 2 up. */
void kvz_oracle_sao_search_frame(const kvz_hip_intra_cost_model *m, int width, int height, const uint8_t *src, uint8_t *rec, const uint8_t *cu_depth,
                                 int deblock, int beta_offset_div2, int tc_offset_div2, kvz_hip_sao_params *luma_out, kvz_hip_sao_params *chroma_out,
                                 uint8_t *merge_out);
void kvz_oracle_deblock_frame_passes(int width, int height, int qp, int beta_offset_div2, int tc_offset_div2, uint8_t *y, uint8_t *u, uint8_t *v,
                                     const uint8_t *cu_depth, int passes);
#include "../include/kvz_hip_dev.h" /* kvz_hip_cu_dbk */
void kvz_oracle_deblock_frame_inter(int width, int height, int qp, int beta_offset_div2, int tc_offset_div2, uint8_t *y, uint8_t *u, uint8_t *v,
                                    const kvz_hip_cu_dbk *info, int slice_is_b);  /* filter.c:405-493 boundary strengths from motion data */
void kvz_oracle_deblock_lcu(int width, int height, int qp, int beta_offset_div2, int tc_offset_div2, uint8_t *y, uint8_t *u, uint8_t *v,
                            const uint8_t *cu_depth, int x_px, int y_px);
void kvz_oracle_deblock_lcu_inter(int width, int height, int qp, int beta_offset_div2, int tc_offset_div2, uint8_t *y, uint8_t *u, uint8_t *v,
                                  const kvz_hip_cu_dbk *info, int slice_is_b, int x_px, int y_px);
void kvz_oracle_sao_search_frame_inter(const kvz_hip_intra_cost_model *m, int width, int height, const uint8_t *src, uint8_t *rec, const kvz_hip_cu_dbk *info,
                                       int slice_is_b, int deblock, int beta_offset_div2, int tc_offset_div2, kvz_hip_sao_params *luma_out,
                                       kvz_hip_sao_params *chroma_out, uint8_t *merge_out);

/* ---- sequences with inter prediction (kvz_oracle_inter.inc, part of kvz_oracle_ctu.c): an I picture followed by B pictures that each reference the previous
 * one in both lists -- `--gop lp-g<gop_len>d<gop_depth>t1` with the `ultrafast` .. `faster` presets (BASELINE config 4 is `veryfast`) ---- */
typedef struct kvz_oracle_cu {  /* cu_info_t (cu.h:130-170) of one 4x4 unit */
  uint8_t type /* 0 not set, 1 intra, 2 inter */, depth, mode /* intra */, tr_depth; uint16_t cbf;
  uint8_t skipped, merged, merge_idx, mv_dir, mv_ref[2], mv_cand[2];  /* motion fields of a list mv_dir does not use: 0 / 255 */
  int16_t mv[2][2];
} kvz_oracle_cu;
typedef struct kvz_oracle_lowdelay_cfg {
  int32_t qp;                  /* --qp */
  int32_t gop_len, gop_depth;  /* lp-g<len>d<depth>t1 */
  int32_t intra_period;        /* --period (64) */
  int32_t fme_level;           /* --subme: 4 `faster`, 2 `veryfast`, 0 `ultrafast` */
  int32_t pu_depth_inter_max;  /* 3 `veryfast`, 2 `ultrafast` */
  int32_t sao, deblock;        /* --sao full / off, --deblock / --no-deblock */
  int32_t mv_constraint;       /* cfg.owf && cfg.wpp (search_inter.c:85) */
  int32_t no_wpp;
  int32_t ra8_qp_model;        /* a --preset came before --gop lp-...: the QP model fields of kvz_gop_ra8 stay in the GOP entries (kvz_oracle_lowdelay_qp) */
  int32_t fast_residual_cost;  /* --fast-residual-cost: 28 `ultrafast` .. `veryfast`, 0 `faster` (coefficients priced with the CABAC model at every QP; rdo.c:311-340) */
} kvz_oracle_lowdelay_cfg;
/* the motion search of single PUs on caller-supplied candidates (the contract of kvz_hip_dev_pu_search, include/kvz_hip_dev.h), and a recorder of every such
 * search the sequence encoder runs: inputs, results and the picture they belong to */
void kvz_oracle_pu_motion_search(const uint8_t *cur, const uint8_t *ref, int width, int height, const kvz_hip_me_pu *pus, int count, const kvz_hip_me_params *prm,
                                 kvz_hip_me_result *out);
void kvz_oracle_me_trace(kvz_hip_me_pu *pus, kvz_hip_me_result *res, int32_t *poc, int capacity);
int  kvz_oracle_me_trace_count(void);
int  kvz_oracle_lowdelay_qp(int qp, int gop_len, int gop_depth, int frame, int intra_period, int ra8_model);
void kvz_oracle_lowdelay_encode(const kvz_oracle_lowdelay_cfg *cfg, const float entropy_fbits[128], const uint64_t coeff_weights[52], int width, int height,
                                int n_frames, const uint8_t *src, uint8_t *rec_search, uint8_t *rec_final, kvz_oracle_cu *cu_out, int32_t *frame_qp);
/* ... and the slice data of every picture (kvz_oracle_entropy.inc): the substreams of all pictures back to back, their sizes (n_frames x (CTU rows | 1)), and where every
 * picture's begin (n_frames + 1 offsets) */
void kvz_oracle_lowdelay_encode_bits(const kvz_oracle_lowdelay_cfg *cfg, const float entropy_fbits[128], const uint64_t coeff_weights[52], int width, int height,
                                     int n_frames, const uint8_t *src, uint8_t *rec_final, kvz_oracle_cu *cu_out, uint8_t *slice_data, size_t slice_capacity,
                                     uint32_t *substream_bytes, uint64_t *picture_offsets);
/* ... what an entropy coder needs of every picture besides the CU records (levels of every CTU, SAO decisions), and the initial context states of a B slice (CX order:
 * KVZ_HIP_CX_*, then skip[3] 150, merge flag 153, merge idx 154, pred mode 155, mvd[2] 156, mvp idx 158, inter dir[5] 160, root cbf 165) */
void kvz_oracle_lowdelay_encode_parts(const kvz_oracle_lowdelay_cfg *cfg, const float entropy_fbits[128], const uint64_t coeff_weights[52], int width, int height,
                                      int n_frames, const uint8_t *src, kvz_oracle_cu *cu_out, int16_t *coeff_out, kvz_hip_sao_params *sao_luma, kvz_hip_sao_params *sao_chroma,
                                      uint8_t *sao_merge, int32_t *frame_qp);
void kvz_oracle_b_slice_contexts(int qp, uint8_t out[172]);
/* one B picture of such a sequence on its own, from its reference picture (after the loop filters) and that picture's CU records: qp / poc are the picture's;
 * of cfg the search options are read (fme_level, pu_depth_inter_max, sao, deblock, mv_constraint, no_wpp).  coeff (or NULL): KVZ_HIP_CTU_COEFFS per CTU. */
void kvz_oracle_inter_picture(int qp, int poc, const kvz_oracle_lowdelay_cfg *cfg, const float entropy_fbits[128], uint64_t coeff_weights, int width, int height,
                              const uint8_t *src, const uint8_t *ref, const kvz_oracle_cu *ref_cu, uint8_t *rec, kvz_oracle_cu *cu, int16_t *coeff);

/* ---- the entropy coder in its real mode (kvz_oracle_entropy.inc): the slice data kvazaar writes for an I picture -- one substream per CTU row with WPP, one for the
 * picture without -- from what the CTU pass returns: CU depth / luma mode per 8x8, NxN flags per 8x8 and PU modes per 4x4 (or NULL), KVZ_HIP_CTU_COEFFS levels per CTU,
 * and the SAO decisions (or NULL: SAO off; merge 0 none / 1 left / 2 up).  m: qp, ctx_init, no_wpp.  Returns the total size; substream_bytes: one entry per substream. ---- */
size_t kvz_oracle_entropy_intra_picture(const kvz_hip_intra_cost_model *m, int width, int height, const uint8_t *cu_depth, const uint8_t *cu_mode, const uint8_t *part,
                                        const uint8_t *mode4, const int16_t *coeff, const kvz_hip_sao_params *sao_luma, const kvz_hip_sao_params *sao_chroma,
                                        const uint8_t *sao_merge, uint8_t *out, size_t capacity, uint32_t *substream_bytes);
size_t kvz_oracle_entropy_intra_tile(const kvz_hip_intra_cost_model *m, int width, int height, const uint8_t *cu_depth, const uint8_t *cu_mode, const uint8_t *part,
                                     const uint8_t *mode4, const int16_t *coeff, const kvz_hip_sao_params *sao_luma, const kvz_hip_sao_params *sao_chroma,
                                     const uint8_t *sao_merge, int not_last, uint8_t *out, size_t capacity, uint32_t *substream_bytes);

/* ... and for a B picture of a low-delay sequence from its CU records (one per 4x4 unit), the reference picture's records (temporal MV predictors, from POC 2 on) and
 * its levels: what kvz_hip_dev_entropy_code_inter reads, without a search in front.  sao_*: NULL (SAO off) or one record per LCU. */
size_t kvz_oracle_entropy_b_picture(int qp, int poc, int no_wpp, int width, int height, const kvz_oracle_cu *cu, const kvz_oracle_cu *ref_cu, const int16_t *coeff,
                                    const kvz_hip_sao_params *sao_luma, const kvz_hip_sao_params *sao_chroma, const uint8_t *sao_merge, uint8_t *out, size_t capacity,
                                    uint32_t *substream_bytes);

/* the per-call form (strategies-encode.h:49-65): one block's residual syntax as bin records (include/kvz_hip.h kvz_hip_coeff_nxn_bins), and records through the
 * arithmetic coder from given context states (KVZ_HIP_CX_* order; 150 of them) + flush + stop bit + alignment */
int kvz_oracle_coeff_nxn_bins(const int16_t *coeff, int width, int type, int scan_mode, uint32_t *records, int capacity);
int kvz_oracle_code_records(const uint8_t *ctx_states, const uint32_t *records, int n, uint8_t *out, int capacity);

/* ---- deblocking of an all-intra, constant-QP picture in place (kvz_oracle_deblock.c; filter.c:783 kvz_filter_deblock_lcu over
 * every LCU).  Planes are tight (stride = width), cu_depth is the CU depth per 8x8 unit as the CTU pass returns it. ---- */
void kvz_oracle_deblock_frame(int width, int height, int qp, int beta_offset_div2, int tc_offset_div2, uint8_t *y, uint8_t *u, uint8_t *v,
                              const uint8_t *cu_depth);

#ifdef __cplusplus
}
#endif
#endif
