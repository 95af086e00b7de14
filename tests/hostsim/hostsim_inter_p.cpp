// hostsim_inter_p.cpp -- TEST INFRASTRUCTURE (see hostsim.cpp and hostsim_inter_models.cpp, which this unit includes whole: one library with everything of
// libkvz_hostsim_inter_models.so plus the twins of the entry points that take a slice type).  The device compiles the inter program with KVZ_ICTU_P 0 and 1; here the
// switch is a variable (as hostsim_inter_me.cpp has KVZ_ICTU_ME), so that this one library holds both forms of the same text -- the B program behind every entry
// point of the units it includes and behind KVZ_HIP_SLICE_B, the P program behind KVZ_HIP_SLICE_P.  The slice type is checked by the text the library checks it
// with (kvz_inter_host.hpp inter_slice_launch_known), the initial context states of the search and of the coder are the rows the library fills
// (inter_model_init, kvz_slice_contexts.hpp entropy_slice_contexts).  It also counts what the P pictures' decisions were (the census of
// tests/golden/inter_p.json).  tests/test_inter_p_sim.py, tests/test_gpu_inter_p.py and tests/golden/make_inter_p_golden.py build and use it.
#include <map>
static int g_kvz_ictu_p = 0;
#define KVZ_ICTU_P g_kvz_ictu_p
// where the entries of a PU's merge list came from, by picture of the launch and PU: n_spatial | n_temporal << 4 | (first zero entry) << 8
static std::map<unsigned long long, unsigned> g_p_merge_origin;
static inline unsigned long long p_origin_key(int picture, int x, int y, int w) { return (unsigned long long)picture << 40 | (unsigned long long)(x >> 3) << 24 | (unsigned long long)(y >> 3) << 8 | (unsigned)w; }
#define IC_MERGE_ORIGIN(x, y, w, n_spatial, n_temporal, n_zero_from) (g_p_merge_origin[p_origin_key(frame, (x), (y), (w))] = (unsigned)(n_spatial) | (unsigned)(n_temporal) << 4 | (unsigned)(n_zero_from) << 8)
#include "hostsim_inter_models.cpp"
#include "../../kvazaar_amd/csrc/kvz_slice_contexts.hpp"

// the twins of the argument checks the three entry points add to those of their _pictures twins: 0 accepted, -1 refused with the library's message.
// stage 0: kvz_hip_dev_inter_ctu_pass_slices, 1: kvz_hip_dev_loop_filters_inter_slices, 2: kvz_hip_dev_entropy_code_inter_slices
extern "C" int kvz_hostsim_inter_slices_check(const kvz_hip_inter_params *p, int has_tile_xy, int slice_type, int stage)
{
  if (stage == 1) {
    if (slice_type == KVZ_HIP_SLICE_B || slice_type == KVZ_HIP_SLICE_P || slice_type == KVZ_HIP_SLICE_I) return 0;
    fprintf(stderr, "kvz_hip_dev_loop_filters_inter_slices: slice type %d is none of KVZ_HIP_SLICE_B (0), KVZ_HIP_SLICE_P (1), KVZ_HIP_SLICE_I (2)\n", slice_type);
    return -1;
  }
  kvz_hip_inter_params full;
  const char *who = stage == 0 ? "kvz_hip_dev_inter_ctu_pass_slices" : "kvz_hip_dev_entropy_code_inter_slices";
  if (!kvz::inter_params_full(p, &full, who)) return -1;
  return kvz::inter_slice_launch_known(&full, stage == 0 && has_tile_xy, slice_type, who) ? 0 : -1;
}

// the initial states of a slice type at a QP in the coder's numbering (KVZ_ENTROPY_CTXS of them), and the value the SAO decision's sao_type_idx context starts from
extern "C" void kvz_hostsim_slice_contexts(int slice_type, int qp, uint8_t *out) { kvz::entropy_slice_contexts(slice_type, qp, out); }
extern "C" int kvz_hostsim_sao_type_init_value(int slice_type) { return kvz::sao_type_init_value(slice_type); }

// kvz_hip_dev_inter_ctu_pass_slices on the host: the arguments of kvz_hostsim_inter_pass_pictures and the slice type.  Returns 0, or -1 for what the library refuses
// (nothing is computed then)
extern "C" int kvz_hostsim_inter_pass_slices(int width, int height, int n_pictures, const kvz_hip_inter_params *p, const kvz_hip_inter_pictures *pictures,
                                             const uint64_t *coeff_weights_of_qp, const float *fbits, const uint8_t *src, const uint8_t *ref, const kvz_hip_cu_info *ref_cu,
                                             uint8_t *rec, kvz_hip_cu_info *cu, int16_t *coeff, const int32_t *tile_xy, int n_references, int slice_type)
{
  kvz_hip_inter_params full;
  if (!kvz::inter_params_full(p, &full, "kvz_hip_dev_inter_ctu_pass")) return -1;
  p = &full;
  if (!kvz::inter_slice_launch_known(p, tile_xy != nullptr, slice_type, "kvz_hip_dev_inter_ctu_pass_slices")) return -1;
  if (pictures && !kvz::inter_pictures_known(pictures, n_pictures, "kvz_hostsim_inter_pass_slices")) return -1;
  if (kvz::inter_pass_geometry_refused(width, height, n_pictures, p->ref_width, p->ref_height, p->tile_x, p->tile_y)) return -1;
  if (!kvz::inter_me_known(p, (p->ref_width || p->ref_height || tile_xy) ? "tiles" : nullptr, "kvz_hip_dev_inter_ctu_pass")) return -1;
  if (slice_type == KVZ_HIP_SLICE_B) {
    if (kvz::inter_me_chosen(p)) { fprintf(stderr, "kvz_hostsim_inter_pass_slices: this library holds the default search only (tests/hostsim/hostsim_inter_me.cpp has the others)\n"); return -1; }
    return kvz_hostsim_inter_pass_pictures(width, height, n_pictures, p, pictures, coeff_weights_of_qp, fbits, src, ref, ref_cu, rec, cu, coeff, tile_xy, n_references);
  }
  static kvz::Tables tb;
  kvz::build_tables(&tb);
  auto model_at_qp = [&](kvz::InterModel *row, int qp) {
    kvz::inter_model_init(row, qp, p->poc, coeff_weights_of_qp[qp], fbits, p->mv_constraint, p->sao, p->deblock, p->fme_level, p->pu_depth_inter_max, p->no_wpp, p->fast_residual_cost,
                          width, height, 0, 0, 0, 0, p->no_tmvp, 0, slice_type);
  };
  kvz::InterPictureTable table;
  kvz::InterModel m;
  if (pictures) table = kvz::inter_picture_table(pictures->qp, pictures->poc, n_pictures, model_at_qp);
  else model_at_qp(&m, p->qp);
  kvz::InterFrames F;
  memset(&F, 0, sizeof F);
  F.W = width; F.H = height; F.wc = (width + 63) / 64; F.hc = (height + 63) / 64; F.frame_px = (long)width * height * 3 / 2; F.cells = (long)(width / 4) * (height / 4);
  F.src = src; F.ref = ref; F.ref_cu = ref_cu; F.rec = rec; F.cu = cu; F.coeff = coeff;
  F.ctx_out = (kvz::ICtx *)calloc((size_t)F.wc * F.hc * n_pictures, sizeof(kvz::ICtx));
  kvz::InterSlab *slab = (kvz::InterSlab *)calloc(1, sizeof(kvz::InterSlab));
  F.slabs = slab;
  F.ref_count = n_references > 0 ? n_references : 0;
  F.pictures = pictures ? (const kvz::InterPicture *)table.image.data() : nullptr;
  memset(cu, 0, (size_t)F.cells * n_pictures * sizeof(kvz_hip_cu_info));
  std::vector<uint32_t> items;
  kvz::inter_ticket_items(F.wc, F.hc, n_pictures, p->no_wpp, items);
  g_p_merge_origin.clear();
  g_kvz_ictu_p = 1;
  kvz::InterCtu::begin_launch(F, pictures ? table.model_of_picture(table.image.data(), 0) : &m, &tb, slab);
  for (const uint32_t item : items) {
    kvz::InterCtu::begin_ctu((int)(item >> 16), (int)(item & 0xff) * 64, (int)((item >> 8) & 0xff) * 64);
    kvz::InterCtu::run();
  }
  g_kvz_ictu_p = 0;
  free(F.ctx_out); free(slab);
  return 0;
}

// What the decisions of picture `picture` of the LAST kvz_hostsim_inter_pass_slices launch of P pictures were, CU by CU, from its records `cu` (the picture's own:
// (height / 4) x (width / 4)) and the origins of the merge lists the program built while it searched.  out[16]: 0 intra CUs, 1 skipped CUs, 2 merged CUs with index 0,
// 3 merged CUs with an index above 0, 4 a chosen temporal merge candidate, 5 a chosen zero merge candidate, 6 AMVP CUs with mvp_idx 0, 7 with mvp_idx 1, 8 fractional
// vectors, 9 / 10 / 11 CUs of depth 1 / 2 / 3, 12 inter CUs with residual, 13 root cbf 0 on a non-merged CU, 14 records whose mv_dir is not 1, 15 merged or skipped
// CUs whose merge list the program did not build (must be 0).  Counts are ADDED to out.
extern "C" void kvz_hostsim_p_census(const kvz_hip_cu_info *cu, int width, int height, int picture, unsigned long long *out)
{
  const int w4 = width >> 2;
  for (int y = 0; y < height; y += 8)
    for (int x = 0; x < width; x += 8) {
      const kvz_hip_cu_info &c = cu[(y >> 2) * w4 + (x >> 2)];
      const int w = 64 >> c.depth;
      if ((x & (w - 1)) || (y & (w - 1)) || (c.type != 1 && c.type != 2)) continue;
      if (c.depth >= 1 && c.depth <= 3) out[8 + c.depth]++;
      if (c.type == 1) { out[0]++; continue; }
      if (c.mv_dir != 1) out[14]++;
      if ((c.mv[0][0] | c.mv[0][1]) & 3) out[8]++;
      if (c.cbf) out[12]++;
      if (c.skipped) out[1]++;
      else if (c.merged) out[c.merge_idx == 0 ? 2 : 3]++;
      else { out[c.mv_cand[0] == 0 ? 6 : 7]++; if (!c.cbf) out[13]++; }
      if (c.skipped || c.merged) {
        const auto it = g_p_merge_origin.find(p_origin_key(picture, x, y, w));
        if (it == g_p_merge_origin.end()) { out[15]++; continue; }
        const int n_spatial = (int)(it->second & 15u), n_temporal = (int)((it->second >> 4) & 15u), zero_from = (int)(it->second >> 8);
        if (c.merge_idx >= n_spatial && c.merge_idx < n_temporal) out[4]++;
        if (c.merge_idx >= zero_from) out[5]++;
      }
    }
}

// kvz_hip_dev_entropy_code_inter_slices on the host: kvz_hostsim_entropy_code_inter_pictures with the slice type -- every picture's initial context states from the
// row of its QP and of the slice type, filled here as the library fills them, and no inter_pred_idc in a P slice.  qp_of_picture / poc_of_picture: [n_pictures]
// (a POC of 0: no temporal predictors).  Returns the bytes, -1 for a slice type the coder refuses or a CTU with more than `cap` records
extern "C" long kvz_hostsim_entropy_code_inter_slices(int slice_type, const int32_t *qp_of_picture, const int32_t *poc_of_picture, int width, int height, int n_pictures, int no_wpp,
                                                      const kvz_hip_cu_info *cu, const kvz_hip_cu_info *ref_cu, const int16_t *coeff, const unsigned long long *sao_recs,
                                                      const uint8_t *sao_merge, uint32_t cap, uint8_t *out, uint32_t *substream_bytes)
{
  if (!kvz::inter_slice_type_known(slice_type, "kvz_hip_dev_entropy_code_inter_slices")) return -1;
  if (!kvz::inter_picture_qps_known(qp_of_picture, n_pictures, "kvz_hostsim_entropy_code_inter_slices")) return -1;
  static kvz::Tables tb;
  kvz::build_tables(&tb);
  int row_of_qp[52], qp_of_row[52];
  const int n_rows = kvz::inter_qp_rows(qp_of_picture, n_pictures, row_of_qp, qp_of_row);
  std::vector<uint8_t> rows((size_t)n_rows * KVZ_ENTROPY_CTX_ROW, 0);
  for (int r = 0; r < n_rows; r++) kvz::entropy_slice_contexts(slice_type, qp_of_row[r], &rows[(size_t)r * KVZ_ENTROPY_CTX_ROW]);
  std::vector<uint16_t> row_of_picture((size_t)n_pictures);
  for (int i = 0; i < n_pictures; i++) row_of_picture[(size_t)i] = (uint16_t)row_of_qp[qp_of_picture[i]];
  kvz::EntropyJob J;
  memset(&J, 0, sizeof J);
  J.W = width; J.H = height; J.wc = (width + 63) / 64; J.hc = (height + 63) / 64; J.n_frames = n_pictures; J.no_wpp = no_wpp;
  J.cu = cu; J.ref_cu = ref_cu; J.coeff = coeff; J.sao = sao_recs; J.sao_merge = sao_merge;
  J.ctx_rows = rows.data(); J.model_of_picture = row_of_picture.data(); J.poc_of_picture = poc_of_picture;
  J.p_slice = slice_type == KVZ_HIP_SLICE_P;
  const long items = (long)n_pictures * J.wc * J.hc, streams = (long)n_pictures * (no_wpp ? 1 : J.hc);
  cap = (cap + 15u) & ~15u;
  J.bins = (uint32_t *)aligned_alloc(64, (size_t)items * cap * sizeof(uint32_t)); J.nbins = (uint32_t *)malloc((size_t)items * sizeof(uint32_t));
  J.nbits = (uint32_t *)malloc((size_t)items * sizeof(uint32_t)); J.cap = cap;
  J.row_ctx = (uint8_t *)malloc((size_t)n_pictures * J.hc * KVZ_ENTROPY_CTXS);
  const kvz::EntropyTabs T{ &tb.ctx_next[0][0] };
  uint8_t ctx[KVZ_ENTROPY_CTXS];
  long total = 0;
  for (long i = 0; i < items; i++) { hostsim_ctu_bins(J, &tb, i); if (J.nbins[i] > cap) total = -1; }
  if (total == 0) {
    if (!no_wpp) for (int f = 0; f < n_pictures; f++) kvz::entropy_row_contexts(J, T, f, ctx);
    const long per_stream = no_wpp ? (long)J.wc * J.hc : J.wc;
    for (long i = 0; i < streams; i++) {
      unsigned long long bits = 0;
      for (long k = 0; k < per_stream; k++) bits += J.nbits[i * per_stream + k];
      substream_bytes[i] = hostsim_code_row(J, tb, i, out + total, (size_t)(((bits + 7) / 8 + 16) * 3 / 2));
      total += substream_bytes[i];
    }
  }
  free(J.bins); free(J.nbins); free(J.nbits); free(J.row_ctx);
  return total;
}
