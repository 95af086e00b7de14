// hostsim_inter_refs.cpp -- TEST INFRASTRUCTURE (see hostsim.cpp and hostsim_inter_p.cpp, which this unit includes whole: one library with everything of
// libkvz_hostsim_inter_p.so plus the twins of the entry points that take reference lists).  The device compiles the P program with KVZ_ICTU_REFS 0 and 1; here
// the switch is a variable (as hostsim_inter_p.cpp has KVZ_ICTU_P), so that this one library holds every form of the same text.  The lists are checked by the text
// the library checks them with (kvz_inter_host.hpp inter_refs_launch_known), the picture table is the library's (inter_picture_table_refs), the scales are
// kvz_inter_refs.hpp's.  It also counts what the program met of the lists (the census of tests/golden/inter_refs.json).  tests/test_inter_refs_sim.py,
// tests/test_gpu_inter_refs.py and tests/golden/make_inter_refs_golden.py build and use it.
static int g_kvz_ictu_refs = 0;
#define KVZ_ICTU_REFS g_kvz_ictu_refs
// 0: a spatial AMVP candidate scaled, 1: a temporal candidate scaled with tb != td, 2: a zero merge candidate of a reference index above 0 evaluated
static unsigned long long g_refs_events[8];
#define IC_REFS_EVENT(slot) ((void)++g_refs_events[slot])
#include "hostsim_inter_p.cpp"

extern "C" void kvz_hostsim_refs_events(unsigned long long *out, int reset)
{
  for (int i = 0; i < 8; i++) { out[i] = g_refs_events[i]; if (reset) g_refs_events[i] = 0; }
}

// the scale of a pair of POC distances and a component scaled by it (kvz_inter_refs.hpp), as the pass and the coder use them
extern "C" int kvz_hostsim_mv_scale_of_distances(int diff_current, int diff_neighbor) { return kvz::mv_scale_of_distances(diff_current, diff_neighbor); }
extern "C" int kvz_hostsim_mv_scale(int mv, int scale) { return kvz::mv_scale(mv, scale); }
extern "C" unsigned kvz_hostsim_mv_scale_packed(unsigned mv, int scale) { return kvz::mv_scale_packed(mv, scale); }
// the record of picture `picture` of a table (116 bytes: n_refs, frame[4], spatial[4][4], temporal[4][4], start[4][4])
extern "C" void kvz_hostsim_inter_refs_record(const kvz_hip_inter_refs *refs, int picture, int poc, void *out) { const kvz::InterRefsRecord r = kvz::inter_refs_record(refs, picture, poc); memcpy(out, &r, sizeof r); }
// the initial states of a slice type at a QP in the coder's numbering with ref_idx_l0's contexts, and the search's (IX_* numbering, 168 of them)
extern "C" void kvz_hostsim_slice_contexts_refs(int slice_type, int qp, uint8_t *out) { kvz::entropy_slice_contexts(slice_type, qp, out, true); }
extern "C" void kvz_hostsim_search_contexts_refs(int slice_type, int qp, int refs, uint8_t *out)
{
  float fbits[128] = { 0 };
  kvz::InterModel m;
  kvz::inter_model_init(&m, qp, 1, 0, fbits, 0, 0, 0, 4, 3, 0, 28, 64, 64, 0, 0, 0, 0, 0, 0, slice_type, refs);
  memcpy(out, m.ctx_init, kvz::IX_COUNT);
}

// the twins of the argument checks the three entry points add to those of their _slices twins: 0 accepted, -1 refused with the library's message.
// stage 0: kvz_hip_dev_inter_ctu_pass_refs, 1: kvz_hip_dev_loop_filters_inter_refs, 2: kvz_hip_dev_entropy_code_inter_refs
extern "C" int kvz_hostsim_inter_refs_check(const kvz_hip_inter_params *p, int has_tile_xy, int slice_type, int stage, int n_pictures, const kvz_hip_inter_pictures *pictures,
                                            const kvz_hip_inter_refs *refs)
{
  const char *who = stage == 0 ? "kvz_hip_dev_inter_ctu_pass_refs" : (stage == 1 ? "kvz_hip_dev_loop_filters_inter_refs" : "kvz_hip_dev_entropy_code_inter_refs");
  if (kvz_hostsim_inter_slices_check(p, has_tile_xy, slice_type, stage)) return -1;
  if (stage == 1) return kvz::inter_refs_launch_known(refs, n_pictures, true, nullptr, slice_type, who) ? 0 : -1;
  if (pictures && !kvz::inter_pictures_known(pictures, n_pictures, who)) return -1;
  return kvz::inter_refs_launch_known(refs, n_pictures, pictures != nullptr, pictures ? pictures->poc : nullptr, slice_type, who) ? 0 : -1;
}

// kvz_hip_dev_inter_ctu_pass_refs on the host: the arguments of kvz_hostsim_inter_pass_slices and the lists; ref / ref_cu are then the pool.  refs == NULL IS that
// call.  Returns 0, or -1 for what the library refuses (nothing is computed then)
extern "C" int kvz_hostsim_inter_pass_refs(int width, int height, int n_pictures, const kvz_hip_inter_params *p, const kvz_hip_inter_pictures *pictures,
                                           const uint64_t *coeff_weights_of_qp, const float *fbits, const uint8_t *src, const uint8_t *ref, const kvz_hip_cu_info *ref_cu,
                                           uint8_t *rec, kvz_hip_cu_info *cu, int16_t *coeff, const int32_t *tile_xy, int n_references, int slice_type, const kvz_hip_inter_refs *refs)
{
  if (!refs) return kvz_hostsim_inter_pass_slices(width, height, n_pictures, p, pictures, coeff_weights_of_qp, fbits, src, ref, ref_cu, rec, cu, coeff, tile_xy, n_references, slice_type);
  kvz_hip_inter_params full;
  if (!kvz::inter_params_full(p, &full, "kvz_hip_dev_inter_ctu_pass")) return -1;
  p = &full;
  if (!kvz::inter_slice_launch_known(p, tile_xy != nullptr, slice_type, "kvz_hip_dev_inter_ctu_pass_refs")) return -1;
  if (pictures && !kvz::inter_pictures_known(pictures, n_pictures, "kvz_hip_dev_inter_ctu_pass_refs")) return -1;
  if (!kvz::inter_refs_launch_known(refs, n_pictures, pictures != nullptr, pictures ? pictures->poc : nullptr, slice_type, "kvz_hip_dev_inter_ctu_pass_refs")) return -1;
  if (kvz::inter_pass_geometry_refused(width, height, n_pictures, p->ref_width, p->ref_height, p->tile_x, p->tile_y)) return -1;
  static kvz::Tables tb;
  kvz::build_tables(&tb);
  auto model_at_qp = [&](kvz::InterModel *row, int qp) {
    kvz::inter_model_init(row, qp, p->poc, coeff_weights_of_qp[qp], fbits, p->mv_constraint, p->sao, p->deblock, p->fme_level, p->pu_depth_inter_max, p->no_wpp, p->fast_residual_cost,
                          width, height, 0, 0, 0, 0, p->no_tmvp, 0, slice_type, 1);
  };
  const kvz::InterPictureTable table = kvz::inter_picture_table_refs(pictures->qp, pictures->poc, n_pictures, model_at_qp, refs);
  kvz::InterFrames F;
  memset(&F, 0, sizeof F);
  F.W = width; F.H = height; F.wc = (width + 63) / 64; F.hc = (height + 63) / 64; F.frame_px = (long)width * height * 3 / 2; F.cells = (long)(width / 4) * (height / 4);
  F.src = src; F.ref = ref; F.ref_cu = ref_cu; F.rec = rec; F.cu = cu; F.coeff = coeff;
  F.ctx_out = (kvz::ICtx *)calloc((size_t)F.wc * F.hc * n_pictures, sizeof(kvz::ICtx));
  kvz::InterSlab *slab = (kvz::InterSlab *)calloc(1, sizeof(kvz::InterSlab));
  F.slabs = slab;
  F.pictures = (const kvz::InterPicture *)table.image.data();
  memset(cu, 0, (size_t)F.cells * n_pictures * sizeof(kvz_hip_cu_info));
  std::vector<uint32_t> items;
  kvz::inter_ticket_items(F.wc, F.hc, n_pictures, p->no_wpp, items);
  g_p_merge_origin.clear();
  g_kvz_ictu_p = 1; g_kvz_ictu_refs = 1;
  kvz::InterCtu::begin_launch(F, table.model_of_picture(table.image.data(), 0), &tb, slab);
  for (const uint32_t item : items) {
    kvz::InterCtu::begin_ctu((int)(item >> 16), (int)(item & 0xff) * 64, (int)((item >> 8) & 0xff) * 64);
    kvz::InterCtu::run();
  }
  g_kvz_ictu_p = 0; g_kvz_ictu_refs = 0;
  free(F.ctx_out); free(slab);
  return 0;
}

// What the decisions of picture `picture` of the LAST kvz_hostsim_inter_pass_refs launch were as far as the lists go, CU by CU, from its records and the origins of
// the merge lists the program built.  n_refs: the length of the picture's list.  out[8]: 0 reference index 1 chosen by the search (not merged), 1 merged with a
// candidate of a reference index above 0, 2 skipped with one, 3 a chosen zero merge candidate of a reference index above 0, 4 ref_idx_l0 coded with its second
// context bin (a searched CU with an index above 0 in a list of three or more), 5 reference index 2 or 3 chosen, 6 a reference index outside the list (must be 0).
// Counts are ADDED to out.
extern "C" void kvz_hostsim_refs_census(const kvz_hip_cu_info *cu, int width, int height, int picture, int n_refs, unsigned long long *out)
{
  const int w4 = width >> 2;
  for (int y = 0; y < height; y += 8)
    for (int x = 0; x < width; x += 8) {
      const kvz_hip_cu_info &c = cu[(y >> 2) * w4 + (x >> 2)];
      const int w = 64 >> c.depth;
      if ((x & (w - 1)) || (y & (w - 1)) || c.type != 2) continue;
      const int r = c.mv_ref[0];
      if (r >= n_refs) out[6]++;
      if (r >= 2) out[5]++;
      if (c.skipped) { if (r > 0) out[2]++; }
      else if (c.merged) { if (r > 0) out[1]++; }
      else { if (r == 1) out[0]++; if (r > 0 && n_refs > 2) out[4]++; }
      if ((c.skipped || c.merged) && r > 0) {
        const auto it = g_p_merge_origin.find(p_origin_key(picture, x, y, w));
        if (it != g_p_merge_origin.end() && c.merge_idx >= (int)(it->second >> 8)) out[3]++;
      }
    }
}

// kvz_hip_dev_entropy_code_inter_refs on the host: kvz_hostsim_entropy_code_inter_slices with the lists -- ref_cu is then the pool, the initial states hold
// ref_idx_l0's contexts, and every picture's record is the one the library lays out.  refs == NULL IS that call
extern "C" long kvz_hostsim_entropy_code_inter_refs(int slice_type, const int32_t *qp_of_picture, const int32_t *poc_of_picture, int width, int height, int n_pictures, int no_wpp,
                                                    const kvz_hip_cu_info *cu, const kvz_hip_cu_info *ref_cu, const int16_t *coeff, const unsigned long long *sao_recs,
                                                    const uint8_t *sao_merge, uint32_t cap, uint8_t *out, uint32_t *substream_bytes, const kvz_hip_inter_refs *refs)
{
  if (!refs) return kvz_hostsim_entropy_code_inter_slices(slice_type, qp_of_picture, poc_of_picture, width, height, n_pictures, no_wpp, cu, ref_cu, coeff, sao_recs, sao_merge, cap, out, substream_bytes);
  if (!kvz::inter_slice_type_known(slice_type, "kvz_hip_dev_entropy_code_inter_refs")) return -1;
  if (!kvz::inter_picture_qps_known(qp_of_picture, n_pictures, "kvz_hostsim_entropy_code_inter_refs")) return -1;
  if (!kvz::inter_refs_launch_known(refs, n_pictures, poc_of_picture != nullptr, poc_of_picture, slice_type, "kvz_hip_dev_entropy_code_inter_refs")) return -1;
  static kvz::Tables tb;
  kvz::build_tables(&tb);
  int row_of_qp[52], qp_of_row[52];
  const int n_rows = kvz::inter_qp_rows(qp_of_picture, n_pictures, row_of_qp, qp_of_row);
  std::vector<uint8_t> rows((size_t)n_rows * KVZ_ENTROPY_CTX_ROW, 0);
  for (int r = 0; r < n_rows; r++) kvz::entropy_slice_contexts(slice_type, qp_of_row[r], &rows[(size_t)r * KVZ_ENTROPY_CTX_ROW], true);
  std::vector<uint16_t> row_of_picture((size_t)n_pictures);
  std::vector<kvz::InterRefsRecord> recs((size_t)n_pictures);
  for (int i = 0; i < n_pictures; i++) { row_of_picture[(size_t)i] = (uint16_t)row_of_qp[qp_of_picture[i]]; recs[(size_t)i] = kvz::inter_refs_record(refs, i, poc_of_picture[i]); }
  kvz::EntropyJob J;
  memset(&J, 0, sizeof J);
  J.W = width; J.H = height; J.wc = (width + 63) / 64; J.hc = (height + 63) / 64; J.n_frames = n_pictures; J.no_wpp = no_wpp;
  J.cu = cu; J.ref_cu = ref_cu; J.coeff = coeff; J.sao = sao_recs; J.sao_merge = sao_merge;
  J.ctx_rows = rows.data(); J.model_of_picture = row_of_picture.data(); J.poc_of_picture = poc_of_picture;
  J.p_slice = 1; J.refs = recs.data();
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
