// hostsim_signhide.cpp -- TEST INFRASTRUCTURE (see hostsim.cpp and hostsim_models.cpp, which this unit includes whole: one library with everything of
// libkvz_hostsim_models.so plus what sign data hiding adds).  kvz_hip_intra_cost_model::signhide on the host: the shared hiding rule on one block (kvz_recon.hpp
// sign_hide_block, what the lanes of the CTU pass apply a group each), the pass on tables that have the switch (hostsim_models.cpp's, which takes the build the
// library takes), and the entropy coder with every picture's switch read from its model's row, as
// kvz_batch.hpp picture_models_stage lays the rows out.  tests/test_signhide_sim.py builds and uses it.
#include "hostsim_models.cpp"

// kvz_quant + sign data hiding of one 2^log2w block (type 0 luma / 2 chroma, I slice, 8 bit, flat lists) at `qp`: coef -> levels, both row-major
extern "C" void kvz_hostsim_signhide_quant(int log2w, int scan_mode, int type, int qp, const int16_t *coef, int16_t *levels)
{
  static kvz::Tables tb;
  kvz::build_tables(&tb);
  const kvz::QuantScalars q = kvz::quant_scalars(qp, 8, 1, 0, 1 << log2w, type);
  for (int e = 0; e < (1 << (2 * log2w)); e++) levels[e] = (int16_t)kvz::quant_level(coef[e], q);
  kvz::sign_hide_block(coef, levels, log2w, scan_mode, q, tb.diag8);
}
// quant-generic.c:94 of one coefficient, as the shared text states it
extern "C" int kvz_hostsim_signhide_delta_u(int log2w, int type, int qp, int coef)
{
  const kvz::QuantScalars q = kvz::quant_scalars(qp, 8, 1, 0, 1 << log2w, type);
  return kvz::quant_delta_u(coef, kvz::quant_level(coef, q), q);
}

// what kvz_hip_intra_frames checks of ONE model before it queues anything: 0 accepted, -1 refused
extern "C" int kvz_hostsim_signhide_model_check(const kvz_hip_intra_cost_model *m, int ticket_schedule)
{
  return kvz::cost_model_known(m, "kvz_hostsim_signhide_model_check") && kvz::signhide_known(m, ticket_schedule != 0, "kvz_hostsim_signhide_model_check") ? 0 : -1;
}

// kvz_hip_intra_frames_models on the host, for tables with and without the switch: the choice of the build sees it (a table with it runs through ONE sign-hiding
// build for the whole batch, which reads the switch of every picture's row), so this is kvz_hostsim_intra_frames_models without the NxN outputs.
extern "C" int kvz_hostsim_signhide_intra_frames_models(const kvz_hip_picture_models *pm, int width, int height, int n_frames, const uint8_t *src, uint8_t *rec,
                                                        int16_t *coeff, uint8_t *cu_depth, uint8_t *cu_mode, double *ctu_cost)
{
  return kvz_hostsim_intra_frames_models(pm, width, height, n_frames, src, rec, coeff, cu_depth, cu_mode, ctu_cost, nullptr, nullptr);
}

// kvz_hip_batch_entropy_code_models on the host with the rows as the library stages them: a model's initial states and, in the row's last byte, its signhide
// switch.  The substreams are coded twice, counting and writing; -2 when the two disagree about a size.
extern "C" long kvz_hostsim_signhide_entropy_code_models(const kvz_hip_picture_models *pm, int width, int height, int n_frames, const uint8_t *cu_depth,
                                                         const uint8_t *cu_mode, const int16_t *coeff, uint32_t cap, uint8_t *out, uint32_t *substream_bytes,
                                                         uint32_t *most_records)
{
  if (!kvz::picture_models_known(pm, n_frames, true, "kvz_hostsim_signhide_entropy_code_models")) return -1;
  static kvz::Tables tb;
  kvz::build_tables(&tb);
  const kvz_hip_intra_cost_model *m = &pm->models[0];
  kvz::EntropyJob J;
  memset(&J, 0, sizeof J);
  J.W = width; J.H = height; J.wc = (width + 63) / 64; J.hc = (height + 63) / 64; J.n_frames = n_frames; J.no_wpp = m->no_wpp;
  J.depth = cu_depth; J.mode = cu_mode; J.coeff = coeff;
  std::vector<uint8_t> rows((size_t)pm->n_models * KVZ_ENTROPY_CTX_ROW, 0);
  for (int i = 0; i < pm->n_models; i++) {
    memcpy(&rows[(size_t)i * KVZ_ENTROPY_CTX_ROW], pm->models[i].ctx_init, sizeof pm->models[i].ctx_init);
    rows[(size_t)i * KVZ_ENTROPY_CTX_ROW + KVZ_ENTROPY_ROW_SIGNHIDE] = pm->models[i].signhide != 0;
  }
  J.ctx_rows = rows.data(); J.model_of_picture = pm->model_of_picture;
  const long items = (long)n_frames * J.wc * J.hc, streams = (long)n_frames * (m->no_wpp ? 1 : J.hc);
  cap = (cap + 15u) & ~15u;
  J.bins = (uint32_t *)aligned_alloc(64, (size_t)items * cap * sizeof(uint32_t)); J.nbins = (uint32_t *)malloc((size_t)items * sizeof(uint32_t)); J.nbits = (uint32_t *)malloc((size_t)items * sizeof(uint32_t)); J.cap = cap;
  J.row_ctx = (uint8_t *)malloc((size_t)n_frames * J.hc * KVZ_ENTROPY_CTXS);
  const kvz::EntropyTabs T{ &tb.ctx_next[0][0] };
  uint8_t ctx[KVZ_ENTROPY_CTXS];
  *most_records = 0;
  for (long i = 0; i < items; i++) { hostsim_ctu_bins(J, &tb, i); if (J.nbins[i] > *most_records) *most_records = J.nbins[i]; }
  long total = -1;
  if (*most_records <= cap) {
    if (!m->no_wpp) for (int f = 0; f < n_frames; f++) kvz::entropy_row_contexts(J, T, f, ctx);
    total = 0;
    for (long i = 0; i < streams; i++) {
      unsigned long long bits = 0;
      const long per_stream = m->no_wpp ? (long)J.wc * J.hc : J.wc;
      for (long k = 0; k < per_stream; k++) bits += J.nbits[i * per_stream + k];
      const size_t room = (size_t)(((bits + 7) / 8 + 16) * 3 / 2);
      const uint32_t counted = hostsim_code_row(J, tb, i, nullptr, room);
      substream_bytes[i] = hostsim_code_row(J, tb, i, out + total, room);
      if (counted != substream_bytes[i]) { total = -2; break; }
      total += substream_bytes[i];
    }
  }
  free(J.bins); free(J.nbins); free(J.nbits); free(J.row_ctx);
  return total;
}
