// hostsim_models.cpp -- TEST INFRASTRUCTURE (see hostsim.cpp, which this unit includes whole: one library with everything of libkvz_hostsim.so plus the twins of
// the kvz_hip_*_models entry points).  A batch whose pictures run under models of their own (kvz_hip_picture_models), walked picture by picture on the host: every
// picture's model is found through the function the device uses (kvz_ctu.hpp / kvz_syntax.hpp picture_model), the table is checked by the text the library checks it
// with (kvz_picture_models.hpp), and the instantiation of the CTU program is chosen as kvz_batch.hpp chooses the kernel -- ONE for the whole batch, the one with the
// CABAC coefficient model when any model asks for it.  tests/test_mixed_qp_sim.py builds and uses it.
#include "hostsim.cpp"
#include "../../kvazaar_amd/csrc/kvz_picture_models.hpp"

namespace {
// the compact rows the device keeps (kvz_batch.hpp picture_models_stage), with host pointers
struct HostModelTable {
  std::vector<kvz::CtuModel> rows;
  kvz::CtuModelTable table;
  explicit HostModelTable(const kvz_hip_picture_models *pm) : rows((size_t)pm->n_models)
  {
    for (int i = 0; i < pm->n_models; i++) {
      kvz::ctu_model_from(&pm->models[i], &rows[(size_t)i]);
      rows[(size_t)i].entropy_fbits = pm->models[0].entropy_fbits;  // the one price table of the launch
    }
    table.models = rows.data();
    table.model_of_picture = pm->model_of_picture;
  }
};
template <bool CABAC, bool S32, bool RDOQ> void run_ctu(const kvz::CtuModel *cm, const kvz::Tables *tb, const kvz::CtuFrames &F, void *sh, int frame, int cx, int cy)
{
  kvz::CtuProgramT<CABAC, S32, RDOQ> p;
  if constexpr (RDOQ) { static kvz::RdoqLds rdoq_lds; p.rl = &rdoq_lds; }
  p.m = cm; p.tb = tb; p.F = F; p.s = (kvz::CtuSharedT<CABAC> *)sh; p.frame = frame; p.cx = cx * 64; p.cy = cy * 64;
  p.run();
}
}  // namespace

// 0 when a batch of n_frames pictures accepts the table, -1 when the library refuses it (ticket_schedule == 0: as under KVZ_HIP_SCHED=wave)
extern "C" int kvz_hostsim_picture_models_check(const kvz_hip_picture_models *pm, int n_frames, int ticket_schedule)
{
  return kvz::picture_models_known(pm, n_frames, ticket_schedule != 0, "kvz_hostsim_picture_models_check") ? 0 : -1;
}

// kvz_hip_intra_frames_models on the host: src / rec / ... hold the n_frames pictures back to back in the batch's layouts (cu_part / cu_mode4 may be null without search_nxn).
// Returns 0, or -1 for a table the library refuses (nothing is computed then).
extern "C" int kvz_hostsim_intra_frames_models(const kvz_hip_picture_models *pm, int width, int height, int n_frames, const uint8_t *src, uint8_t *rec, int16_t *coeff,
                                               uint8_t *cu_depth, uint8_t *cu_mode, double *ctu_cost, uint8_t *cu_part, uint8_t *cu_mode4)
{
  if (!kvz::picture_models_known(pm, n_frames, true, "kvz_hostsim_intra_frames_models")) return -1;
  static kvz::Tables tb;
  kvz::build_tables(&tb);
  kvz::CtuFrames F;
  F.W = width; F.H = height; F.wc = (width + 63) / 64; F.hc = (height + 63) / 64; F.frame_px = (long)width * height * 3 / 2;
  F.src = src; F.rec = rec; F.coeff = coeff; F.cu_depth = cu_depth; F.cu_mode = cu_mode; F.ctu_cost = ctu_cost; F.prof = nullptr;
  F.cu_part = cu_part; F.cu_mode4 = cu_mode4;
  const size_t nctu = (size_t)F.wc * F.hc * n_frames;
  uint8_t *border = (uint8_t *)calloc(nctu, KVZ_BORDER_BYTES);
  F.border = border;
  int16_t *scratch = (int16_t *)calloc(nctu * 6144, sizeof(int16_t));
  F.coeff_scratch = scratch;
  void *sh = calloc(1, sizeof(kvz::CtuSharedT<true>) > sizeof(kvz::CtuSharedT<false>) ? sizeof(kvz::CtuSharedT<true>) : sizeof(kvz::CtuSharedT<false>));
  const HostModelTable T(pm);
  const kvz_hip_intra_cost_model &m0 = pm->models[0];
  const bool any_cabac = kvz::picture_models_any_cabac(pm);
  for (int f = 0; f < n_frames; f++) {
    const kvz::CtuModel *cm = kvz::picture_model(T.table, f);  // what thread 0 of a workgroup loads for the CTU it drew
    for (int cy = 0; cy < F.hc; cy++)
      for (int cx = 0; cx < F.wc; cx++) {
        if (m0.rdoq || m0.search_nxn) run_ctu<true, true, true>(cm, &tb, F, sh, f, cx, cy);
        else if (m0.search_32x32) { if (any_cabac) run_ctu<true, true, false>(cm, &tb, F, sh, f, cx, cy); else run_ctu<false, true, false>(cm, &tb, F, sh, f, cx, cy); }
        else if (any_cabac) run_ctu<true, false, false>(cm, &tb, F, sh, f, cx, cy);
        else run_ctu<false, false, false>(cm, &tb, F, sh, f, cx, cy);
      }
  }
  free(sh); free(scratch); free(border);
  return 0;
}

// kvz_hip_batch_entropy_code_models on the host: kvz_hostsim_entropy_code with every picture's initial context states from its row of the table
extern "C" long kvz_hostsim_entropy_code_models(const kvz_hip_picture_models *pm, int width, int height, int n_frames, const uint8_t *cu_depth, const uint8_t *cu_mode,
                                                const uint8_t *part, const uint8_t *mode4, const int16_t *coeff, const unsigned long long *sao_recs, const uint8_t *sao_merge,
                                                uint32_t cap, uint8_t *out, uint32_t *substream_bytes, uint32_t *most_records)
{
  if (!kvz::picture_models_known(pm, n_frames, true, "kvz_hostsim_entropy_code_models")) return -1;
  static kvz::Tables tb;
  kvz::build_tables(&tb);
  const kvz_hip_intra_cost_model *m = &pm->models[0];
  kvz::EntropyJob J;
  memset(&J, 0, sizeof J);
  J.W = width; J.H = height; J.wc = (width + 63) / 64; J.hc = (height + 63) / 64; J.n_frames = n_frames; J.no_wpp = m->no_wpp;
  J.depth = cu_depth; J.mode = cu_mode; J.part = part; J.mode4 = mode4; J.coeff = coeff; J.sao = sao_recs; J.sao_merge = sao_merge;
  std::vector<uint8_t> rows((size_t)pm->n_models * KVZ_ENTROPY_CTX_ROW, 0);  // as kvz_batch.hpp picture_models_stage lays them out
  for (int i = 0; i < pm->n_models; i++) memcpy(&rows[(size_t)i * KVZ_ENTROPY_CTX_ROW], pm->models[i].ctx_init, sizeof pm->models[i].ctx_init);
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
      substream_bytes[i] = hostsim_code_row(J, tb, i, out + total, (size_t)(((bits + 7) / 8 + 16) * 3 / 2));
      total += substream_bytes[i];
    }
  }
  free(J.bins); free(J.nbins); free(J.nbits); free(J.row_ctx);
  return total;
}
