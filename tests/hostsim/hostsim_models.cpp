// hostsim_models.cpp -- TEST INFRASTRUCTURE (see hostsim.cpp, which this unit includes whole: one library with everything of libkvz_hostsim.so plus the twins of
// the kvz_hip_*_models entry points).  A batch whose pictures run under models of their own (kvz_hip_picture_models), walked picture by picture on the host: every
// picture's model is found through the function the device uses (kvz_ctu.hpp / kvz_syntax.hpp picture_model), the table is checked by the text the library checks it
// with (kvz_picture_models.hpp), and the instantiation of the CTU program is the build kvz_batch.hpp launches -- ONE for the whole batch, chosen by the function
// the library asks and reached through its dispatcher (kvz_ctu_builds.hpp).  tests/test_mixed_qp_sim.py builds and uses it.
#include "hostsim.cpp"
#include "../../kvazaar_amd/csrc/kvz_picture_models.hpp"
#include "../../kvazaar_amd/csrc/kvz_scaling_lists.hpp"

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
// kvz_intra_frames_queue on the host, the table checked: ONE build for the whole batch, every picture under its row of the table and, on a batch with scaling lists
// (n_sets > 0; rows: as kvz_hip_batch_set_scaling_lists lays them out), on its two rows of the factor table.  -1: no build serves the launch
int host_intra_frames_models(const kvz_hip_picture_models *pm, HostFrames &hf, int n_frames, const uint32_t *rows = nullptr, int n_sets = 0, const uint16_t *set_of_picture = nullptr)
{
  const HostModelTable T(pm);
  const bool ran = kvz::ctu_build_dispatch(kvz::picture_models_build(&pm, 1, n_sets > 0, false), [&](auto bt) {
    if constexpr (!bt.joint)
      for (int f = 0; f < n_frames; f++) {
        const kvz::CtuModel *cm = kvz::picture_model(T.table, f);  // what thread 0 of a workgroup loads for the CTU it drew
        const uint32_t at = n_sets ? kvz::scaling_list_rows_of_picture(set_of_picture ? set_of_picture[f] : 0, n_sets, cm->qp) : 0;
        for (int cy = 0; cy < hf.F.hc; cy++)
          for (int cx = 0; cx < hf.F.wc; cx++)
            run_ctu(bt, cm, host_tables(), hf.F, hf.shared.data(), f, cx, cy, rows + (size_t)(at & 0xffffu) * kvz::KVZ_LIST_ROW, rows + (size_t)(at >> 16) * kvz::KVZ_LIST_ROW);
      }
  });
  return ran ? 0 : -1;
}
}  // namespace

// The build list and the choice (kvz_ctu_builds.hpp), for tests/test_ctu_builds_sim.py.  rows [n][7]: unit, CABAC, S32, RDOQ, SH, LISTS, JOINT of every build of the
// list; returns n.  *unit_mask: the translation units, a bit each.
extern "C" int kvz_hostsim_ctu_builds(int *rows, unsigned long long *unit_mask)
{
#define KVZ_CTU_X(...) __VA_ARGS__,
  const int list[] = { KVZ_CTU_BUILDS(KVZ_CTU_X) };
#undef KVZ_CTU_X
  memcpy(rows, list, sizeof list);
  *unit_mask = kvz::KVZ_CTU_UNIT_MASK;
  return (int)(sizeof list / sizeof list[0] / 7);
}
extern "C" int kvz_hostsim_ctu_build_choose(int search_32x32, int rdoq, int search_nxn, int any_cabac, int any_signhide, int lists, int joint)
{
  return kvz::ctu_build_choose({ search_32x32 != 0, rdoq != 0, search_nxn != 0, any_cabac != 0, any_signhide != 0, lists != 0, joint != 0 });
}

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
  HostFrames hf(width, height, n_frames, src, rec, coeff, cu_depth, cu_mode, ctu_cost, cu_part, cu_mode4);
  return host_intra_frames_models(pm, hf, n_frames);
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
