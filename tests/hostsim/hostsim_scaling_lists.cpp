// hostsim_scaling_lists.cpp -- TEST INFRASTRUCTURE (see hostsim.cpp and hostsim_models.cpp, which this unit includes whole: one library with everything of
// libkvz_hostsim_models.so plus what scaling lists add).  kvz_hip_batch_set_scaling_lists on the host: the shared arithmetic on one block (kvz_recon.hpp quant_level /
// dequant_level under the factors kvz_scaling_lists.hpp derives, indexed by list_index), and the LISTS instantiations of the CTU program -- the other units only
// instantiate the others -- chosen as kvz_batch.hpp chooses the kernel, every picture on its two rows of the factor table as the library stages them.
// tests/test_scaling_lists_sim.py builds and uses it.
#include "hostsim_models.cpp"
#include "../../kvazaar_amd/csrc/kvz_scaling_lists.hpp"

extern "C" void kvz_hostsim_scaling_lists_default(kvz_hip_scaling_lists *l) { kvz::scaling_lists_default(l); }

// what kvz_hip_batch_set_scaling_lists checks: 0 accepted, -1 refused
extern "C" int kvz_hostsim_lists_check(const kvz_hip_scaling_lists *sets, int n_sets, const uint16_t *set_of_picture, int n_frames, int ticket_schedule)
{
  return kvz::scaling_list_sets_known(sets, n_sets, set_of_picture, n_frames, ticket_schedule != 0, "kvz_hostsim_lists_check") ? 0 : -1;
}

// kvz_quant of one 2^log2w block of plane c (0 Y, 1 U, 2 V; I slice, 8 bit) at `qp` under the set's lists (set == NULL: the flat list): coef -> levels, row-major
extern "C" void kvz_hostsim_lists_quant(const kvz_hip_scaling_lists *set, int log2w, int c, int qp, const int16_t *coef, int16_t *levels)
{
  std::vector<uint32_t> rows(6 * kvz::KVZ_LIST_ROW);
  kvz::scaling_list_rows(set, rows.data());
  const kvz::QuantScalars q = kvz::quant_scalars(qp, 8, 1, 1, 1 << log2w, c ? 2 : 0);
  const uint32_t *plane = rows.data() + (kvz::scaled_qp(c ? 2 : 0, qp, 0) % 6) * kvz::KVZ_LIST_ROW + c * kvz::KVZ_LIST_PLANE;
  for (int e = 0; e < (1 << (2 * log2w)); e++) levels[e] = (int16_t)kvz::quant_level(coef[e], q, kvz::list_factor(plane[kvz::list_index(log2w, e)]).fwd);
}
// ... and kvz_dequant: levels -> coef
extern "C" void kvz_hostsim_lists_dequant(const kvz_hip_scaling_lists *set, int log2w, int c, int qp, const int16_t *levels, int16_t *coef)
{
  std::vector<uint32_t> rows(6 * kvz::KVZ_LIST_ROW);
  kvz::scaling_list_rows(set, rows.data());
  const kvz::QuantScalars q = kvz::quant_scalars(qp, 8, 1, 1, 1 << log2w, c ? 2 : 0);
  const uint32_t *plane = rows.data() + (kvz::scaled_qp(c ? 2 : 0, qp, 0) % 6) * kvz::KVZ_LIST_ROW + c * kvz::KVZ_LIST_PLANE;
  for (int e = 0; e < (1 << (2 * log2w)); e++) coef[e] = kvz::dequant_level(levels[e], q, kvz::list_factor(plane[kvz::list_index(log2w, e)]).inv);
}

namespace {
template <bool CABAC, bool S32> void run_ctu_lists(const kvz::CtuModel *cm, const kvz::Tables *tb, const kvz::CtuFrames &F, void *sh, int frame, int cx, int cy, const uint32_t *lf_y,
                                                   const uint32_t *lf_c)
{
  kvz::CtuProgramT<CABAC, S32, false, false, true> p;
  p.m = cm; p.tb = tb; p.F = F; p.s = (kvz::CtuSharedT<CABAC> *)sh; p.frame = frame; p.cx = cx * 64; p.cy = cy * 64;
  p.lf_y = lf_y; p.lf_c = lf_c;
  p.run();
}
}  // namespace

// kvz_hip_intra_frames_models on a batch that was given kvz_hip_batch_set_scaling_lists(sets, n_sets, set_of_picture) -- n_sets == 0: a batch without lists, which
// runs as before (kvz_hostsim_intra_frames_models).  Returns 0, or -1 where the library refuses the sets, the table, or the table on a batch with lists.
extern "C" int kvz_hostsim_lists_intra_frames_models(const kvz_hip_picture_models *pm, const kvz_hip_scaling_lists *sets, int n_sets, const uint16_t *set_of_picture, int width,
                                                     int height, int n_frames, const uint8_t *src, uint8_t *rec, int16_t *coeff, uint8_t *cu_depth, uint8_t *cu_mode, double *ctu_cost)
{
  const char *who = "kvz_hostsim_lists_intra_frames_models";
  if (!kvz::scaling_list_sets_known(sets, n_sets, set_of_picture, n_frames, true, who)) return -1;
  if (!kvz::picture_models_known(pm, n_frames, true, who)) return -1;
  if (!kvz::scaling_lists_known(pm, n_sets > 0, who)) return -1;
  if (n_sets == 0) return kvz_hostsim_intra_frames_models(pm, width, height, n_frames, src, rec, coeff, cu_depth, cu_mode, ctu_cost, nullptr, nullptr);
  static kvz::Tables tb;
  kvz::build_tables(&tb);
  std::vector<uint32_t> rows((size_t)(n_sets + 1) * 6 * kvz::KVZ_LIST_ROW);  // as kvz_hip_batch_set_scaling_lists lays them out: the sets, then the flat list
  for (int k = 0; k < n_sets; k++) kvz::scaling_list_rows(&sets[k], rows.data() + (size_t)k * 6 * kvz::KVZ_LIST_ROW);
  kvz::scaling_list_rows(nullptr, rows.data() + (size_t)n_sets * 6 * kvz::KVZ_LIST_ROW);
  kvz::CtuFrames F;
  F.W = width; F.H = height; F.wc = (width + 63) / 64; F.hc = (height + 63) / 64; F.frame_px = (long)width * height * 3 / 2;
  F.src = src; F.rec = rec; F.coeff = coeff; F.cu_depth = cu_depth; F.cu_mode = cu_mode; F.ctu_cost = ctu_cost; F.prof = nullptr;
  const size_t nctu = (size_t)F.wc * F.hc * n_frames;
  uint8_t *border = (uint8_t *)calloc(nctu, KVZ_BORDER_BYTES);
  F.border = border;
  int16_t *scratch = (int16_t *)calloc(nctu * 6144, sizeof(int16_t));
  F.coeff_scratch = scratch;
  void *sh = calloc(1, sizeof(kvz::CtuSharedT<true>) > sizeof(kvz::CtuSharedT<false>) ? sizeof(kvz::CtuSharedT<true>) : sizeof(kvz::CtuSharedT<false>));
  const HostModelTable T(pm);
  const bool s32 = pm->models[0].search_32x32 != 0, any_cabac = kvz::picture_models_any_cabac(pm);
  for (int f = 0; f < n_frames; f++) {
    const kvz::CtuModel *cm = kvz::picture_model(T.table, f);
    const uint32_t at = kvz::scaling_list_rows_of_picture(set_of_picture ? set_of_picture[f] : 0, n_sets, cm->qp);
    const uint32_t *lf_y = rows.data() + (size_t)(at & 0xffffu) * kvz::KVZ_LIST_ROW, *lf_c = rows.data() + (size_t)(at >> 16) * kvz::KVZ_LIST_ROW;
    for (int cy = 0; cy < F.hc; cy++)
      for (int cx = 0; cx < F.wc; cx++) {
        if (s32) { if (any_cabac) run_ctu_lists<true, true>(cm, &tb, F, sh, f, cx, cy, lf_y, lf_c); else run_ctu_lists<false, true>(cm, &tb, F, sh, f, cx, cy, lf_y, lf_c); }
        else if (any_cabac) run_ctu_lists<true, false>(cm, &tb, F, sh, f, cx, cy, lf_y, lf_c);
        else run_ctu_lists<false, false>(cm, &tb, F, sh, f, cx, cy, lf_y, lf_c);
      }
  }
  free(sh); free(scratch); free(border);
  return 0;
}
