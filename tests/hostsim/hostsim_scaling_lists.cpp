// hostsim_scaling_lists.cpp -- TEST INFRASTRUCTURE (see hostsim.cpp and hostsim_models.cpp, which this unit includes whole: one library with everything of
// libkvz_hostsim_models.so plus what scaling lists add).  kvz_hip_batch_set_scaling_lists on the host: the shared arithmetic on one block (kvz_recon.hpp quant_level /
// dequant_level under the factors kvz_scaling_lists.hpp derives, indexed by list_index), and the pass on a batch that has lists (hostsim_models.cpp's, which takes
// the build the library takes), every picture on its two rows of the factor table as the library stages them.
// tests/test_scaling_lists_sim.py builds and uses it.
#include "hostsim_models.cpp"

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

// kvz_hip_intra_frames_models on a batch that was given kvz_hip_batch_set_scaling_lists(sets, n_sets, set_of_picture) -- n_sets == 0: a batch without lists, which
// takes the builds without them.  Returns 0, or -1 where the library refuses the sets, the table, or the table on a batch with lists.
extern "C" int kvz_hostsim_lists_intra_frames_models(const kvz_hip_picture_models *pm, const kvz_hip_scaling_lists *sets, int n_sets, const uint16_t *set_of_picture, int width,
                                                     int height, int n_frames, const uint8_t *src, uint8_t *rec, int16_t *coeff, uint8_t *cu_depth, uint8_t *cu_mode, double *ctu_cost)
{
  const char *who = "kvz_hostsim_lists_intra_frames_models";
  if (!kvz::scaling_list_sets_known(sets, n_sets, set_of_picture, n_frames, true, who)) return -1;
  if (!kvz::picture_models_known(pm, n_frames, true, who)) return -1;
  if (!kvz::scaling_lists_known(pm, n_sets > 0, who)) return -1;
  std::vector<uint32_t> rows((size_t)(n_sets ? n_sets + 1 : 0) * 6 * kvz::KVZ_LIST_ROW);  // as kvz_hip_batch_set_scaling_lists lays them out: the sets, then the flat list
  for (int k = 0; k < n_sets; k++) kvz::scaling_list_rows(&sets[k], rows.data() + (size_t)k * 6 * kvz::KVZ_LIST_ROW);
  if (n_sets) kvz::scaling_list_rows(nullptr, rows.data() + (size_t)n_sets * 6 * kvz::KVZ_LIST_ROW);
  HostFrames hf(width, height, n_frames, src, rec, coeff, cu_depth, cu_mode, ctu_cost);
  return host_intra_frames_models(pm, hf, n_frames, rows.data(), n_sets, set_of_picture);
}
