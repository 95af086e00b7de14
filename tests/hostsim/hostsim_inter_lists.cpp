// hostsim_inter_lists.cpp -- TEST INFRASTRUCTURE (see hostsim.cpp and hostsim_inter_models.cpp, which this unit includes whole: one library with everything of
// libkvz_hostsim_inter_models.so plus the twin of kvz_hip_dev_inter_ctu_pass_lists).  The inter CTU pass with per-coefficient scaling lists on the host: the device
// compiles the program twice, with KVZ_ICTU_LISTS 0 and 1; here the switch is a variable, so that this one library holds both forms of the same text -- the flat
// one behind every entry point of the units it includes and behind n_sets == 0, the LISTS one behind a launch with sets.  The sets are checked by the text the
// library checks them with (kvz_scaling_lists.hpp), the table is laid out by the function the library lays it out with (kvz_inter_host.hpp
// inter_picture_table_lists: records, model rows, factor rows from scaling_list_rows_inter) and read by the kernel's own begin_ctu and quantize_tu.
// tests/test_inter_scaling_lists_sim.py builds and uses it.
static int g_kvz_ictu_lists = 0;
#define KVZ_ICTU_LISTS g_kvz_ictu_lists
#include "hostsim_inter_models.cpp"

// kvz_hip_dev_inter_ctu_pass_lists on the host: the arguments of kvz_hostsim_inter_pass_pictures and the sets.  Returns 0, or -1 for what the library refuses
// (nothing is computed then).
extern "C" int kvz_hostsim_inter_pass_lists(int width, int height, int n_pictures, const kvz_hip_inter_params *p, const kvz_hip_inter_pictures *pictures,
                                            const uint64_t *coeff_weights_of_qp, const float *fbits, const uint8_t *src, const uint8_t *ref, const kvz_hip_cu_info *ref_cu,
                                            uint8_t *rec, kvz_hip_cu_info *cu, int16_t *coeff, const int32_t *tile_xy, int n_references,
                                            const kvz_hip_scaling_lists *sets, int n_sets, const uint16_t *set_of_picture)
{
  const char *who = "kvz_hostsim_inter_pass_lists";
  if (pictures && !kvz::inter_pictures_known(pictures, n_pictures, who)) return -1;
  if (kvz::inter_pass_geometry_refused(width, height, n_pictures, p->ref_width, p->ref_height, p->tile_x, p->tile_y)) return -1;
  if (!kvz::scaling_list_sets_known(sets, n_sets, set_of_picture, n_pictures, true, who)) return -1;
  if (n_sets == 0) return kvz_hostsim_inter_pass_pictures(width, height, n_pictures, p, pictures, coeff_weights_of_qp, fbits, src, ref, ref_cu, rec, cu, coeff, tile_xy, n_references);
  static kvz::Tables tb;
  kvz::build_tables(&tb);
  auto model_at_qp = [&](kvz::InterModel *row, int qp) {
    kvz::inter_model_init(row, qp, p->poc, coeff_weights_of_qp[qp], fbits, p->mv_constraint, p->sao, p->deblock, p->fme_level, p->pu_depth_inter_max, p->no_wpp, p->fast_residual_cost,
                          width, height, p->ref_width, p->ref_height, p->tile_x, p->tile_y, p->no_tmvp, 1);
  };
  std::vector<int32_t> qp_all, poc_all;
  if (!pictures) { qp_all.assign((size_t)n_pictures, p->qp); poc_all.assign((size_t)n_pictures, p->poc); }
  const kvz::InterPictureTable table = kvz::inter_picture_table_lists(pictures ? pictures->qp : qp_all.data(), pictures ? pictures->poc : poc_all.data(), n_pictures, model_at_qp, sets, n_sets, set_of_picture);
  kvz::InterFrames F;
  memset(&F, 0, sizeof F);
  F.W = width; F.H = height; F.wc = (width + 63) / 64; F.hc = (height + 63) / 64; F.frame_px = (long)width * height * 3 / 2; F.cells = (long)(width / 4) * (height / 4);
  F.src = src; F.ref = ref; F.ref_cu = ref_cu; F.rec = rec; F.cu = cu; F.coeff = coeff;
  F.ctx_out = (kvz::ICtx *)calloc((size_t)F.wc * F.hc * n_pictures, sizeof(kvz::ICtx));
  kvz::InterSlab *slab = (kvz::InterSlab *)calloc(1, sizeof(kvz::InterSlab));
  F.slabs = slab;
  F.tile_xy = (p->ref_width || p->ref_height) ? tile_xy : nullptr;
  F.ref_count = n_references > 0 ? n_references : 0;
  F.pictures = (const kvz::InterPicture *)table.image.data();
  memset(cu, 0, (size_t)F.cells * n_pictures * sizeof(kvz_hip_cu_info));
  std::vector<uint32_t> items;
  kvz::inter_ticket_items(F.wc, F.hc, n_pictures, p->no_wpp, items);
  g_kvz_ictu_lists = 1;
  kvz::InterCtu::begin_launch(F, table.model_of_picture(table.image.data(), 0), &tb, slab);
  for (const uint32_t item : items) {
    kvz::InterCtu::begin_ctu((int)(item >> 16), (int)(item & 0xff) * 64, (int)((item >> 8) & 0xff) * 64);
    kvz::InterCtu::run();
  }
  g_kvz_ictu_lists = 0;
  free(F.ctx_out); free(slab);
  return 0;
}

// The factors quantize_tu takes for element e of a 2^log2w block of plane c in an intra / inter CU of a picture at `qp` under `set` (NULL: flat), through the table
// and the records a launch of that one picture gets: *fwd / *inv.  What tests/test_inter_scaling_lists_sim.py holds against the tables of the reference's list index.
extern "C" void kvz_hostsim_inter_list_factors(const kvz_hip_scaling_lists *set, int qp, int intra_cu, int c, int log2w, int32_t *fwd, int32_t *inv)
{
  const int32_t poc = 1;
  const kvz::InterPictureTable table = kvz::inter_picture_table_lists(&qp, &poc, 1, [](kvz::InterModel *m, int) { memset(m, 0, sizeof *m); }, set, set ? 1 : 0, nullptr);
  const kvz::InterPictureLists *rec = (const kvz::InterPictureLists *)table.image.data();
  const uint32_t *plane = (const uint32_t *)((const uint8_t *)table.image.data() + (c ? rec->lists_c_at : rec->lists_y_at)) + kvz::list_plane_of(intra_cu != 0, c) * kvz::KVZ_LIST_PLANE;
  for (int e = 0; e < (1 << (2 * log2w)); e++) { const kvz::ListFactor f = kvz::list_factor(plane[kvz::list_index(log2w, e)]); fwd[e] = f.fwd; inv[e] = f.inv; }
}
