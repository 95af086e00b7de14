// hostsim_inter_me.cpp -- TEST INFRASTRUCTURE (see hostsim.cpp and hostsim_inter_models.cpp, which this unit includes whole: one library with everything of
// libkvz_hostsim_inter_models.so plus the twin of a launch that chooses its integer motion search).  The device compiles the inter program with KVZ_ICTU_ME 0 and 1;
// here the switch is a variable (as hostsim_inter_lists.cpp has KVZ_ICTU_LISTS), so that this one library holds both forms of the same text -- the default search
// behind every entry point of the units it includes and behind three zero members, the chosen one behind a launch with a non-zero member.  The members are checked by
// the text the library checks them with (kvz_inter_host.hpp inter_me_known) and reach the program through the model rows the library fills (inter_model_set_me).
// tests/test_inter_me_sim.py, tests/test_me_search_reference.py and tests/golden/make_inter_me_golden.py build and use it.
static int g_kvz_ictu_me = 0;
#define KVZ_ICTU_ME g_kvz_ictu_me
#include "hostsim_inter_models.cpp"

// the twin of the argument check of kvz_hip_dev_inter_ctu_pass[_tiles|_pictures|_lists] (has_tiles: ref_width / ref_height / tile_xy given; n_sets) and of
// kvz_hip_dev_inter_ctu_pass_groups (joint): 0 accepted, -1 refused with the library's message
extern "C" int kvz_hostsim_inter_me_check(const kvz_hip_inter_params *p, int has_tiles, int n_sets, int joint)
{
  kvz_hip_inter_params full;  // (either known version of the struct, as the entry points take it)
  if (!kvz::inter_params_full(p, &full, joint ? "kvz_hip_dev_inter_ctu_pass_groups" : "kvz_hip_dev_inter_ctu_pass")) return -1;
  p = &full;
  const char *excluded = joint ? "a joint launch" : ((has_tiles || p->ref_width || p->ref_height) ? "tiles" : (n_sets > 0 ? "scaling lists" : nullptr));
  return kvz::inter_me_known(p, excluded, joint ? "kvz_hip_dev_inter_ctu_pass_groups" : "kvz_hip_dev_inter_ctu_pass") ? 0 : -1;
}

// what the searches met since the last reset (kvz_inter_ctu_pix.inc g_me_events): out[16]
extern "C" void kvz_hostsim_me_events(unsigned long long *out, int reset)
{
  for (int i = 0; i < 16; i++) { out[i] = kvz::g_me_events[i]; if (reset) kvz::g_me_events[i] = 0; }
}

// kvz_hip_dev_inter_ctu_pass_pictures on the host with the launch's choice of search: the arguments of kvz_hostsim_inter_pass_pictures.  Returns 0, -1 for what the
// library refuses (nothing is computed then), -2 when a search loop reached its bound.
extern "C" int kvz_hostsim_inter_pass_me(int width, int height, int n_pictures, const kvz_hip_inter_params *p, const kvz_hip_inter_pictures *pictures,
                                         const uint64_t *coeff_weights_of_qp, const float *fbits, const uint8_t *src, const uint8_t *ref, const kvz_hip_cu_info *ref_cu,
                                         uint8_t *rec, kvz_hip_cu_info *cu, int16_t *coeff, const int32_t *tile_xy, int n_references)
{
  kvz_hip_inter_params full;
  if (!kvz::inter_params_full(p, &full, "kvz_hip_dev_inter_ctu_pass")) return -1;
  p = &full;
  if (pictures && !kvz::inter_pictures_known(pictures, n_pictures, "kvz_hostsim_inter_pass_me")) return -1;
  if (kvz::inter_pass_geometry_refused(width, height, n_pictures, p->ref_width, p->ref_height, p->tile_x, p->tile_y)) return -1;
  if (kvz_hostsim_inter_me_check(p, tile_xy != nullptr, 0, 0)) return -1;
  if (!kvz::inter_me_chosen(p)) return kvz_hostsim_inter_pass_pictures(width, height, n_pictures, p, pictures, coeff_weights_of_qp, fbits, src, ref, ref_cu, rec, cu, coeff, tile_xy, n_references);
  static kvz::Tables tb;
  kvz::build_tables(&tb);
  auto model_at_qp = [&](kvz::InterModel *row, int qp) {
    kvz::inter_model_init(row, qp, p->poc, coeff_weights_of_qp[qp], fbits, p->mv_constraint, p->sao, p->deblock, p->fme_level, p->pu_depth_inter_max, p->no_wpp, p->fast_residual_cost,
                          width, height, 0, 0, 0, 0, p->no_tmvp);
    kvz::inter_model_set_me(row, p);
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
  g_kvz_ictu_me = 1;
  kvz::InterCtu::begin_launch(F, pictures ? table.model_of_picture(table.image.data(), 0) : &m, &tb, slab);
  int overrun = 0;
  for (const uint32_t item : items) {
    kvz::InterCtu::begin_ctu((int)(item >> 16), (int)(item & 0xff) * 64, (int)((item >> 8) & 0xff) * 64);
    kvz::InterCtu::run();
    overrun |= kvz::g_ic.me_overrun;
  }
  g_kvz_ictu_me = 0;
  free(F.ctx_out); free(slab);
  return overrun ? -2 : 0;
}

// me_integer for ONE PU on given pictures and candidates: src / ref are whole pictures (Y|U|V) of width x height, the PU the w x w block at (x, y), mv_cand the two
// AMVP predictors, merge n_merge records of {mv[2][2], dir} (int16 x 4, then dir as int16), (sx, sy) the co-located motion if has_start.  The model is the
// launch's at p->qp.  out_mv[2] (quarter samples), out_cost, out_bits: L->best as the program leaves it.  Returns -2 when a search loop reached its bound.
extern "C" int kvz_hostsim_me_integer_pu(int width, int height, const kvz_hip_inter_params *p, const uint64_t *coeff_weights_of_qp, const float *fbits, const uint8_t *src,
                                         const uint8_t *ref, int x, int y, int w, const int16_t *mv_cand, const int16_t *merge, int n_merge, int has_start, int sx, int sy,
                                         int32_t *out_mv, double *out_cost, double *out_bits)
{
  if (kvz_hostsim_inter_me_check(p, 0, 0, 0) || n_merge < 0 || n_merge > 5) return -1;
  static kvz::Tables tb;
  kvz::build_tables(&tb);
  kvz::InterModel m;
  kvz::inter_model_init(&m, p->qp, p->poc, coeff_weights_of_qp[p->qp], fbits, p->mv_constraint, p->sao, p->deblock, p->fme_level, p->pu_depth_inter_max, p->no_wpp, p->fast_residual_cost,
                        width, height, 0, 0, 0, 0, p->no_tmvp);
  kvz::inter_model_set_me(&m, p);
  kvz::InterFrames F;
  memset(&F, 0, sizeof F);
  F.W = width; F.H = height; F.wc = (width + 63) / 64; F.hc = (height + 63) / 64; F.frame_px = (long)width * height * 3 / 2; F.cells = (long)(width / 4) * (height / 4);
  std::vector<kvz_hip_cu_info> cells((size_t)F.cells);
  std::vector<uint8_t> rec((size_t)F.frame_px);
  F.src = src; F.ref = ref; F.ref_cu = cells.data(); F.rec = rec.data(); F.cu = cells.data();
  kvz::InterSlab *slab = (kvz::InterSlab *)calloc(1, sizeof(kvz::InterSlab));
  F.slabs = slab;
  g_kvz_ictu_me = kvz::inter_me_chosen(p) ? 1 : 0;
  kvz::InterCtu::begin_launch(F, &m, &tb, slab);
  kvz::InterCtu::begin_ctu(0, x & ~63, y & ~63);
  kvz::PuSearch &pu = kvz::g_il.pu;
  memset(&pu, 0, sizeof pu);
  pu.x = x; pu.y = y; pu.w = w;
  for (int i = 0; i < 4; i++) pu.mv_cand[i >> 1][i & 1] = mv_cand[i];
  pu.num_merge = n_merge;
  for (int i = 0; i < n_merge; i++) {
    for (int k = 0; k < 4; k++) pu.merge[i].mv[k >> 1][k & 1] = merge[5 * i + k];
    pu.merge[i].dir = (uint8_t)merge[5 * i + 4];
  }
  kvz::InterCtu::load_org_quadrant(x & ~31, y & ~31);
  kvz::InterCtu::me_integer(has_start != 0, sx, sy);
  out_mv[0] = kvz::g_il.best.mvx; out_mv[1] = kvz::g_il.best.mvy; *out_cost = kvz::g_il.best.cost; *out_bits = kvz::g_il.best.bits;
  const int overrun = kvz::g_ic.me_overrun;
  g_kvz_ictu_me = 0;
  free(slab);
  return overrun ? -2 : 0;
}
