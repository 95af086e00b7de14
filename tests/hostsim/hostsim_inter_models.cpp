// hostsim_inter_models.cpp -- TEST INFRASTRUCTURE (see hostsim.cpp, which this unit includes whole: one library with everything of libkvz_hostsim.so plus the twin
// of kvz_hip_dev_inter_ctu_pass_pictures).  A launch of the inter CTU pass whose pictures have a QP and a POC of their own (kvz_hip_inter_pictures), walked on the host
// as ONE persistent workgroup walks it: the program's state is set up once (begin_launch), then the CTUs are taken in the launch's ticket order -- anti-diagonals,
// pictures interleaved -- so that consecutive CTUs belong to different pictures, QPs and POCs, and whatever the program keeps from one CTU to the next meets another
// picture's.  The table is checked by the text the library checks it with (kvz_inter_pictures.hpp), laid out by the function the library lays it out with
// (kvz_inter_host.hpp inter_picture_table) and found by the kernel's own begin_ctu.  tests/test_inter_mixed_qp_sim.py builds and uses it.
#include "hostsim.cpp"
#include "../../kvazaar_amd/csrc/kvz_inter_pictures.hpp"
#include "../../kvazaar_amd/csrc/kvz_inter_builds.hpp"

// The build list and the choice (kvz_inter_builds.hpp), for tests/test_inter_builds_sim.py.  rows [n][7]: unit, CABAC, LISTS, JOINT, ME, P, REFS of every build of the
// list; returns n.  *unit_mask: the translation units, a bit each.  kvz_hostsim_inter_build_suffix: the suffix of a unit's kernel name
extern "C" int kvz_hostsim_inter_builds(int *rows, unsigned long long *unit_mask)
{
#define KVZ_ICTU_X(unit, suffix, ...) unit, __VA_ARGS__,
  const int list[] = { KVZ_ICTU_BUILDS(KVZ_ICTU_X) };
#undef KVZ_ICTU_X
  memcpy(rows, list, sizeof list);
  *unit_mask = kvz::KVZ_ICTU_UNIT_MASK;
  return (int)(sizeof list / sizeof list[0] / 7);
}
extern "C" const char *kvz_hostsim_inter_build_suffix(int unit) { return kvz::inter_build_suffix(unit); }
extern "C" int kvz_hostsim_inter_build_choose(int any_cabac, int lists, int joint, int me, int p_slice, int refs)
{
  return kvz::inter_build_choose({ any_cabac != 0, lists != 0, joint != 0, me != 0, p_slice != 0, refs != 0 });
}

// 0 when a launch of n_pictures accepts the table / the bare QP array (the loop filters), -1 when the library refuses it
extern "C" int kvz_hostsim_inter_pictures_check(const kvz_hip_inter_pictures *ip, int n_pictures)
{
  return kvz::inter_pictures_known(ip, n_pictures, "kvz_hostsim_inter_pictures_check") ? 0 : -1;
}
extern "C" int kvz_hostsim_inter_picture_qps_check(const int32_t *qp, int n_pictures)
{
  return kvz::inter_picture_qps_known(qp, n_pictures, "kvz_hostsim_inter_picture_qps_check") ? 0 : -1;
}

// kvz_hip_dev_inter_ctu_pass_pictures on the host: src / ref / ref_cu / rec / cu / coeff hold the n_pictures pictures back to back in the pass's layouts (coeff may be
// null; tile_xy is a host array here).  coeff_weights_of_qp[52] / fbits: the constants the library has built in (kvz_fast_coeff_cost's weights per QP, kvz_f_entropy_bits).
// pictures == NULL: params->qp / params->poc for every picture.  Returns 0, or -1 for a table the library refuses (nothing is computed then).
extern "C" int kvz_hostsim_inter_pass_pictures(int width, int height, int n_pictures, const kvz_hip_inter_params *p, const kvz_hip_inter_pictures *pictures,
                                               const uint64_t *coeff_weights_of_qp, const float *fbits, const uint8_t *src, const uint8_t *ref, const kvz_hip_cu_info *ref_cu,
                                               uint8_t *rec, kvz_hip_cu_info *cu, int16_t *coeff, const int32_t *tile_xy, int n_references)
{
  if (pictures && !kvz::inter_pictures_known(pictures, n_pictures, "kvz_hostsim_inter_pass_pictures")) return -1;
  if (kvz::inter_pass_geometry_refused(width, height, n_pictures, p->ref_width, p->ref_height, p->tile_x, p->tile_y)) return -1;
  static kvz::Tables tb;
  kvz::build_tables(&tb);
  auto model_at_qp = [&](kvz::InterModel *row, int qp) {
    kvz::inter_model_init(row, qp, p->poc, coeff_weights_of_qp[qp], fbits, p->mv_constraint, p->sao, p->deblock, p->fme_level, p->pu_depth_inter_max, p->no_wpp, p->fast_residual_cost,
                          width, height, p->ref_width, p->ref_height, p->tile_x, p->tile_y, p->no_tmvp);
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
  F.tile_xy = (p->ref_width || p->ref_height) ? tile_xy : nullptr;
  F.ref_count = n_references > 0 ? n_references : 0;
  F.pictures = pictures ? (const kvz::InterPicture *)table.image.data() : nullptr;
  memset(cu, 0, (size_t)F.cells * n_pictures * sizeof(kvz_hip_cu_info));
  std::vector<uint32_t> items;
  kvz::inter_ticket_items(F.wc, F.hc, n_pictures, p->no_wpp, items);
  kvz::InterCtu::begin_launch(F, pictures ? table.model_of_picture(table.image.data(), 0) : &m, &tb, slab);
  for (const uint32_t item : items) {
    kvz::InterCtu::begin_ctu((int)(item >> 16), (int)(item & 0xff) * 64, (int)((item >> 8) & 0xff) * 64);
    kvz::InterCtu::run();
  }
  free(F.ctx_out); free(slab);
  return 0;
}

// kvz_hip_dev_entropy_code_inter_pictures on the host: kvz_hostsim_entropy_code_inter over n_pictures pictures with every picture's initial context states from its QP's
// row and its own POC (0: no temporal predictors).  ctx_rows: n_rows x KVZ_ENTROPY_CTX_ROW bytes; row_of_picture / poc_of_picture: [n_pictures]
extern "C" long kvz_hostsim_entropy_code_inter_pictures(const uint8_t *ctx_rows, const uint16_t *row_of_picture, const int32_t *poc_of_picture, int width, int height, int n_pictures,
                                                        int no_wpp, const kvz_hip_cu_info *cu, const kvz_hip_cu_info *ref_cu, const int16_t *coeff, const unsigned long long *sao_recs,
                                                        const uint8_t *sao_merge, uint32_t cap, uint8_t *out, uint32_t *substream_bytes)
{
  static kvz::Tables tb;
  kvz::build_tables(&tb);
  kvz::EntropyJob J;
  memset(&J, 0, sizeof J);
  J.W = width; J.H = height; J.wc = (width + 63) / 64; J.hc = (height + 63) / 64; J.n_frames = n_pictures; J.no_wpp = no_wpp;
  J.cu = cu; J.ref_cu = ref_cu; J.coeff = coeff; J.sao = sao_recs; J.sao_merge = sao_merge;
  J.ctx_rows = ctx_rows; J.model_of_picture = row_of_picture; J.poc_of_picture = poc_of_picture;
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
