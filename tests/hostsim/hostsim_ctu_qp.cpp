// hostsim_ctu_qp.cpp -- TEST INFRASTRUCTURE (see hostsim.cpp and hostsim_models.cpp, which this unit includes whole: one library with everything of
// libkvz_hostsim_models.so plus what a cost model per CTU adds).  kvz_hip_ctu_models on the host: the check the library makes (kvz_cu_qp.hpp ctu_models_known), the pass
// with every CTU under the row its map names -- fetched as ticket_loop's CTUQP branch fetches it, through the build kvz_batch.hpp launches (kvz_ctu_qp_builds.hpp) --
// and the three steps that derive the QP of every CU, each lane a loop iteration.  tests/ctu_qp_common.py builds and uses it.
#include "hostsim_models.cpp"
#include "../../kvazaar_amd/csrc/kvz_cu_qp.hpp"

// The build list and the choice (kvz_ctu_qp_builds.hpp).  rows [n][3]: unit, CABAC, S32 of every build of the list; returns n.  *unit_mask: the translation units, a bit each.
extern "C" int kvz_hostsim_ctu_qp_builds(int *rows, unsigned long long *unit_mask)
{
#define KVZ_CTU_QP_X(...) __VA_ARGS__,
  const int list[] = { KVZ_CTU_QP_BUILDS(KVZ_CTU_QP_X) };
#undef KVZ_CTU_QP_X
  memcpy(rows, list, sizeof list);
  *unit_mask = kvz::KVZ_CTU_QP_UNIT_MASK;
  return (int)(sizeof list / sizeof list[0] / 3);
}
extern "C" int kvz_hostsim_ctu_qp_build_choose(int search_32x32, int any_cabac) { return kvz::ctu_qp_build_choose(search_32x32 != 0, any_cabac != 0); }

// 0 when a batch of n_frames width x height pictures accepts the map, -1 when the library refuses it (ticket_schedule == 0: as under KVZ_HIP_SCHED=wave; lists: the batch has scaling lists)
extern "C" int kvz_hostsim_ctu_models_check(const kvz_hip_ctu_models *cm, int width, int height, int n_frames, int ticket_schedule, int lists)
{
  return kvz::ctu_models_known(cm, n_frames, ((width + 63) / 64) * ((height + 63) / 64), ticket_schedule != 0, lists != 0, "kvz_hostsim_ctu_models_check") ? 0 : -1;
}

// The three steps of kvz_cu_qp.hpp on the host: coeff / cu_depth as a pass left them, qp_of_ctu [n_frames][ctu] and qp_of_picture [n_frames] -> cu_qp, ctu_qp (kvz_hip_batch_download_cu_qps)
extern "C" void kvz_hostsim_cu_qps(int width, int height, int n_frames, int no_wpp, const int16_t *coeff, const uint8_t *cu_depth, const uint8_t *qp_of_ctu, const int32_t *qp_of_picture,
                                   uint8_t *cu_qp, uint32_t *ctu_qp)
{
  const kvz::CuQpJob J{ width, height, (width + 63) / 64, (height + 63) / 64, n_frames, no_wpp, coeff, cu_depth, qp_of_ctu, qp_of_picture, cu_qp, ctu_qp };
  for (long f = 0; f < n_frames; f++)
    for (int cy = 0; cy < J.hc; cy++)
      for (int cx = 0; cx < J.wc; cx++) {
        unsigned long long bits = 0;  // (the device: a ballot over the wavefront)
        for (int lane = 0; lane < 64; lane++) bits |= (unsigned long long)kvz::cu_qp_unit_bit(J, f, cx, cy, lane) << lane;
        ctu_qp[(f * J.hc + cy) * J.wc + cx] = kvz::cu_qp_ctu_word(J, f, cx, cy, bits);
      }
  for (long c = 0; c < (long)n_frames * (no_wpp ? 1 : J.hc); c++) kvz::cu_qp_chain(J, c);
  for (long f = 0; f < n_frames; f++)
    for (int y8 = 0; y8 < height / 8; y8++)
      for (int x8 = 0; x8 < width / 8; x8++) kvz::cu_qp_unit(J, f, x8, y8);
}

// The SAO decision of kvz_hip_batch_loop_filters_ctu_models on the host for one picture: kvz_hostsim_sao_decide (hostsim.cpp: the statistics by plain loops over the
// R / V / D view, the device's candidate code) with the chain as dev_sao_chain_kernel_ctu runs it -- every LCU under lambda_of_lcu [lcu], the two contexts from the
// slice model `m`.
extern "C" void kvz_hostsim_sao_decide_ctu(const kvz_hip_intra_cost_model *m, const double *lambda_of_lcu, int width, int height, const uint8_t *src, const uint8_t *R,
                                           const uint8_t *V, const uint8_t *D, kvz_hip_sao_params *luma, kvz_hip_sao_params *chroma, uint8_t *merge)
{
  using namespace kvz;
  const int wl = (width + 63) / 64, hl = (height + 63) / 64;
  std::vector<SaoStats> stats((size_t)wl * hl * 3);
  std::vector<SaoCand> cand((size_t)wl * hl * 3);
  std::vector<SaoRec> recs((size_t)wl * hl * 3);
  for (int lcu = 0; lcu < wl * hl; lcu++)
    for (int color = 0; color < 3; color++) {
      const int lx = lcu % wl, ly = lcu / wl, sh = color ? 1 : 0, n = 64 >> sh, fw = width >> sh, fh = height >> sh;
      const long plane = color == 0 ? 0 : (color == 1 ? (long)width * height : (long)width * height * 5 / 4);
      const int bw = imin(n, fw - lx * n), bh = imin(n, fh - ly * n);
      SaoView view{ R + plane, V + plane, D + plane, fw, n, lx * n, ly * n, lx == wl - 1, ly == hl - 1, color ? 1 : 3 };
      SaoStats &st = stats[(size_t)lcu * 3 + color];
      memset(&st, 0, sizeof st);
      for (int y = 0; y < bh; y++)
        for (int x = 0; x < bw; x++) {
          const int c = view.at(x, y), diff = (int)src[plane + (long)(ly * n + y) * fw + lx * n + x] - c;
          st.band_sum[c >> 3] += diff;
          st.band_cnt[c >> 3]++;
          if (x >= 1 && x < bw - 1 && y >= 1 && y < bh - 1)
            for (int ec = 0; ec < 4; ec++) {
              int ax, ay, bx, by;
              eo_offsets(ec, ax, ay, bx, by);
              const int cat = eo_cat(view.at(x + ax, y + ay), view.at(x + bx, y + by), c);
              st.edge_sum[ec][cat] += diff;
              st.edge_cnt[ec][cat]++;
            }
        }
      sao_candidates(st, cand[(size_t)lcu * 3 + color]);
    }
  sao_chain_picture(m->entropy_fbits, host_tables()->ctx_next[0], host_tables()->ctx_next[1], m->lambda, m->ctx_init[KVZ_HIP_CX_SAO_MERGE], m->ctx_init[KVZ_HIP_CX_SAO_TYPE], m->no_wpp, wl, hl,
                    stats.data(), cand.data(), recs.data(), merge, lambda_of_lcu);
  for (int i = 0; i < wl * hl; i++) {
    auto unpack = [&](kvz_hip_sao_params *o, int plane, int slot) {
      const SaoRec r = recs[(size_t)i * 3 + plane];
      if (slot == 0) { memset(o, 0, sizeof *o); o->bitdepth = 8; o->type = (int)(r & 0xff); o->eo_class = (int)((r >> 8) & 0xff); }
      o->band_position[slot] = (int)((r >> 16) & 0xff);
      for (int k = 0; k < 5; k++) o->offsets[5 * slot + k] = (int)(int8_t)(r >> (24 + 8 * k));
    };
    unpack(&luma[i], 0, 0);
    unpack(&chroma[i], 1, 0);
    unpack(&chroma[i], 2, 1);
  }
}

// kvz_hip_intra_frames_ctu_models on the host: src / rec / ... hold the n_frames pictures back to back in the batch's layouts; cu_qp / ctu_qp as kvz_hip_batch_download_cu_qps
// hands them out.  Returns 0, or -1 for a map the library refuses (nothing is computed then).
extern "C" int kvz_hostsim_intra_frames_ctu_models(const kvz_hip_ctu_models *cm, int width, int height, int n_frames, const uint8_t *src, uint8_t *rec, int16_t *coeff,
                                                   uint8_t *cu_depth, uint8_t *cu_mode, double *ctu_cost, uint8_t *cu_qp, uint32_t *ctu_qp)
{
  const int ctus = ((width + 63) / 64) * ((height + 63) / 64);
  if (!kvz::ctu_models_known(cm, n_frames, ctus, true, false, "kvz_hostsim_intra_frames_ctu_models")) return -1;
  const kvz_hip_picture_models *pm = cm->pictures;
  HostFrames hf(width, height, n_frames, src, rec, coeff, cu_depth, cu_mode, ctu_cost);
  const HostModelTable T(pm);
  const bool ran = kvz::ctu_qp_build_dispatch(kvz::ctu_models_build(cm), [&](auto bt) {
    for (int f = 0; f < n_frames; f++)
      for (int cy = 0; cy < hf.F.hc; cy++)
        for (int cx = 0; cx < hf.F.wc; cx++) {
          kvz::CtuModel m = T.table.models[cm->model_of_ctu[(long)f * ctus + cy * hf.F.wc + cx]];  // what thread 0 of a workgroup loads for the CTU it drew
          m.ctx_init = kvz::picture_model(T.table, f)->ctx_init;
          kvz::CtuProgramT<decltype(bt)::cabac != 0, decltype(bt)::s32 != 0, false, false, false, true> p;  // (ticket_loop's CTUQP instantiation)
          p.m = &m; p.tb = host_tables(); p.F = hf.F; p.s = (kvz::CtuSharedT<decltype(bt)::cabac != 0> *)hf.shared.data(); p.frame = f; p.cx = cx * 64; p.cy = cy * 64;
          p.run();
        }
  });
  if (!ran) return -1;
  std::vector<uint8_t> qp_of_ctu((size_t)n_frames * ctus);
  std::vector<int32_t> qp_of_picture((size_t)n_frames);
  for (size_t i = 0; i < qp_of_ctu.size(); i++) qp_of_ctu[i] = (uint8_t)pm->models[cm->model_of_ctu[i]].qp;  // as kvz_batch.hpp ctu_models_stage / picture_models_stage lay them out
  for (int f = 0; f < n_frames; f++) qp_of_picture[(size_t)f] = pm->models[pm->model_of_picture[f]].qp;
  kvz_hostsim_cu_qps(width, height, n_frames, pm->models[0].no_wpp != 0, coeff, cu_depth, qp_of_ctu.data(), qp_of_picture.data(), cu_qp, ctu_qp);
  return 0;
}

// kvz_hip_batch_entropy_code_ctu_models on the host: kvz_hostsim_entropy_code_models (hostsim_models.cpp) with stage 1 as dev_entropy_bins_phased_kernel_cuqp runs it --
// every CTU's cu_qp_delta from its word of the CU-QP step (ctu_qp [n_frames][ctu]) -- and the rows as kvz_batch.hpp picture_models_stage lays them out: a model's initial
// states and, in the two bytes of cu_qp_delta_abs, init value 154 at the row's QP.  The substreams are coded twice, counting and writing; -2 when the two disagree.
extern "C" long kvz_hostsim_entropy_code_ctu_models(const kvz_hip_ctu_models *cm, int width, int height, int n_frames, const uint8_t *cu_depth, const uint8_t *cu_mode,
                                                    const int16_t *coeff, const uint32_t *ctu_qp, const unsigned long long *sao_recs, const uint8_t *sao_merge, uint32_t cap,
                                                    uint8_t *out, uint32_t *substream_bytes, uint32_t *most_records)
{
  const int ctus = ((width + 63) / 64) * ((height + 63) / 64);
  if (!kvz::ctu_models_known(cm, n_frames, ctus, true, false, "kvz_hostsim_entropy_code_ctu_models")) return -1;
  const kvz_hip_picture_models *pm = cm->pictures;
  static kvz::Tables tb;
  kvz::build_tables(&tb);
  const kvz_hip_intra_cost_model *m = &pm->models[0];
  kvz::EntropyJob J;
  memset(&J, 0, sizeof J);
  J.W = width; J.H = height; J.wc = (width + 63) / 64; J.hc = (height + 63) / 64; J.n_frames = n_frames; J.no_wpp = m->no_wpp;
  J.depth = cu_depth; J.mode = cu_mode; J.coeff = coeff; J.sao = sao_recs; J.sao_merge = sao_merge;
  std::vector<uint8_t> rows((size_t)pm->n_models * KVZ_ENTROPY_CTX_ROW, 0);
  for (int i = 0; i < pm->n_models; i++) {
    uint8_t *row = &rows[(size_t)i * KVZ_ENTROPY_CTX_ROW];
    memcpy(row, pm->models[i].ctx_init, sizeof pm->models[i].ctx_init);
    const int qp = pm->models[i].qp, slope = (154 >> 4) * 5 - 45, offset = ((154 & 15) << 3) - 16;  // context.c:202-213 kvz_ctx_init of init value 154
    int st = ((slope * qp) >> 4) + offset;
    st = st < 1 ? 1 : (st > 126 ? 126 : st);
    row[kvz::KVZ_EB_CX_QP_DELTA] = row[kvz::KVZ_EB_CX_QP_DELTA + 1] = (uint8_t)(st >= 64 ? ((st - 64) << 1) + 1 : (63 - st) << 1);
  }
  J.ctx_rows = rows.data(); J.model_of_picture = pm->model_of_picture;
  const long items = (long)n_frames * ctus, streams = (long)n_frames * (m->no_wpp ? 1 : J.hc);
  cap = (cap + 15u) & ~15u;
  J.bins = (uint32_t *)aligned_alloc(64, (size_t)items * cap * sizeof(uint32_t)); J.nbins = (uint32_t *)malloc((size_t)items * sizeof(uint32_t)); J.nbits = (uint32_t *)malloc((size_t)items * sizeof(uint32_t)); J.cap = cap;
  J.row_ctx = (uint8_t *)malloc((size_t)n_frames * J.hc * KVZ_ENTROPY_CTXS);
  const kvz::EntropyTabs T{ &tb.ctx_next[0][0] };
  uint8_t ctx[KVZ_ENTROPY_CTXS];
  *most_records = 0;
  for (long i = 0; i < items; i++) {
    uint32_t queue[kvz::DeferSink::QCAP];
    uint16_t stack[16];
    kvz::entropy_ctu_bins_phased<true>(J, &tb, i, true, queue, stack, 1, ctu_qp);
    if (J.nbins[i] > *most_records) *most_records = J.nbins[i];
  }
  long total = -1;
  if (*most_records <= cap) {
    if (!m->no_wpp) for (int f = 0; f < n_frames; f++) kvz::entropy_row_contexts(J, T, f, ctx);
    total = 0;
    for (long i = 0; i < streams; i++) {
      unsigned long long bits = 0;
      const long per_stream = m->no_wpp ? (long)ctus : J.wc;
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
