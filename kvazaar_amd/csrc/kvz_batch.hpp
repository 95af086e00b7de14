// kvz_batch.hpp -- host side of the batched CTU pass: device buffers of a frame batch, the launches of the CTU kernels (kvz_ctu_kernels.hpp: persistent launch
// with an in-order ticket list; one launch per anti-diagonal kept for A/B), the cost model.  Included by kvz_hip.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include <vector>

#include "../../include/kvz_hip_batch.h"
#include "kvz_ctu.hpp"
#include "kvz_entropy.hpp"  // KVZ_ENTROPY_CTX_ROW: the rows of a model table
#include "kvz_joint.hpp"
#include "kvz_picture_models.hpp"
#include "kvz_runtime.hpp"
#include "kvz_scaling_lists.hpp"

#include "kvz_ctu_kernels.hpp"
#include "kvz_cu_qp.hpp"

namespace kvz {
struct DevBuf { void *p = nullptr; size_t bytes = 0; };  // a grow-only device buffer (kvz_dev.hpp EntropyScratch::need)

// The words of a batch's or a group's ticket schedule.  Device: the ticket, the sticky error word, two words of what the first CTU to give up saw, the launch's tables
// (KVZ_SCHED_TABLE_AT, KVZ_SCHED_LISTS_AT).  Pinned: the error words as the last pass left them (a synchronous copy would wait for all the copy engine holds: 84 ms).
struct TicketWords {
  unsigned *d_ticket = nullptr, *d_error = nullptr, *h_error = nullptr;
  void create(hipStream_t stream)  // the stream of the passes (a non-blocking stream does not order against the null stream)
  {
    KVZ_HIP_CHECK(hipMalloc((void **)&d_ticket, KVZ_SCHED_TICKET_WORDS * sizeof(unsigned)));
    KVZ_HIP_CHECK(hipMemsetAsync(d_ticket, 0, KVZ_SCHED_TICKET_WORDS * sizeof(unsigned), stream));
    KVZ_HIP_CHECK(hipStreamSynchronize(stream));
    d_error = d_ticket + 1;
    KVZ_HIP_CHECK(hipHostMalloc((void **)&h_error, 64, hipHostMallocDefault));
    h_error[0] = h_error[1] = h_error[2] = 0;
  }
  void destroy() { (void)hipFree(d_ticket); if (h_error) (void)hipHostFree(h_error); }
  void clear_error() { KVZ_HIP_CHECK(hipMemset(d_error, 0, 3 * sizeof(unsigned))); h_error[0] = h_error[1] = h_error[2] = 0; }  // the sticky word (the stream of the passes has drained)
  unsigned error(int i = 0) const { return ((volatile unsigned *)h_error)[i]; }
  // one pass on `stream`: launch() between ev0 and ev1, in front of it the ticket zeroed (the error word behind it stays: sticky across passes), behind it the copy of the error words
  template <class Launch> void pass(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, Launch &&launch)
  {
    KVZ_HIP_CHECK(hipMemsetAsync(d_ticket, 0, sizeof(unsigned), stream));
    KVZ_HIP_CHECK(hipEventRecord(ev0, stream));
    launch();
    KVZ_HIP_CHECK(hipGetLastError());
    KVZ_HIP_CHECK(hipEventRecord(ev1, stream));
    KVZ_HIP_CHECK(hipMemcpyAsync(h_error, d_error, 3 * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
  }
};
}  // namespace kvz

struct kvz_hip_batch {
  kvz::CtuFrames F;
  int n_frames;
  hipStream_t stream;
  hipEvent_t ev0, ev1;
  hipEvent_t ev_up = nullptr;  // kvz_hip_batch_upload_all_async: what the next pass waits for
  int up_pending = 0;
  hipEvent_t ev_src_read = nullptr;  // behind the last reader of d_src that is not the pass (kvz_hip_batch_sse_async): what kvz_hip_batch_upload_all_async also waits for
  int src_read_set = 0;              // ... once one has been recorded (never, unless such a reader was queued)
  unsigned long long *d_sse = nullptr;  // kvz_hip_batch_sse: n_frames x 3 sums (allocated on first use)
  uint8_t *d_src, *d_rec, *d_depth, *d_mode;
  uint8_t *d_part, *d_mode4;  // search_nxn: NxN flag per 8x8 CU, luma mode per 4x4 unit (allocated with the first model that has it set)
  int16_t *d_coeff, *d_scratch;
  double *d_cost;
  uint8_t *d_border;
  unsigned long long *d_prof;
  float *d_entropy;  // the model's entropy_fbits [128 floats] followed by its ctx_init [160 bytes] of the run in flight
  uint32_t *d_items, *d_items_raster;  // ticket order with WPP (anti-diagonals) / without (raster order per picture)
  unsigned *d_done;
  kvz::TicketWords tw;
  float last_entropy[128 + 40];  // the price table and initial contexts d_entropy holds (a launch with the same model skips the copy)
  int entropy_valid = 0;
  int entropy_deferred = 0;     // kvz_hip_batch_entropy_defer_download: the coder's calls return with the slice data's download queued, not finished
  kvz::DevBuf entropy_out;      // ... and compact into this buffer of the batch's own instead of the device's shared one
  unsigned total_items, epoch;
  int sched_ticket, grid_ticket;
  int slots_per_cu, cus;  // what the persistent pass may occupy at most (occupancy x CU count); grid_ticket = its share of that (kvz_hip_batch_set_device_share)
  // SAO (kvz_hip_batch_loop_filters with sao != 0; allocated on first use): the picture after the vertical edges and after all edges,
  // statistics / context-free candidates / packed parameter records per (LCU, plane), merge choice per LCU
  uint8_t *d_ver, *d_dbk, *d_sao_merge;
  void *d_sao_stats, *d_sao_cand;
  unsigned long long *d_sao_recs;
  float *d_sao_fbits;
  // the model table of the kvz_hip_*_models entry points on the device -- the two pointers of a CtuModelTable (also behind the ticket words, for the pass) | CtuModel rows | their ctx_init rows | qp_of_picture | model_of_picture (kvz::ModelTableView) --
  // and the host image it was copied from: a call with the same table skips the copy, like last_entropy
  kvz::DevBuf d_models;
  std::vector<uint8_t> h_models;
  // scaling lists (kvz_hip_batch_set_scaling_lists; n_list_sets == 0: none): the factor rows of every set and, behind them, of the flat list (kvz_scaling_lists.hpp),
  // and every picture's set.  On the device, staged per launch like the model table (scaling_lists_stage): the rows | every picture's two rows at its QP
  int n_list_sets = 0;
  std::vector<uint32_t> list_rows;
  std::vector<uint16_t> list_set_of_picture;
  kvz::DevBuf d_lists;
  std::vector<uint32_t> h_lists;
  // a model per CTU (kvz_hip_intra_frames_ctu_models; allocated on first use).  Staged per launch like the model table (ctu_models_stage): every CTU's lambda | its row
  // of the table (also behind the ticket words, for the pass) | its QP.  What the step behind the pass leaves (kvz_cu_qp.hpp): the QP of every 8x8 unit and a word per
  // CTU, and the pass they belong to (0: none)
  kvz::DevBuf d_ctu_map;
  std::vector<uint8_t> h_ctu_map;
  uint8_t *d_cu_qp = nullptr;
  uint32_t *d_ctu_qp = nullptr;
  unsigned cu_qp_epoch = 0;
  hipEvent_t ev_cu_qp0 = nullptr, ev_cu_qp1 = nullptr;  // around that step (kvz_hip_batch_last_cu_qp_ms)
  int device;  // the batch's buffers and stream live here; every entry point binds the calling thread to it
  int failed;   // sticky: a CTU hand-off wait of some run timed out, the results of that run are invalid
  unsigned long long wait_ticks;
  kvz_hip_batch_group *joint = nullptr;  // the group whose joint pass was the last one queued on this batch (kvz_hip_batch_group_intra_frames): batch_check also reads ITS error word; cleared by kvz_hip_batch_reset
};

namespace kvz {
int joint_check(kvz_hip_batch *b);  // (below, with the group)
// kvazaar worker threads other than the creating one call into a batch (search_lcu_hip.c): bind them to the batch's device
inline void batch_enter(const kvz_hip_batch *b) { KVZ_HIP_CHECK(hipSetDevice(b->device)); thread_state().bound = true; }
// after the stream has drained: did a hand-off wait time out?  0 ok, -1 invalid results (reported, never fatal: the embedding
// encoder decides what to do)
inline int batch_check(kvz_hip_batch *b)
{
  if (b->joint && !b->failed) joint_check(b);
  if (b->sched_ticket && !b->failed) {
    if (const unsigned err = b->tw.error()) {
      const HandoffTag tag = handoff_tag_read(err);
      b->failed = 1;
      fprintf(stderr, "kvz_hip: a CTU hand-off wait timed out (KVZ_HIP_WAIT_MS to raise the bound) -- the results of this batch are invalid [first to give up waited for CTU x %u y %u of picture %u (%s), pass %u of the batch; that CTU's flag read at the memory side then: %u; tickets drawn then: %u of %u]\n",
              tag.x, tag.y, tag.picture, tag.neighbour, b->epoch, b->tw.error(1), b->tw.error(2), b->total_items);
    }
  }
  return b->failed ? -1 : 0;
}
// a reader of the source pictures other than the pass has just been queued on the batch's stream: the next kvz_hip_batch_upload_all_async copies behind it
inline void batch_src_read(kvz_hip_batch *b)
{
  if (!b->ev_src_read) KVZ_HIP_CHECK(hipEventCreateWithFlags(&b->ev_src_read, hipEventDisableTiming));
  KVZ_HIP_CHECK(hipEventRecord(b->ev_src_read, b->stream));
  b->src_read_set = 1;
}
}  // namespace kvz

namespace kvz {


// kvazaar's default fast-coefficient-cost weights per QP (fast_coeff_cost.h:48-101: four doubles per QP for |level| = 0, 1, 2, >= 3),
// packed as kvz_fast_coeff_use_default_table does (fast_coeff_cost.c:39-52, 76-82: Q8.8 each, |level| = 0 in the low word) --
// what kvz_fast_coeff_get_weights(state) returns unless --fastrd-learning-outdir / a custom table is used.  QP < 50
// (MAX_FAST_COEFF_COST_QP).  Constant data; tests/test_ctu_pipeline.py pins it against the reference build's values.
static const uint64_t kDefaultCoeffWeights[50] = {
  0x06f8038004200029ull, 0x06f8038004200029ull, 0x06f8038004200029ull, 0x06f8038004200029ull, 0x06f8038004200029ull,
  0x06f8038004200029ull, 0x06f8038004200029ull, 0x06f8038004200029ull, 0x06f8038004200029ull, 0x06f8038004200029ull,
  0x06f8038004200029ull, 0x06e5038f040a0028ull, 0x06f703eb044f0021ull, 0x06e603f2046c001cull, 0x06ce0429047b0018ull,
  0x06b9040b04a10013ull, 0x068f040004f6000dull, 0x067903f40522000aull, 0x066b03ce052f0009ull, 0x065a03c905340007ull,
  0x065903cc05510006ull, 0x065303d105390005ull, 0x065403f0052c0004ull, 0x064b042505170003ull, 0x0644043405040002ull,
  0x0635044e04f50002ull, 0x062d046704ea0001ull, 0x0622046304e80001ull, 0x0627048604df0001ull, 0x0627049704dd0001ull,
  0x0624049b04dd0001ull, 0x063b04cb04c60001ull, 0x064604ca04cb0000ull, 0x063c04ca04d80000ull, 0x064604ce04d90000ull,
  0x065904de04d70000ull, 0x067304f804c60000ull, 0x06aa050d04be0000ull, 0x069a050904cd0000ull, 0x06be051404cc0000ull,
  0x06df052504c80000ull, 0x073a053804ea0000ull, 0x0748052704f90000ull, 0x0696048305510000ull, 0x06c6048e054e0000ull,
  0x06f604b105430000ull, 0x071a04bc05310000ull, 0x075704d5052e0000ull, 0x075704d4052f0000ull, 0x0744048505640000ull,
};

// context.c:202-213 kvz_ctx_init
inline int ctx_state(int qp, int init_value)
{
  const int slope = (init_value >> 4) * 5 - 45, offset = ((init_value & 15) << 3) - 16;
  int st = ((slope * qp) >> 4) + offset;
  st = st < 1 ? 1 : (st > 126 ? 126 : st);
  return st >= 64 ? ((st - 64) << 1) + 1 : (63 - st) << 1;
}

inline void cost_model_init(int qp, uint64_t coeff_weights, kvz_hip_intra_cost_model *m)
{
  // I-slice rows of context.c:96-193 (HEVC spec tables 9-5 ff.); 154 = CNU, never coded
  static const uint8_t init_split[3] = { 139, 141, 157 }, init_cbf_luma[2] = { 111, 141 }, init_cbf_chroma[2] = { 94, 138 };
  static const uint8_t init_sig_cg[4] = { 91, 171, 134, 141 };
  static const uint8_t init_sig[42] = { 111, 111, 125, 110, 110, 94, 124, 108, 124, 107, 125, 141, 179, 153, 125, 107, 125, 141, 179, 153, 125, 107, 125, 141, 179, 153, 125,
                                        140, 139, 182, 182, 152, 136, 152, 136, 153, 136, 139, 111, 136, 139, 111 };
  static const uint8_t init_last[30] = { 110, 110, 124, 125, 140, 153, 125, 127, 140, 109, 111, 143, 127, 111, 79, 108, 123, 63,
                                         154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154 };
  static const uint8_t init_one[24] = { 140, 92, 137, 138, 140, 152, 138, 139, 153, 74, 149, 92, 139, 107, 122, 152, 140, 179, 166, 182, 140, 227, 122, 197 };
  static const uint8_t init_abs[6] = { 138, 153, 136, 167, 152, 152 };
  memset(m, 0, sizeof *m);
  m->struct_size = (uint32_t)sizeof *m;
  m->qp = qp;
  m->lambda = 0.57 * pow(2.0, (qp - 12) / 3.0);
  m->lambda_sqrt = sqrt(m->lambda);
  m->coeff_weights = coeff_weights;
  for (int i = 0; i < 128; i++) m->entropy_fbits[i] = (float)kEntropyBits[i] / 32768.0f;
  int n = 0;
  auto fill = [&](float dst[2], int init) {
    const int st = ctx_state(qp, init);
    m->ctx_init[n++] = (uint8_t)st;  // same order as the KVZ_HIP_CX_* indices
    dst[0] = m->entropy_fbits[st ^ 0];
    dst[1] = m->entropy_fbits[st ^ 1];
  };
  for (int i = 0; i < 3; i++) fill(m->split_flag[i], init_split[i]);
  fill(m->part_size, 184);
  fill(m->intra_mode, 184);
  fill(m->chroma_mode, 63);
  for (int i = 0; i < 2; i++) fill(m->cbf_luma[i], init_cbf_luma[i]);
  for (int i = 0; i < 2; i++) fill(m->cbf_chroma[i], init_cbf_chroma[i]);
  auto put = [&](int at, const uint8_t *init, int count) { for (int i = 0; i < count; i++) m->ctx_init[at + i] = (uint8_t)ctx_state(qp, init[i]); };
  put(KVZ_HIP_CX_SIG_CG, init_sig_cg, 4);
  put(KVZ_HIP_CX_SIG_LUMA, init_sig, 27);
  put(KVZ_HIP_CX_SIG_CHROMA, init_sig + 27, 15);
  put(KVZ_HIP_CX_LAST_Y_LUMA, init_last, 15);
  put(KVZ_HIP_CX_LAST_Y_CHROMA, init_last + 15, 15);
  put(KVZ_HIP_CX_LAST_X_LUMA, init_last, 15);
  put(KVZ_HIP_CX_LAST_X_CHROMA, init_last + 15, 15);
  put(KVZ_HIP_CX_ONE_LUMA, init_one, 16);
  put(KVZ_HIP_CX_ONE_CHROMA, init_one + 16, 8);
  put(KVZ_HIP_CX_ABS_LUMA, init_abs, 4);
  put(KVZ_HIP_CX_ABS_CHROMA, init_abs + 4, 2);
  {
    static const uint8_t init_cbf_chroma_deep[2] = { 182, 154 };  // INIT_QT_CBF[2][6..7] (context.c:130-134)
    put(KVZ_HIP_CX_CBF_CHROMA_DEEP, init_cbf_chroma_deep, 2);
  }
  m->ctx_init[KVZ_HIP_CX_SAO_MERGE] = (uint8_t)ctx_state(qp, 153);  // context.c:38-39 INIT_SAO_MERGE_FLAG / INIT_SAO_TYPE_IDX, I slice
  m->ctx_init[KVZ_HIP_CX_SAO_TYPE] = (uint8_t)ctx_state(qp, 200);
  m->adaptive = 1;
  m->coeff_cabac = qp >= 28;  // `ultrafast`: fast-residual-cost 28 (cfg.c:485-512), rdo.c:311-340
}


// ---- per-picture models (kvz_hip_picture_models) ----
// Where the parts of kvz_hip_batch::d_models are: what the kernels of a mixed launch are handed
struct ModelTableView {
  CtuModelTable ctu;             // the SAO decision: compact rows + the row of every picture
                                 // (the CTU pass reads the same two pointers behind the batch's ticket words: kvz_ctu_kernels.hpp KVZ_SCHED_TABLE_AT)
  const uint8_t *ctx_rows;       // the entropy coder: [n_models][KVZ_ENTROPY_CTX_ROW]
  const int32_t *qp_of_picture;  // deblocking: [n_frames]
};
// The table (checked by picture_models_known) on the device: copied when it differs from what the batch holds (the sources are the caller's: staged before this returns)
inline ModelTableView picture_models_stage(kvz_hip_batch *b, const kvz_hip_picture_models *pm)
{
  const size_t n = (size_t)pm->n_models, nf = (size_t)b->n_frames, ctx_bytes = KVZ_ENTROPY_CTX_ROW;  // a model's ctx_init and zeros up to what the entropy coder reads of a row
  static_assert(sizeof(((kvz_hip_intra_cost_model *)0)->ctx_init) <= KVZ_ENTROPY_CTX_ROW && KVZ_ENTROPY_CTXS <= KVZ_ENTROPY_CTX_ROW, "a row of initial states");
  const size_t at_rows = 16, at_ctx = (at_rows + n * sizeof(CtuModel) + 15) & ~(size_t)15, at_qp = at_ctx + n * ctx_bytes, at_index = at_qp + nf * sizeof(int32_t), bytes = at_index + nf * sizeof(uint16_t);
  bool fresh = false;
  if (bytes > b->d_models.bytes) {
    KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));  // a launch in flight may still read the old one
    if (b->d_models.p) KVZ_HIP_CHECK(hipFree(b->d_models.p));
    b->d_models.bytes = bytes + bytes / 8;
    KVZ_HIP_CHECK(hipMalloc(&b->d_models.p, b->d_models.bytes));
    fresh = true;
  }
  uint8_t *d = (uint8_t *)b->d_models.p;
  std::vector<uint8_t> image(bytes, 0);
  for (size_t i = 0; i < n; i++) {
    CtuModel cm;
    memset(&cm, 0, sizeof cm);  // (padding bytes take part in the comparison below)
    ctu_model_from(&pm->models[i], &cm);
    cm.entropy_fbits = b->d_entropy;
    cm.ctx_init = d + at_ctx + i * ctx_bytes;
    memcpy(image.data() + at_rows + i * sizeof(CtuModel), &cm, sizeof cm);
    memcpy(image.data() + at_ctx + i * ctx_bytes, pm->models[i].ctx_init, sizeof pm->models[i].ctx_init);
    static_assert(sizeof pm->models[i].ctx_init <= KVZ_ENTROPY_ROW_SIGNHIDE && KVZ_ENTROPY_CTXS <= KVZ_ENTROPY_ROW_SIGNHIDE, "the switch sits behind the states");
    image[at_ctx + i * ctx_bytes + KVZ_ENTROPY_ROW_SIGNHIDE] = pm->models[i].signhide != 0;  // what the entropy coder reads of the model besides its states (entropy_signhide)
    // cu_qp_delta_abs[2] (context.c: init value 154 for every slice type) at the row's QP, where an I picture has no other context: read only by the coder of
    // kvz_hip_batch_entropy_code_ctu_models, for the pictures whose slice model the row is.  kvz_hip_intra_cost_model keeps its size.
    static_assert(KVZ_EB_CX_QP_DELTA >= KVZ_HIP_CX_SAO_TYPE + 1 && KVZ_EB_CX_QP_DELTA + 2 <= (int)sizeof(((kvz_hip_intra_cost_model *)0)->ctx_init), "two bytes of a row that no I-picture syntax uses");
    image[at_ctx + i * ctx_bytes + KVZ_EB_CX_QP_DELTA] = image[at_ctx + i * ctx_bytes + KVZ_EB_CX_QP_DELTA + 1] = (uint8_t)ctx_state(pm->models[i].qp, 154);
  }
  for (size_t f = 0; f < nf; f++) {
    const int32_t qp = pm->models[pm->model_of_picture[f]].qp;
    memcpy(image.data() + at_qp + f * sizeof(int32_t), &qp, sizeof qp);
  }
  memcpy(image.data() + at_index, pm->model_of_picture, nf * sizeof(uint16_t));
  ModelTableView v;
  v.ctu.models = (const CtuModel *)(d + at_rows);
  v.ctu.model_of_picture = (const uint16_t *)(d + at_index);
  static_assert(sizeof(CtuModelTable) <= 16 && sizeof(CtuModelTable) <= (KVZ_SCHED_TICKET_WORDS - KVZ_SCHED_TABLE_AT) * sizeof(unsigned), "at_rows, d_ticket");
  memcpy(image.data(), &v.ctu, sizeof v.ctu);
  if (fresh || image != b->h_models) {
    KVZ_HIP_CHECK(hipMemcpyAsync(d, image.data(), bytes, hipMemcpyHostToDevice, b->stream));
    KVZ_HIP_CHECK(hipMemcpyAsync(b->tw.d_ticket + KVZ_SCHED_TABLE_AT, image.data(), sizeof(CtuModelTable), hipMemcpyHostToDevice, b->stream));
    KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));
    b->h_models.swap(image);
  }
  v.ctx_rows = d + at_ctx;
  v.qp_of_picture = (const int32_t *)(d + at_qp);
  return v;
}


// The price table and initial contexts of a launch's (first) model in kvz_hip_batch::d_entropy: copied when they differ from what the device holds (a small
// host-to-device copy waits behind whatever the copy engine is busy with)
inline void entropy_table_stage(kvz_hip_batch *b, const kvz_hip_intra_cost_model *model)
{
  static_assert(sizeof model->ctx_init <= 40 * sizeof(float), "last_entropy");
  float now[128 + 40] = { 0 };
  memcpy(now, model->entropy_fbits, 128 * sizeof(float));
  memcpy(now + 128, model->ctx_init, sizeof model->ctx_init);
  if (!b->entropy_valid || memcmp(now, b->last_entropy, sizeof now) != 0) {
    KVZ_HIP_CHECK(hipMemcpyAsync(b->d_entropy, model->entropy_fbits, 128 * sizeof(float), hipMemcpyHostToDevice, b->stream));
    KVZ_HIP_CHECK(hipMemcpyAsync(b->d_entropy + 128, model->ctx_init, sizeof model->ctx_init, hipMemcpyHostToDevice, b->stream));
    KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));  // the sources are the caller's: staged before this call returns
    memcpy(b->last_entropy, now, sizeof now);
    b->entropy_valid = 1;
  }
}

// The factor table of a launch on a batch that has lists: the batch's rows and every picture's two rows at the QP of its model (pm: the launch's table, or nullptr
// and `qp` for all), copied when it differs from what the device holds; the two pointers go behind the ticket words (kvz_ctu_kernels.hpp KVZ_SCHED_LISTS_AT).
inline void scaling_lists_stage(kvz_hip_batch *b, const kvz_hip_picture_models *pm, int qp)
{
  const size_t n_rows = b->list_rows.size(), nf = (size_t)b->n_frames, bytes = (n_rows + nf) * sizeof(uint32_t);
  bool fresh = false;
  if (bytes > b->d_lists.bytes) {
    KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));  // a launch in flight may still read the old one
    if (b->d_lists.p) KVZ_HIP_CHECK(hipFree(b->d_lists.p));
    b->d_lists.bytes = bytes;
    KVZ_HIP_CHECK(hipMalloc(&b->d_lists.p, b->d_lists.bytes));
    fresh = true;
  }
  std::vector<uint32_t> image(b->list_rows);
  image.resize(n_rows + nf);
  for (size_t f = 0; f < nf; f++) image[n_rows + f] = scaling_list_rows_of_picture(b->list_set_of_picture[f], b->n_list_sets, pm ? pm->models[pm->model_of_picture[f]].qp : qp);
  if (fresh || image != b->h_lists) {
    CtuListTable lt;
    lt.rows = (const uint32_t *)b->d_lists.p;
    lt.rows_of_picture = lt.rows + n_rows;
    static_assert(sizeof(CtuListTable) <= (KVZ_SCHED_TICKET_WORDS - KVZ_SCHED_LISTS_AT) * sizeof(unsigned), "d_ticket");
    KVZ_HIP_CHECK(hipMemcpyAsync(b->d_lists.p, image.data(), bytes, hipMemcpyHostToDevice, b->stream));
    KVZ_HIP_CHECK(hipMemcpyAsync(b->tw.d_ticket + KVZ_SCHED_LISTS_AT, &lt, sizeof lt, hipMemcpyHostToDevice, b->stream));
    KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));
    b->h_lists.swap(image);
  }
}

// The map of a launch with a model per CTU (checked by ctu_models_known; its table is staged by picture_models_stage) on the device: what the kernels are handed
struct CtuMapView {
  const double *lambda_of_ctu;    // the SAO decision: [n_frames][ctu]
  const uint16_t *model_of_ctu;   // the pass (the pointer also goes behind the ticket words: kvz_ctu_kernels.hpp KVZ_SCHED_CTU_MAP_AT)
  const uint8_t *qp_of_ctu;       // the CU-QP step
};
// same_as_staged (the loop filters: the CU QPs they read come from the pass): nothing is staged and *same_as_staged says whether this is the map the device holds
inline CtuMapView ctu_models_stage(kvz_hip_batch *b, const kvz_hip_ctu_models *cm, bool *same_as_staged = nullptr)
{
  const size_t nctu = (size_t)b->F.wc * b->F.hc * b->n_frames, at_map = nctu * sizeof(double), at_qp = at_map + nctu * sizeof(uint16_t), bytes = at_qp + nctu;
  if (same_as_staged && bytes > b->d_ctu_map.bytes) { *same_as_staged = false; return CtuMapView{}; }
  bool fresh = false;
  if (bytes > b->d_ctu_map.bytes) {
    KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));  // a launch in flight may still read the old one
    if (b->d_ctu_map.p) KVZ_HIP_CHECK(hipFree(b->d_ctu_map.p));
    b->d_ctu_map.bytes = bytes;
    KVZ_HIP_CHECK(hipMalloc(&b->d_ctu_map.p, b->d_ctu_map.bytes));
    fresh = true;
  }
  if (!b->d_cu_qp) {
    KVZ_HIP_CHECK(hipMalloc((void **)&b->d_cu_qp, (size_t)(b->F.W / 8) * (b->F.H / 8) * b->n_frames));
    KVZ_HIP_CHECK(hipMalloc((void **)&b->d_ctu_qp, nctu * sizeof(uint32_t)));
  }
  std::vector<uint8_t> image(bytes, 0);
  for (size_t i = 0; i < nctu; i++) {
    const kvz_hip_intra_cost_model &m = cm->pictures->models[cm->model_of_ctu[i]];
    memcpy(image.data() + i * sizeof(double), &m.lambda, sizeof(double));
    image[at_qp + i] = (uint8_t)m.qp;
  }
  memcpy(image.data() + at_map, cm->model_of_ctu, nctu * sizeof(uint16_t));
  uint8_t *d = (uint8_t *)b->d_ctu_map.p;
  CtuMapView v{ (const double *)d, (const uint16_t *)(d + at_map), d + at_qp };
  if (same_as_staged) { *same_as_staged = image == b->h_ctu_map; return v; }
  if (fresh || image != b->h_ctu_map) {
    CtuMapTable mt;
    mt.model_of_ctu = v.model_of_ctu;
    static_assert(sizeof(CtuMapTable) <= (KVZ_SCHED_TICKET_WORDS - KVZ_SCHED_CTU_MAP_AT) * sizeof(unsigned) && KVZ_SCHED_CTU_MAP_AT * sizeof(unsigned) % alignof(CtuMapTable) == 0, "d_ticket");
    KVZ_HIP_CHECK(hipMemcpyAsync(d, image.data(), bytes, hipMemcpyHostToDevice, b->stream));
    KVZ_HIP_CHECK(hipMemcpyAsync(b->tw.d_ticket + KVZ_SCHED_CTU_MAP_AT, &mt, sizeof mt, hipMemcpyHostToDevice, b->stream));
    KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));
    b->h_ctu_map.swap(image);
  }
  return v;
}
// the job of the CU-QP step of a batch whose pass ran under (cm, its staged views)
inline CuQpJob cu_qp_job(const kvz_hip_batch *b, const ModelTableView &t, const CtuMapView &v, int no_wpp)
{
  return CuQpJob{ b->F.W, b->F.H, b->F.wc, b->F.hc, b->n_frames, no_wpp, b->d_coeff, b->d_depth, v.qp_of_ctu, t.qp_of_picture, b->d_cu_qp, b->d_ctu_qp };
}

}  // namespace kvz

extern "C" {

void kvz_hip_scaling_lists_default(kvz_hip_scaling_lists *lists) { kvz::scaling_lists_default(lists); }

int kvz_hip_batch_set_scaling_lists(kvz_hip_batch *b, const kvz_hip_scaling_lists *sets, int n_sets, const uint16_t *set_of_picture)
{
  if (!b || !kvz::scaling_list_sets_known(sets, n_sets, set_of_picture, b->n_frames, b->sched_ticket != 0, "kvz_hip_batch_set_scaling_lists")) return -1;
  b->n_list_sets = n_sets;
  b->list_rows.assign(n_sets ? (size_t)(n_sets + 1) * 6 * kvz::KVZ_LIST_ROW : 0, 0);
  b->list_set_of_picture.assign(n_sets ? (size_t)b->n_frames : 0, 0);
  for (int k = 0; k < n_sets; k++) kvz::scaling_list_rows(&sets[k], b->list_rows.data() + (size_t)k * 6 * kvz::KVZ_LIST_ROW);
  if (n_sets) kvz::scaling_list_rows(nullptr, b->list_rows.data() + (size_t)n_sets * 6 * kvz::KVZ_LIST_ROW);
  if (n_sets && set_of_picture) b->list_set_of_picture.assign(set_of_picture, set_of_picture + b->n_frames);
  return 0;
}

void kvz_hip_intra_cost_model_init(int qp, uint64_t coeff_weights, kvz_hip_intra_cost_model *model) { kvz::cost_model_init(qp, coeff_weights, model); }
uint64_t kvz_hip_default_coeff_weights(int qp) { return qp >= 0 && qp < 50 ? kvz::kDefaultCoeffWeights[qp] : 0; }

kvz_hip_batch *kvz_hip_batch_create(int width, int height, int n_frames) { return kvz_hip_batch_create_on(-1, width, height, n_frames); }

kvz_hip_batch *kvz_hip_batch_create_on(int device, int width, int height, int n_frames)
{
  if (width <= 0 || height <= 0 || n_frames <= 0 || (width & 7) || (height & 7)) {
    fprintf(stderr, "kvz_hip_batch_create: width and height must be positive multiples of 8\n");
    return nullptr;
  }
  kvz::runtime_init(-1);
  if (device >= kvz::runtime().n_devices) {
    fprintf(stderr, "kvz_hip_batch_create_on: device %d of %d\n", device, kvz::runtime().n_devices);
    return nullptr;
  }
  if (device >= 0) KVZ_HIP_CHECK(hipSetDevice(device));  // (the calling thread stays on it, as after any call on the batch)
  kvz_hip_batch *b = new kvz_hip_batch();
  b->device = kvz::current_device();
  b->failed = 0;
  {
    const char *e = getenv("KVZ_HIP_WAIT_MS");  // bound of one hand-off wait (wall clock); a whole 4K picture without WPP is a 2.5 s chain
    const double ms = e && atof(e) > 0 ? atof(e) : 30000.0;
    b->wait_ticks = (unsigned long long)(ms * 1e5);
  }
  kvz::CtuFrames &F = b->F;
  F.W = width; F.H = height; F.wc = (width + 63) / 64; F.hc = (height + 63) / 64;
  F.frame_px = (long)width * height * 3 / 2;
  b->n_frames = n_frames;
  const size_t nctu = (size_t)F.wc * F.hc * n_frames, ncu = (size_t)(width / 8) * (height / 8) * n_frames;
  KVZ_HIP_CHECK(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
  KVZ_HIP_CHECK(hipEventCreate(&b->ev0));
  KVZ_HIP_CHECK(hipEventCreate(&b->ev1));
  KVZ_HIP_CHECK(hipMalloc((void **)&b->d_src, F.frame_px * n_frames));
  KVZ_HIP_CHECK(hipMalloc((void **)&b->d_rec, F.frame_px * n_frames));
  KVZ_HIP_CHECK(hipMalloc((void **)&b->d_coeff, nctu * 6144 * sizeof(int16_t)));
  KVZ_HIP_CHECK(hipMalloc((void **)&b->d_scratch, nctu * 6144 * sizeof(int16_t)));
  KVZ_HIP_CHECK(hipMalloc((void **)&b->d_depth, ncu));
  KVZ_HIP_CHECK(hipMalloc((void **)&b->d_mode, ncu));
  KVZ_HIP_CHECK(hipMalloc((void **)&b->d_cost, nctu * sizeof(double)));
  KVZ_HIP_CHECK(hipMemsetAsync(b->d_rec, 0, F.frame_px * n_frames, b->stream));  // on the batch's stream: a non-blocking stream does not order against the null stream
#ifdef KVZ_CTU_TRACE
  KVZ_HIP_CHECK(hipMalloc((void **)&b->d_prof, (size_t)nctu * sizeof(unsigned long long)));  // a word per CTU: where it is (kvz_ctu_kernels.hpp KVZ_TRACE)
  KVZ_HIP_CHECK(hipMemsetAsync(b->d_prof, 0, (size_t)nctu * sizeof(unsigned long long), b->stream));
#else
  KVZ_HIP_CHECK(hipMalloc((void **)&b->d_prof, KVZ_PROF_WORDS * sizeof(unsigned long long)));  // + 8: the sections of rdoq_block_wave
  KVZ_HIP_CHECK(hipMemsetAsync(b->d_prof, 0, KVZ_PROF_WORDS * sizeof(unsigned long long), b->stream));
#endif
  F.prof = b->d_prof;
  KVZ_HIP_CHECK(hipMalloc((void **)&b->d_entropy, 128 * sizeof(float) + sizeof(((kvz_hip_intra_cost_model *)0)->ctx_init)));
  KVZ_HIP_CHECK(hipMalloc((void **)&b->d_border, nctu * KVZ_BORDER_BYTES));
  KVZ_HIP_CHECK(hipMemsetAsync(b->d_border, 0, nctu * KVZ_BORDER_BYTES, b->stream));
  F.border = b->d_border;
  {  // ticket schedule: items in dependency order, with WPP (anti-diagonal, frame, row) and without (every CTU depends on its raster predecessor) -- the lists of a group of one
    const kvz::JointGeometry geo{ F.wc, F.hc, n_frames };
    std::vector<uint32_t> wpp, raster;
    kvz::joint_ticket_lists(&geo, 1, &wpp, &raster);
    b->total_items = (unsigned)wpp.size();
    b->epoch = 0;
    KVZ_HIP_CHECK(hipMalloc((void **)&b->d_items, wpp.size() * sizeof(uint32_t)));
    KVZ_HIP_CHECK(hipMemcpy(b->d_items, wpp.data(), wpp.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    KVZ_HIP_CHECK(hipMalloc((void **)&b->d_items_raster, raster.size() * sizeof(uint32_t)));
    KVZ_HIP_CHECK(hipMemcpy(b->d_items_raster, raster.data(), raster.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    KVZ_HIP_CHECK(hipMalloc((void **)&b->d_done, nctu * sizeof(unsigned)));
    KVZ_HIP_CHECK(hipMemsetAsync(b->d_done, 0, nctu * sizeof(unsigned), b->stream));
    b->tw.create(b->stream);
    const char *e = getenv("KVZ_HIP_SCHED");  // "wave": one launch per anti-diagonal (the simpler schedule, kept for A/B)
    b->sched_ticket = !(e && e[0] == 'w') && n_frames < 65536 && F.wc < 256 && F.hc < 256;
    int per_cu = 0, dev = 0, cus = 0;
    KVZ_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kvz::intra_ctu_ticket_kernel<true>, KVZ_CTU_THREADS, 0));
    KVZ_HIP_CHECK(hipGetDevice(&dev));
    KVZ_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (per_cu < 1) per_cu = 1;
    if (const char *lim = getenv("KVZ_HIP_WG_PER_CU")) { const int v = atoi(lim); if (v >= 1 && v < per_cu) per_cu = v; }  // occupancy experiments
    b->slots_per_cu = per_cu; b->cus = cus;
    b->grid_ticket = per_cu * cus;
    if ((unsigned)b->grid_ticket > b->total_items) b->grid_ticket = (int)b->total_items;
  }
  KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));
  F.src = b->d_src; F.rec = b->d_rec; F.coeff = b->d_coeff; F.coeff_scratch = b->d_scratch;
  F.cu_depth = b->d_depth; F.cu_mode = b->d_mode; F.ctu_cost = b->d_cost;
  return b;
}

void kvz_hip_batch_destroy(kvz_hip_batch *b)
{
  if (!b) return;
  kvz::batch_enter(b);
  (void)hipStreamSynchronize(b->stream);
  (void)hipFree(b->d_ver); (void)hipFree(b->d_dbk); (void)hipFree(b->d_sao_merge); (void)hipFree(b->d_sao_stats); (void)hipFree(b->d_sao_cand); (void)hipFree(b->d_sao_recs); (void)hipFree(b->d_sao_fbits);
  (void)hipFree(b->d_border); (void)hipFree(b->d_items); (void)hipFree(b->d_items_raster); (void)hipFree(b->d_done); b->tw.destroy(); (void)hipFree(b->d_prof); (void)hipFree(b->d_entropy);
  (void)hipFree(b->d_src); (void)hipFree(b->d_rec); (void)hipFree(b->d_coeff); (void)hipFree(b->d_scratch); (void)hipFree(b->d_depth); (void)hipFree(b->d_mode); (void)hipFree(b->d_cost); (void)hipFree(b->d_part); (void)hipFree(b->d_mode4);
  (void)hipEventDestroy(b->ev0); (void)hipEventDestroy(b->ev1);
  if (b->entropy_out.p) (void)hipFree(b->entropy_out.p);
  if (b->ev_up) { (void)hipEventSynchronize(b->ev_up); (void)hipEventDestroy(b->ev_up); }
  if (b->ev_src_read) (void)hipEventDestroy(b->ev_src_read);
  (void)hipFree(b->d_sse); (void)hipFree(b->d_models.p); (void)hipFree(b->d_lists.p);
  (void)hipFree(b->d_ctu_map.p); (void)hipFree(b->d_cu_qp); (void)hipFree(b->d_ctu_qp);
  if (b->ev_cu_qp0) { (void)hipEventDestroy(b->ev_cu_qp0); (void)hipEventDestroy(b->ev_cu_qp1); }
  (void)hipStreamDestroy(b->stream);
  delete b;
}

int kvz_hip_batch_ctus_per_frame(const kvz_hip_batch *b) { return b->F.wc * b->F.hc; }

void kvz_hip_batch_upload(kvz_hip_batch *b, int frame, const uint8_t *y, const uint8_t *u, const uint8_t *v)
{
  kvz::batch_enter(b);
  const long ys = (long)b->F.W * b->F.H, cs = ys / 4;
  uint8_t *dst = b->d_src + (long)frame * b->F.frame_px;
  KVZ_HIP_CHECK(hipMemcpyAsync(dst, y, ys, hipMemcpyHostToDevice, b->stream));
  KVZ_HIP_CHECK(hipMemcpyAsync(dst + ys, u, cs, hipMemcpyHostToDevice, b->stream));
  KVZ_HIP_CHECK(hipMemcpyAsync(dst + ys + cs, v, cs, hipMemcpyHostToDevice, b->stream));
  KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));
}

namespace kvz {
// ONE upload queue per device, shared by its batches: the runtime multiplexes streams onto four hardware queues, and a stream that lands on the queue of an upload
// stream waits for the copy in front of it (a fifth stream -- two batches, the coder's side stream, an upload stream per batch -- made the coder's kernels wait 84 ms
// for another batch's pictures: tools/chain_h2d_trace.sh)
inline hipStream_t upload_stream(int device)
{
  static std::mutex lock;
  static hipStream_t streams[64] = {};
  std::lock_guard<std::mutex> guard(lock);
  hipStream_t &st = streams[device & 63];
  if (!st) KVZ_HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  return st;
}
}  // namespace kvz

void kvz_hip_batch_upload_all_async(kvz_hip_batch *b, const uint8_t *src)
{
  kvz::batch_enter(b);
  const hipStream_t up = kvz::upload_stream(b->device);
  if (!b->ev_up) KVZ_HIP_CHECK(hipEventCreateWithFlags(&b->ev_up, hipEventDisableTiming));
  // the source pictures are only read by the CTU pass (and by SAO's statistics): the copy may start as soon as the batch's last pass has ended (ev1; a no-op
  // before the first pass), whatever its stream still holds behind it -- deblocking, the entropy coder, downloads
  KVZ_HIP_CHECK(hipStreamWaitEvent(up, b->ev1, 0));
  if (b->src_read_set) KVZ_HIP_CHECK(hipStreamWaitEvent(up, b->ev_src_read, 0));  // ... and the last distortion sum queued on them (kvz_hip_batch_sse_async)
  KVZ_HIP_CHECK(hipMemcpyAsync(b->d_src, src, (size_t)b->n_frames * b->F.frame_px, hipMemcpyHostToDevice, up));
  KVZ_HIP_CHECK(hipEventRecord(b->ev_up, up));
  b->up_pending = 1;
}

int kvz_hip_batch_download(kvz_hip_batch *b, int frame, uint8_t *rec_y, uint8_t *rec_u, uint8_t *rec_v, int16_t *coeff, uint8_t *cu_depth,
                           uint8_t *cu_mode, double *ctu_cost)
{
  kvz::batch_enter(b);
  const kvz::CtuFrames &F = b->F;
  const long ys = (long)F.W * F.H, cs = ys / 4, nctu = (long)F.wc * F.hc, ncu = (long)(F.W / 8) * (F.H / 8);
  const uint8_t *src = b->d_rec + (long)frame * F.frame_px;
  KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));
  if (rec_y) KVZ_HIP_CHECK(hipMemcpy(rec_y, src, ys, hipMemcpyDeviceToHost));
  if (rec_u) KVZ_HIP_CHECK(hipMemcpy(rec_u, src + ys, cs, hipMemcpyDeviceToHost));
  if (rec_v) KVZ_HIP_CHECK(hipMemcpy(rec_v, src + ys + cs, cs, hipMemcpyDeviceToHost));
  if (coeff) KVZ_HIP_CHECK(hipMemcpy(coeff, b->d_coeff + frame * nctu * 6144, nctu * 6144 * sizeof(int16_t), hipMemcpyDeviceToHost));
  if (cu_depth) KVZ_HIP_CHECK(hipMemcpy(cu_depth, b->d_depth + frame * ncu, ncu, hipMemcpyDeviceToHost));
  if (cu_mode) KVZ_HIP_CHECK(hipMemcpy(cu_mode, b->d_mode + frame * ncu, ncu, hipMemcpyDeviceToHost));
  if (ctu_cost) KVZ_HIP_CHECK(hipMemcpy(ctu_cost, b->d_cost + frame * nctu, nctu * sizeof(double), hipMemcpyDeviceToHost));
  return kvz::batch_check(b);
}

int kvz_hip_batch_download_partitions(kvz_hip_batch *b, int frame, uint8_t *cu_part, uint8_t *cu_mode4)
{
  kvz::batch_enter(b);
  const kvz::CtuFrames &F = b->F;
  const long ncu = (long)(F.W / 8) * (F.H / 8), n4 = (long)(F.W / 4) * (F.H / 4);
  KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));
  if (!b->d_part) { fprintf(stderr, "kvz_hip_batch_download_partitions: no pass with model.search_nxn has run on this batch\n"); return -1; }
  if (cu_part) KVZ_HIP_CHECK(hipMemcpy(cu_part, b->d_part + frame * ncu, ncu, hipMemcpyDeviceToHost));
  if (cu_mode4) KVZ_HIP_CHECK(hipMemcpy(cu_mode4, b->d_mode4 + frame * n4, n4, hipMemcpyDeviceToHost));
  return kvz::batch_check(b);
}

void *kvz_hip_host_alloc(size_t bytes)
{
  kvz::runtime_init(-1);
  void *p = nullptr;
  KVZ_HIP_CHECK(hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault));
  return p;
}
void kvz_hip_host_free(void *p) { if (p) KVZ_HIP_CHECK(hipHostFree(p)); }

void kvz_hip_batch_download_all_async(kvz_hip_batch *b, uint8_t *rec, int16_t *coeff, uint8_t *cu_depth, uint8_t *cu_mode)
{
  kvz::batch_enter(b);
  const kvz::CtuFrames &F = b->F;
  const size_t n = (size_t)b->n_frames, nctu = (size_t)F.wc * F.hc * n, ncu = (size_t)(F.W / 8) * (F.H / 8) * n;
  if (rec) KVZ_HIP_CHECK(hipMemcpyAsync(rec, b->d_rec, (size_t)F.frame_px * n, hipMemcpyDeviceToHost, b->stream));
  if (coeff) KVZ_HIP_CHECK(hipMemcpyAsync(coeff, b->d_coeff, nctu * 6144 * sizeof(int16_t), hipMemcpyDeviceToHost, b->stream));
  if (cu_depth) KVZ_HIP_CHECK(hipMemcpyAsync(cu_depth, b->d_depth, ncu, hipMemcpyDeviceToHost, b->stream));
  if (cu_mode) KVZ_HIP_CHECK(hipMemcpyAsync(cu_mode, b->d_mode, ncu, hipMemcpyDeviceToHost, b->stream));
}

void kvz_hip_batch_set_device_share(kvz_hip_batch *b, int num, int den)
{
  if (!b || !b->sched_ticket || num < 1 || den < num) return;
  int per_cu = b->slots_per_cu * num / den;
  if (per_cu < 1) per_cu = 1;
  b->grid_ticket = per_cu * b->cus;
  if ((unsigned)b->grid_ticket > b->total_items) b->grid_ticket = (int)b->total_items;
}

void kvz_hip_batch_order_after(kvz_hip_batch *b, kvz_hip_batch *other)
{
  kvz::batch_enter(b);
  hipEvent_t ev;
  KVZ_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  KVZ_HIP_CHECK(hipEventRecord(ev, other->stream));
  KVZ_HIP_CHECK(hipStreamWaitEvent(b->stream, ev, 0));
  KVZ_HIP_CHECK(hipEventDestroy(ev));  // released once the wait has been satisfied
}

// The pass of kvz_hip_intra_frames (!table: `model` for every picture) and of kvz_hip_intra_frames_models (table: picture_models_stage has put it on the device; `model` = its first: the switches and
// the price table every model shares; any_cabac: some model prices coefficients with the CABAC model -- that instantiation then prices the others' through its run-time switch;
// any_signhide: some model hides sign bits -- the launch takes a sign-hiding instantiation, which reads the switch of the drawn picture's model; pm: the table, or nullptr).
// A batch that has scaling lists takes the instantiations that quantise under a factor per position (the entry points have refused rdoq, search_nxn and signhide).
// ctu_map: the pass of kvz_hip_intra_frames_ctu_models (ctu_models_stage has put the map on the device) -- a build of kvz_ctu_qp_builds.hpp, which fetches the drawn CTU's row.
static int kvz_intra_frames_queue(kvz_hip_batch *b, const kvz_hip_intra_cost_model *model, const kvz_hip_picture_models *pm, bool any_cabac, bool any_signhide, bool ctu_map = false)
{
  const bool table = pm != nullptr, lists = b->n_list_sets > 0;
  const int build = ctu_map ? kvz::ctu_qp_build_choose(model->search_32x32 != 0, any_cabac)
                            : kvz::ctu_build_choose({ model->search_32x32 != 0, model->rdoq != 0, model->search_nxn != 0, any_cabac, any_signhide, lists, false });  // (of the ticket schedule)
  if (b->sched_ticket && build == kvz::KVZ_CTU_BUILD_NONE) { fprintf(stderr, "kvz_hip_intra_frames: no kernel build for this launch\n"); return -1; }  // (before anything is staged; the entry points refuse these with the reason)
  kvz::batch_enter(b);
  const kvz::CtuFrames &F = b->F;
  int launches = 0;
  kvz::CtuModel cm;
  kvz::ctu_model_from(model, &cm);
  cm.coeff_cabac = any_cabac;
  cm.entropy_fbits = b->d_entropy;
  cm.ctx_init = (const uint8_t *)(b->d_entropy + 128);
  if (b->up_pending) { KVZ_HIP_CHECK(hipStreamWaitEvent(b->stream, b->ev_up, 0)); b->up_pending = 0; }  // pictures on their way (kvz_hip_batch_upload_all_async)
  kvz::entropy_table_stage(b, model);
  // argument errors are reported, not fatal (a HIP failure still aborts: there is no error channel for it and no CPU path to fall back to)
  if (!b->sched_ticket && (cm.search_32x32 || cm.rdoq || cm.search_nxn)) { fprintf(stderr, "kvz_hip_intra_frames: search_32x32 / rdoq / search_nxn need the ticket schedule\n"); return -1; }
  if (!b->sched_ticket && cm.no_wpp) { fprintf(stderr, "kvz_hip_intra_frames: the one-launch-per-diagonal schedule (KVZ_HIP_SCHED=wave) needs WPP\n"); return -1; }
  if (cm.rdoq && !cm.coeff_cabac) { fprintf(stderr, "kvz_hip_intra_frames: rdoq needs coeff_cabac (kvazaar's presets with --rdoq have --fast-residual-cost 0)\n"); return -1; }
  if (lists) kvz::scaling_lists_stage(b, pm, model->qp);  // (a batch under the other schedule has none)
  if (b->sched_ticket) {
    b->epoch++;
    kvz::CtuSched sc{ cm.no_wpp ? b->d_items_raster : b->d_items, b->tw.d_ticket, b->d_done, b->tw.d_error, b->total_items, b->epoch, cm.no_wpp | (table ? kvz::KVZ_SCHED_MODEL_TABLE : 0), b->wait_ticks };
    b->tw.pass(b->stream, b->ev0, b->ev1, [&] {
      if (ctu_map) {
        kvz::ctu_qp_build_dispatch(build, [&](auto bt) {
          hipLaunchKernelGGL((kvz::intra_ctu_ticket_kernel_ctuqp<decltype(bt)::cabac != 0, decltype(bt)::s32 != 0>), dim3(b->grid_ticket), dim3(KVZ_CTU_THREADS), 0, b->stream, F, cm, kvz::device_tables(), sc);
        });
        return;
      }
      kvz::ctu_build_dispatch(build, [&](auto bt) {
        kvz::CtuFrames Fr = F;
        if constexpr (bt.rdoq) {  // the build that writes NxN flags and 4x4 modes
          if (cm.search_nxn && !b->d_part) {
            KVZ_HIP_CHECK(hipMalloc((void **)&b->d_part, (size_t)(F.W / 8) * (F.H / 8) * b->n_frames));
            KVZ_HIP_CHECK(hipMalloc((void **)&b->d_mode4, (size_t)(F.W / 4) * (F.H / 4) * b->n_frames));
          }
          Fr.cu_part = b->d_part; Fr.cu_mode4 = b->d_mode4;
        }
        if constexpr (!bt.joint) hipLaunchKernelGGL(kvz::ctu_build_kernel(bt), dim3(b->grid_ticket), dim3(KVZ_CTU_THREADS), 0, b->stream, Fr, cm, kvz::device_tables(), sc);
      });
    });
    return 1;
  }
  KVZ_HIP_CHECK(hipEventRecord(b->ev0, b->stream));
  // CTU (x, y) needs (x-1, y), (x, y-1), (x+1, y-1): all of them lie on earlier anti-diagonals x + 2y (the WPP order of
  // encoderstate.c:793-903), so one launch per diagonal needs no synchronisation inside the launch.
  for (int wave = 0; wave <= (F.wc - 1) + 2 * (F.hc - 1); wave++) {
    int y_min = (wave - (F.wc - 1) + 1) / 2;
    if (y_min < 0) y_min = 0;
    int y_max = wave / 2;
    if (y_max > F.hc - 1) y_max = F.hc - 1;
    const int n_diag = y_max - y_min + 1;
    if (n_diag <= 0) continue;
    if (cm.coeff_cabac) hipLaunchKernelGGL(kvz::intra_ctu_wave_kernel<true>, dim3(n_diag * b->n_frames), dim3(KVZ_CTU_THREADS), 0, b->stream, F, cm, kvz::device_tables(), wave,
                                           y_min, n_diag);
    else hipLaunchKernelGGL(kvz::intra_ctu_wave_kernel<false>, dim3(n_diag * b->n_frames), dim3(KVZ_CTU_THREADS), 0, b->stream, F, cm, kvz::device_tables(), wave,
                            y_min, n_diag);
    launches++;
  }
  KVZ_HIP_CHECK(hipGetLastError());
  KVZ_HIP_CHECK(hipEventRecord(b->ev1, b->stream));
  return launches;
}

int kvz_hip_intra_frames(kvz_hip_batch *b, const kvz_hip_intra_cost_model *model)
{
  if (!b || !kvz::cost_model_known(model, "kvz_hip_intra_frames")) return -1;
  if (!kvz::signhide_known(model, b->sched_ticket != 0, "kvz_hip_intra_frames")) return -1;
  if (!kvz::scaling_lists_known(model, b->n_list_sets > 0, "kvz_hip_intra_frames")) return -1;
  return kvz_intra_frames_queue(b, model, nullptr, model->coeff_cabac != 0, model->signhide != 0);
}

int kvz_hip_intra_frames_models(kvz_hip_batch *b, const kvz_hip_picture_models *pm)
{
  if (!b || !kvz::picture_models_known(pm, b->n_frames, b->sched_ticket != 0, "kvz_hip_intra_frames_models")) return -1;
  if (!kvz::scaling_lists_known(pm, b->n_list_sets > 0, "kvz_hip_intra_frames_models")) return -1;
  kvz::batch_enter(b);
  kvz::picture_models_stage(b, pm);
  return kvz_intra_frames_queue(b, &pm->models[0], pm, kvz::picture_models_any_cabac(pm), kvz::picture_models_any_signhide(pm));
}

int kvz_hip_intra_frames_ctu_models(kvz_hip_batch *b, const kvz_hip_ctu_models *cm)
{
  if (!b || !kvz::ctu_models_known(cm, b->n_frames, b->F.wc * b->F.hc, b->sched_ticket != 0, b->n_list_sets > 0, "kvz_hip_intra_frames_ctu_models")) return -1;
  kvz::batch_enter(b);
  const kvz_hip_picture_models *pm = cm->pictures;
  const kvz::ModelTableView table = kvz::picture_models_stage(b, pm);
  const kvz::CtuMapView map = kvz::ctu_models_stage(b, cm);
  const int rc = kvz_intra_frames_queue(b, &pm->models[0], pm, kvz::picture_models_any_cabac(pm), false, true);
  if (rc < 0) return rc;
  if (!b->ev_cu_qp0) { KVZ_HIP_CHECK(hipEventCreate(&b->ev_cu_qp0)); KVZ_HIP_CHECK(hipEventCreate(&b->ev_cu_qp1)); }
  KVZ_HIP_CHECK(hipEventRecord(b->ev_cu_qp0, b->stream));
  kvz::cu_qp_frames_on(b->stream, kvz::cu_qp_job(b, table, map, pm->models[0].no_wpp != 0));  // behind the pass: the QP of every CU, for the loop filters
  KVZ_HIP_CHECK(hipGetLastError());
  KVZ_HIP_CHECK(hipEventRecord(b->ev_cu_qp1, b->stream));
  b->cu_qp_epoch = b->epoch;
  return rc;
}

float kvz_hip_batch_last_cu_qp_ms(kvz_hip_batch *b)
{
  float ms = 0;
  kvz::batch_enter(b);
  if (!b->ev_cu_qp0) return 0;
  KVZ_HIP_CHECK(hipEventSynchronize(b->ev_cu_qp1));
  KVZ_HIP_CHECK(hipEventElapsedTime(&ms, b->ev_cu_qp0, b->ev_cu_qp1));
  return ms;
}

int kvz_hip_batch_download_cu_qps(kvz_hip_batch *b, int frame, uint8_t *cu_qp, uint32_t *ctu_qp)
{
  if (!b || frame < 0 || frame >= b->n_frames) { fprintf(stderr, "kvz_hip_batch_download_cu_qps: bad argument\n"); return -1; }
  kvz::batch_enter(b);
  KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));
  if (!b->cu_qp_epoch || b->cu_qp_epoch != b->epoch) { fprintf(stderr, "kvz_hip_batch_download_cu_qps: the batch's last pass was no kvz_hip_intra_frames_ctu_models\n"); return -1; }
  const size_t ncu = (size_t)(b->F.W / 8) * (b->F.H / 8), nctu = (size_t)b->F.wc * b->F.hc;
  if (cu_qp) KVZ_HIP_CHECK(hipMemcpy(cu_qp, b->d_cu_qp + frame * ncu, ncu, hipMemcpyDeviceToHost));
  if (ctu_qp) KVZ_HIP_CHECK(hipMemcpy(ctu_qp, b->d_ctu_qp + frame * nctu, nctu * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return kvz::batch_check(b);
}

int kvz_hip_batch_sync(kvz_hip_batch *b)
{
  kvz::batch_enter(b);
  KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));
  return kvz::batch_check(b);
}

/* developer diagnostics (tools/chain_stress.py): the hand-off flags of every CTU as they stand in memory -- a CTU's flag holds the number of the last pass that completed
 * it -- into out [n_frames x ctus_per_frame]; returns the number of the batch's last pass */
#ifdef KVZ_CTU_TRACE
extern "C" void kvz_hip_batch_debug_trace(kvz_hip_batch *b, unsigned long long *out)
{
  kvz::batch_enter(b);
  KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));
  KVZ_HIP_CHECK(hipMemcpy(out, b->d_prof, (size_t)b->n_frames * b->F.wc * b->F.hc * sizeof(unsigned long long), hipMemcpyDeviceToHost));
}
#endif
unsigned kvz_hip_batch_debug_flags(kvz_hip_batch *b, unsigned *out)
{
  kvz::batch_enter(b);
  KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));
  KVZ_HIP_CHECK(hipMemcpy(out, b->d_done, (size_t)b->n_frames * b->F.wc * b->F.hc * sizeof(unsigned), hipMemcpyDeviceToHost));
  return b->epoch;
}

int kvz_hip_batch_reset(kvz_hip_batch *b)
{
  kvz::batch_enter(b);
  KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));
  b->tw.clear_error();
  b->failed = 0;
  b->joint = nullptr;  // (the group clears its own word at its next launch, once every batch it marked has been reset)
  return 0;
}

/* cycle counters of a -DKVZ_CTU_PROFILE build (all zero otherwise); reading resets them */
int kvz_hip_batch_profile(kvz_hip_batch *b, unsigned long long *out, int n)
{
  kvz::batch_enter(b);
  KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));
  if (n > KVZ_PROF_WORDS) n = KVZ_PROF_WORDS;  // cycles per category, marks per category, rdoq_block_wave's sections and sizes, the same two tables inside eval_pu (kvz_ctu.hpp KVZ_PROF_PU_AT)
  KVZ_HIP_CHECK(hipMemcpy(out, b->d_prof, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  KVZ_HIP_CHECK(hipMemsetAsync(b->d_prof, 0, KVZ_PROF_WORDS * sizeof(unsigned long long), b->stream));
  KVZ_HIP_CHECK(hipStreamSynchronize(b->stream));
  return kvz::KVZ_P_COUNT;
}

float kvz_hip_batch_last_kernel_ms(kvz_hip_batch *b)
{
  float ms = 0;
  kvz::batch_enter(b);
  KVZ_HIP_CHECK(hipEventSynchronize(b->ev1));
  KVZ_HIP_CHECK(hipEventElapsedTime(&ms, b->ev0, b->ev1));
  return ms;
}
}

// ---- kvz_hip_batch_group: the CTU passes of several batches as ONE persistent launch (kvz_joint.hpp) ----
struct kvz_hip_batch_group {
  std::vector<kvz_hip_batch *> batches;
  std::vector<uint32_t> batch_of_picture;
  hipStream_t stream;              // the joint launch's own: it starts behind every batch's stream and every batch's stream continues behind it
  hipEvent_t ev0, ev1, ev_done;    // around the kernel; behind the copy of the error words
  hipEvent_t ev_staged[2];         // behind the copy out of records[k]
  uint32_t *d_items, *d_items_raster, *d_pictures;
  kvz::JointBatch *d_records;      // [batches], rewritten in front of every launch (the pass numbers, the model tables)
  kvz::JointBatch *h_records[2];   // pinned; launch k is staged from [k & 1]
  kvz::TicketWords tw;             // as a batch's; the JointTable at KVZ_SCHED_TABLE_AT
  unsigned total_items, launches = 0;
  int grid, reported = 0;
  unsigned long long wait_ticks;
};

namespace kvz {
inline std::vector<JointBatchInfo> joint_infos(kvz_hip_batch *const *batches, int n)
{
  std::vector<JointBatchInfo> info;
  for (int i = 0; batches && i < n; i++) {
    const kvz_hip_batch *b = batches[i];
    info.push_back(b ? JointBatchInfo{ b, b->device, b->sched_ticket, b->n_frames, b->n_list_sets > 0, b->failed } : JointBatchInfo{ nullptr, 0, 0, 0, 0, 0 });
  }
  return info;
}
// the error words of the last joint pass, as copied behind it: set -> every batch still attached to the group is invalid until reset
int joint_check(kvz_hip_batch *b)
{
  kvz_hip_batch_group *g = b->joint;
  const unsigned err[3] = { g->tw.error(0), g->tw.error(1), g->tw.error(2) };
  std::vector<int> failed(g->batches.size(), 0);
  char msg[640];
  if (joint_error_fan_out(err, g->batch_of_picture.data(), (unsigned)g->batch_of_picture.size(), (int)g->batches.size(), failed.data(), msg, sizeof msg) == -2) return 0;
  for (size_t i = 0; i < g->batches.size(); i++) if (g->batches[i]->joint == g && failed[i]) g->batches[i]->failed = 1;
  if (!g->reported) { fprintf(stderr, "kvz_hip: %s\n", msg); g->reported = 1; }
  return -1;
}
}  // namespace kvz

extern "C" {

kvz_hip_batch_group *kvz_hip_batch_group_create(kvz_hip_batch *const *batches, int n)
{
  const std::vector<kvz::JointBatchInfo> info = kvz::joint_infos(batches, n);
  if (!kvz::joint_group_known(batches ? info.data() : nullptr, n, "kvz_hip_batch_group_create")) return nullptr;
  kvz::batch_enter(batches[0]);
  kvz_hip_batch_group *g = new kvz_hip_batch_group();
  g->batches.assign(batches, batches + n);
  std::vector<kvz::JointGeometry> geo;
  for (int i = 0; i < n; i++) geo.push_back({ batches[i]->F.wc, batches[i]->F.hc, batches[i]->n_frames });
  g->batch_of_picture = kvz::joint_pictures(geo.data(), n);
  std::vector<uint32_t> wpp, raster;
  kvz::joint_ticket_lists(geo.data(), n, &wpp, &raster);
  g->total_items = (unsigned)wpp.size();
  g->wait_ticks = batches[0]->wait_ticks;
  g->grid = batches[0]->slots_per_cu * batches[0]->cus;  // the device's whole occupancy (KVZ_HIP_WG_PER_CU as the batch read it); a batch's set_device_share is not consulted
  if ((unsigned)g->grid > g->total_items) g->grid = (int)g->total_items;
  KVZ_HIP_CHECK(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
  KVZ_HIP_CHECK(hipEventCreate(&g->ev0));
  KVZ_HIP_CHECK(hipEventCreate(&g->ev1));
  KVZ_HIP_CHECK(hipEventCreateWithFlags(&g->ev_done, hipEventDisableTiming));
  for (int k = 0; k < 2; k++) {
    KVZ_HIP_CHECK(hipEventCreateWithFlags(&g->ev_staged[k], hipEventDisableTiming));
    KVZ_HIP_CHECK(hipHostMalloc((void **)&g->h_records[k], (size_t)n * sizeof(kvz::JointBatch), hipHostMallocDefault));
  }
  KVZ_HIP_CHECK(hipMalloc((void **)&g->d_items, wpp.size() * sizeof(uint32_t)));
  KVZ_HIP_CHECK(hipMalloc((void **)&g->d_items_raster, raster.size() * sizeof(uint32_t)));
  KVZ_HIP_CHECK(hipMalloc((void **)&g->d_pictures, g->batch_of_picture.size() * sizeof(uint32_t)));
  KVZ_HIP_CHECK(hipMalloc((void **)&g->d_records, (size_t)n * sizeof(kvz::JointBatch)));
  g->tw.create(g->stream);
  KVZ_HIP_CHECK(hipMemcpy(g->d_items, wpp.data(), wpp.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  KVZ_HIP_CHECK(hipMemcpy(g->d_items_raster, raster.data(), raster.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  KVZ_HIP_CHECK(hipMemcpy(g->d_pictures, g->batch_of_picture.data(), g->batch_of_picture.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  kvz::JointTable jt;
  jt.batch_of_picture = g->d_pictures; jt.batches = g->d_records;
  static_assert(sizeof(kvz::JointTable) <= (kvz::KVZ_SCHED_LISTS_AT - kvz::KVZ_SCHED_TABLE_AT) * sizeof(unsigned), "d_ticket");
  KVZ_HIP_CHECK(hipMemcpy(g->tw.d_ticket + kvz::KVZ_SCHED_TABLE_AT, &jt, sizeof jt, hipMemcpyHostToDevice));
  return g;
}

void kvz_hip_batch_group_destroy(kvz_hip_batch_group *g)
{
  if (!g) return;
  kvz::batch_enter(g->batches[0]);
  (void)hipStreamSynchronize(g->stream);
  for (kvz_hip_batch *b : g->batches)
    if (b->joint == g) { (void)hipStreamSynchronize(b->stream); if (!b->failed) kvz::joint_check(b); b->joint = nullptr; }  // what the last joint pass left stays with the batches
  (void)hipFree(g->d_items); (void)hipFree(g->d_items_raster); (void)hipFree(g->d_pictures); (void)hipFree(g->d_records); g->tw.destroy();
  for (int k = 0; k < 2; k++) { (void)hipHostFree(g->h_records[k]); (void)hipEventDestroy(g->ev_staged[k]); }
  (void)hipEventDestroy(g->ev0); (void)hipEventDestroy(g->ev1); (void)hipEventDestroy(g->ev_done);
  (void)hipStreamDestroy(g->stream);
  delete g;
}

int kvz_hip_batch_group_intra_frames(kvz_hip_batch_group *g, const kvz_hip_picture_models *const *models)
{
  if (!g) return -1;
  const int n = (int)g->batches.size();
  for (kvz_hip_batch *b : g->batches) (void)kvz::batch_check(b);  // a joint pass that failed since marks its batches now
  const std::vector<kvz::JointBatchInfo> info = kvz::joint_infos(g->batches.data(), n);
  if (!kvz::joint_launch_known(info.data(), n, models, "kvz_hip_batch_group_intra_frames")) return -1;
  const kvz_hip_intra_cost_model &m0 = models[0]->models[0];
  const int build = kvz::picture_models_build(models, n, false, true);  // (joint_launch_known: no batch has lists)
  if (build == kvz::KVZ_CTU_BUILD_NONE) { fprintf(stderr, "kvz_hip_batch_group_intra_frames: no kernel build for this launch\n"); return -1; }  // (joint_launch_known has refused these, with the reason)
  kvz::batch_enter(g->batches[0]);
  if (g->tw.error()) {  // every batch the word marked has been reset since: the group starts over
    KVZ_HIP_CHECK(hipStreamSynchronize(g->stream));
    g->tw.clear_error();
    g->reported = 0;
  }
  const int slot = (int)(g->launches & 1u);
  if (g->launches >= 2) KVZ_HIP_CHECK(hipEventSynchronize(g->ev_staged[slot]));  // the launch before the last has copied out of it
  for (int i = 0; i < n; i++) {
    kvz_hip_batch *b = g->batches[i];
    const kvz::ModelTableView view = kvz::picture_models_stage(b, models[i]);
    kvz::entropy_table_stage(b, &models[i]->models[0]);
    if (b->up_pending) { KVZ_HIP_CHECK(hipStreamWaitEvent(b->stream, b->ev_up, 0)); b->up_pending = 0; }  // pictures on their way (kvz_hip_batch_upload_all_async)
    b->epoch++;  // the joint pass is this batch's next pass: its flags are compared with its own count
    kvz::JointBatch &r = g->h_records[slot][i];
    memset(&r, 0, sizeof r);
    r.F = b->F; r.models = view.ctu; r.done = b->d_done; r.epoch = b->epoch; r.index = i;
    KVZ_HIP_CHECK(hipEventRecord(b->ev0, b->stream));  // the joint launch starts after whatever the batch's stream held
    KVZ_HIP_CHECK(hipStreamWaitEvent(g->stream, b->ev0, 0));
  }
  KVZ_HIP_CHECK(hipMemcpyAsync(g->d_records, g->h_records[slot], (size_t)n * sizeof(kvz::JointBatch), hipMemcpyHostToDevice, g->stream));
  KVZ_HIP_CHECK(hipEventRecord(g->ev_staged[slot], g->stream));
  const kvz::CtuSched sc{ m0.no_wpp ? g->d_items_raster : g->d_items, g->tw.d_ticket, nullptr, g->tw.d_error, g->total_items, 0u, (m0.no_wpp ? 1 : 0) | kvz::KVZ_SCHED_MODEL_TABLE, g->wait_ticks };
  g->tw.pass(g->stream, g->ev0, g->ev1, [&] {  // (what the copy behind it leaves, joint_check reads once a batch's stream has drained)
    kvz::ctu_build_dispatch(build, [&](auto bt) {
      if constexpr (bt.joint) hipLaunchKernelGGL(kvz::ctu_build_kernel(bt), dim3(g->grid), dim3(KVZ_CTU_THREADS), 0, g->stream, kvz::device_tables(), sc);
    });
  });
  KVZ_HIP_CHECK(hipEventRecord(g->ev_done, g->stream));
  for (kvz_hip_batch *b : g->batches) {  // everything queued on a batch from now on starts after the joint pass; ev1 is what the batch's next upload waits for
    KVZ_HIP_CHECK(hipStreamWaitEvent(b->stream, g->ev_done, 0));
    KVZ_HIP_CHECK(hipEventRecord(b->ev1, b->stream));
    b->joint = g;
  }
  g->launches++;
  return 1;
}

float kvz_hip_batch_group_last_kernel_ms(kvz_hip_batch_group *g)
{
  float ms = 0;
  kvz::batch_enter(g->batches[0]);
  KVZ_HIP_CHECK(hipEventSynchronize(g->ev1));
  KVZ_HIP_CHECK(hipEventElapsedTime(&ms, g->ev0, g->ev1));
  return ms;
}
}
