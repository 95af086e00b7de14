// kvz_cu_qp.hpp -- a cost model per CTU (kvz_hip_ctu_models, HEVC's cu_qp_delta with one quantisation group per CTU): which maps the library accepts, and the
// QP every CU ends up with after the pass (encoderstate.c:574-633 set_cu_qps with max_qp_delta_depth 0).  The rule, once:
//   a substream's predictor `last` starts at the slice QP (encoderstate.c:784: at the start of every CTU row under WPP, once per picture without);
//   for each CTU of the substream, pred = last (kvz_get_cu_ref_qp of a quantisation group at the CTU's corner: both neighbours lie outside, so it is last_qp);
//   CUs in coding order before the first CU with any coded block flag take QP pred, that CU and all after it the CTU's QP Q;
//   afterwards last = Q if the CTU has a coefficient anywhere, else pred.
// Three steps on the device, none of them on the host: a wavefront per CTU reads which 8x8 units carry a level (the coded block flags, read off the levels like the
// coder reads them) and finds the first CU with one; one lane per substream runs the chain over the CTUs' words; a lane per 8x8 unit writes the plane of CU QPs the
// loop filters read.  The checks and the per-unit functions have no HIP dependency: the host simulation (tests/hostsim/hostsim_ctu_qp.cpp) compiles the same text.
#pragma once
#include <stdio.h>

#include "../../include/kvz_hip_types.h"
#include "kvz_ctu_qp_builds.hpp"
#include "kvz_ops.hpp"
#include "kvz_picture_models.hpp"

namespace kvz {

// Is this a map a batch of n_frames pictures of `ctus` CTUs can run (ticket_schedule: not under KVZ_HIP_SCHED=wave; lists: the batch has scaling lists)?  Everything an
// entry point refuses is refused here, before anything is queued.
inline bool ctu_models_known(const kvz_hip_ctu_models *cm, int n_frames, int ctus, bool ticket_schedule, bool lists, const char *who)
{
  if (!cm || cm->struct_size != sizeof(kvz_hip_ctu_models)) {
    fprintf(stderr, "%s: kvz_hip_ctu_models.struct_size %u is not this library's %zu\n", who, cm ? cm->struct_size : 0u, sizeof(kvz_hip_ctu_models));
    return false;
  }
  if (!cm->pictures || !cm->model_of_ctu) { fprintf(stderr, "%s: kvz_hip_ctu_models needs a table (pictures) and a model index per CTU (model_of_ctu)\n", who); return false; }
  const kvz_hip_picture_models *pm = cm->pictures;
  if (!picture_models_known(pm, n_frames, ticket_schedule, who)) return false;
  for (int i = 0; i < pm->n_models; i++)
    if (pm->models[i].rdoq || pm->models[i].search_nxn || pm->models[i].signhide) {
      fprintf(stderr, "%s: model %d has rdoq / search_nxn / signhide: a model per CTU is not supported with them\n", who, i);
      return false;
    }
  if (lists) { fprintf(stderr, "%s: the batch has scaling lists: a model per CTU is not supported with them\n", who); return false; }
  for (int f = 0; f < n_frames; f++) {
    const int slice_qp = pm->models[pm->model_of_picture[f]].qp;
    int lo = slice_qp, hi = slice_qp;
    for (int c = 0; c < ctus; c++) {
      const unsigned row = cm->model_of_ctu[(long)f * ctus + c];
      if (row >= (unsigned)pm->n_models) { fprintf(stderr, "%s: model_of_ctu[%d][%d] = %u of %d models\n", who, f, c, row, pm->n_models); return false; }
      const int qp = pm->models[row].qp;
      lo = qp < lo ? qp : lo; hi = qp > hi ? qp : hi;
    }
    if (lo < 0 || hi > 51) { fprintf(stderr, "%s: picture %d has a QP outside 0 .. 51 (%d .. %d)\n", who, f, lo, hi); return false; }
    // which CTU predicts which depends on results: only the pairwise bound keeps every possible cu_qp_delta inside -26 .. 25 (encode_coding_tree.c:286)
    if (hi - lo > 25) { fprintf(stderr, "%s: the QPs of picture %d (slice QP %d, CTU QPs %d .. %d) span more than 25: a cu_qp_delta might not be codable\n", who, f, slice_qp, lo, hi); return false; }
  }
  return true;
}
// the build that serves a launch of this (checked) map, as ctu_qp_build_choose picks it
inline int ctu_models_build(const kvz_hip_ctu_models *cm) { return ctu_qp_build_choose(cm->pictures->models[0].search_32x32 != 0, picture_models_any_cabac(cm->pictures)); }

// ---- the QP of every CU
// A CTU's word: pred | Q << 8 | coded << 16 | first << 24 (kvz_hip_batch_download_cu_qps)
#define KVZ_CU_QP_WORD(pred, q, coded, first) ((uint32_t)(pred) | (uint32_t)(q) << 8 | (uint32_t)(coded) << 16 | (uint32_t)(first) << 24)
struct CuQpJob {
  int W, H, wc, hc, n_frames, no_wpp;
  const int16_t *coeff;          // [frames][ctu][6144]: the levels the pass left
  const uint8_t *cu_depth;       // [frames][(H/8)*(W/8)]
  const uint8_t *qp_of_ctu;      // [frames][ctu]: Q
  const int32_t *qp_of_picture;  // [frames]: the slice QP
  uint8_t *cu_qp;                // [frames][(H/8)*(W/8)]
  uint32_t *ctu_qp;              // [frames][ctu]
};
// 8x8 unit i of a CTU in coding (z-) order: where it lies, in units
KVZ_HD int cu_qp_unit_x(int i) { return (i & 1) | ((i >> 1) & 2) | ((i >> 2) & 4); }
KVZ_HD int cu_qp_unit_y(int i) { return ((i >> 1) & 1) | ((i >> 2) & 2) | ((i >> 3) & 4); }
KVZ_HD int cu_qp_unit_index(int x8, int y8) { return (x8 & 1) | (y8 & 1) << 1 | (x8 & 2) << 1 | (y8 & 2) << 2 | (x8 & 4) << 2 | (y8 & 4) << 3; }
KVZ_HD const uint8_t *cu_qp_depth_at(const CuQpJob &J, long frame, int x8, int y8) { return J.cu_depth + frame * (long)(J.W >> 3) * (J.H >> 3) + (long)y8 * (J.W >> 3) + x8; }
// does unit i of the CTU whose levels start at `ctu` carry a level in any plane?  (The levels of a CU lie in z-order: 64 of luma and 16 of each chroma plane per unit)
KVZ_HD bool cu_qp_unit_coded(const int16_t *ctu, int i)
{
  const unsigned long long *y = (const unsigned long long *)(ctu + i * 64), *u = (const unsigned long long *)(ctu + 4096 + i * 16), *v = (const unsigned long long *)(ctu + 5120 + i * 16);
  unsigned long long any = 0;
  for (int k = 0; k < 16; k++) any |= y[k];
  for (int k = 0; k < 4; k++) any |= u[k] | v[k];
  return any != 0;
}
// is unit i of CTU (cx, cy) inside the picture, and does it carry a level?
KVZ_HD bool cu_qp_unit_bit(const CuQpJob &J, long frame, int cx, int cy, int i)
{
  const int x8 = cx * 8 + cu_qp_unit_x(i), y8 = cy * 8 + cu_qp_unit_y(i);
  if (x8 >= (J.W >> 3) || y8 >= (J.H >> 3)) return false;
  return cu_qp_unit_coded(J.coeff + (frame * J.wc * J.hc + (long)cy * J.wc + cx) * 6144, i);
}
// the first unit of the CU that unit i of CTU (cx, cy) belongs to: a CU of depth d covers 4^(3 - d) units that follow each other
KVZ_HD int cu_qp_cu_start(const CuQpJob &J, long frame, int cx, int cy, int i)
{
  const int d = *cu_qp_depth_at(J, frame, cx * 8 + cu_qp_unit_x(i), cy * 8 + cu_qp_unit_y(i));
  return i & ~((1 << (2 * (3 - (d > 3 ? 3 : d)))) - 1);
}
// step 1, a CTU's word from its units' bits: Q, whether a delta is coded and where the first CU with a coded block flag starts (pred is the chain's)
KVZ_HD uint32_t cu_qp_ctu_word(const CuQpJob &J, long frame, int cx, int cy, unsigned long long unit_bits)
{
  const int q = J.qp_of_ctu[frame * J.wc * J.hc + (long)cy * J.wc + cx];
  if (!unit_bits) return KVZ_CU_QP_WORD(0, q, 0, 64);
  int lowest = 0;
  while (!(unit_bits >> lowest & 1)) lowest++;
  return KVZ_CU_QP_WORD(0, q, 1, cu_qp_cu_start(J, frame, cx, cy, lowest));
}
// step 2, substream `chain` of the job (a CTU row of a picture; no_wpp: a picture): every CTU's predictor
KVZ_HD void cu_qp_chain(const CuQpJob &J, long chain)
{
  const int rows = J.no_wpp ? 1 : J.hc, n = J.no_wpp ? J.wc * J.hc : J.wc;
  const long frame = chain / rows;
  uint32_t *w = J.ctu_qp + frame * J.wc * J.hc + (chain % rows) * n;
  int last = J.qp_of_picture[frame];
  for (int k = 0; k < n; k++) {
    const uint32_t word = w[k];
    w[k] = word | (uint32_t)last;  // pred = last
    if (word >> 16 & 1) last = (int)(word >> 8 & 0xff);
  }
}
// step 3, the QP of the CU that covers 8x8 unit (x8, y8) of the picture
KVZ_HD void cu_qp_unit(const CuQpJob &J, long frame, int x8, int y8)
{
  const int cx = x8 >> 3, cy = y8 >> 3;
  const uint32_t word = J.ctu_qp[frame * J.wc * J.hc + (long)cy * J.wc + cx];
  const int start = cu_qp_cu_start(J, frame, cx, cy, cu_qp_unit_index(x8 & 7, y8 & 7));
  J.cu_qp[frame * (long)(J.W >> 3) * (J.H >> 3) + (long)y8 * (J.W >> 3) + x8] = (uint8_t)(start >= (int)(word >> 24) ? word >> 8 : word);
}

#ifdef __HIPCC__
// step 1: a wavefront per CTU, a lane per 8x8 unit
__global__ void __launch_bounds__(256) dev_cu_qp_cbf_kernel(const CuQpJob J, const long ctus_total)
{
  const long ctu = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ctu >= ctus_total) return;  // (the whole wavefront)
  const int per = J.wc * J.hc, lane = threadIdx.x & 63;
  const long frame = ctu / per;
  const int r = (int)(ctu % per), cx = r % J.wc, cy = r / J.wc;
  const unsigned long long bits = __ballot(cu_qp_unit_bit(J, frame, cx, cy, lane));
  if (lane == 0) J.ctu_qp[ctu] = cu_qp_ctu_word(J, frame, cx, cy, bits);
}
// step 2: a lane per substream
__global__ void __launch_bounds__(64) dev_cu_qp_chain_kernel(const CuQpJob J, const long chains)
{
  const long c = (long)blockIdx.x * 64 + threadIdx.x;
  if (c < chains) cu_qp_chain(J, c);
}
// step 3: a lane per 8x8 unit
__global__ void __launch_bounds__(256) dev_cu_qp_plane_kernel(const CuQpJob J, const long units)
{
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= units) return;
  const int w8 = J.W >> 3, per = w8 * (J.H >> 3), r = (int)(p % per);
  cu_qp_unit(J, p / per, r % w8, r / w8);
}
inline void cu_qp_frames_on(hipStream_t stream, const CuQpJob &J)
{
  const long ctus = (long)J.n_frames * J.wc * J.hc, chains = (long)J.n_frames * (J.no_wpp ? 1 : J.hc), units = (long)J.n_frames * (J.W >> 3) * (J.H >> 3);
  hipLaunchKernelGGL(dev_cu_qp_cbf_kernel, dim3((unsigned)((ctus + 3) / 4)), dim3(256), 0, stream, J, ctus);
  hipLaunchKernelGGL(dev_cu_qp_chain_kernel, dim3((unsigned)((chains + 63) / 64)), dim3(64), 0, stream, J, chains);
  hipLaunchKernelGGL(dev_cu_qp_plane_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, stream, J, units);
}
#endif

}  // namespace kvz
