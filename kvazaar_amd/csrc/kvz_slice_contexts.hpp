// kvz_slice_contexts.hpp -- the entropy coder's initial context states of an inter slice (kvz_init_contexts, context.c:202-305), B or P, in the coder's numbering:
// KVZ_HIP_CX_* (kvz_hip_types.h) then KVZ_EB_CX_* (kvz_entropy.hpp).  The values are kvz_inter_host.hpp's (slice_syntax_init, slice_residual_init_values), which
// the inter CTU pass's search contexts are filled from as well.  Host code: kvz_dev.hpp fills the coder's rows with it, the host simulation of the P coder
// (tests/hostsim/hostsim_inter_p.cpp) the rows of its twin.
#pragma once
#include "kvz_entropy.hpp"
#include "kvz_inter_host.hpp"

namespace kvz {

// refs: pictures with reference lists (kvz_hip_dev_entropy_code_inter_refs) -- the set then holds ref_idx_l0's two contexts (KVZ_EB_CX_REF_IDX)
inline void entropy_slice_contexts(int slice_type, int qp, uint8_t out[KVZ_ENTROPY_CTXS], bool refs = false)
{
  const SliceSyntaxInit &v = slice_syntax_init(slice_type);
  uint8_t init[KVZ_ENTROPY_CTXS];
  memset(init, 154, sizeof init);
  for (int i = 0; i < 3; i++) { init[KVZ_HIP_CX_SPLIT + i] = v.split[i]; init[KVZ_EB_CX_SKIP + i] = v.skip[i]; }
  init[KVZ_HIP_CX_PART] = v.part; init[KVZ_HIP_CX_INTRA] = v.intra; init[KVZ_HIP_CX_CHROMA] = v.chroma;
  init[KVZ_HIP_CX_CBF_LUMA] = v.cbf_luma[0]; init[KVZ_HIP_CX_CBF_LUMA + 1] = v.cbf_luma[1];
  init[KVZ_HIP_CX_CBF_CHROMA] = v.cbf_chroma[0]; init[KVZ_HIP_CX_CBF_CHROMA + 1] = v.cbf_chroma[1]; init[KVZ_HIP_CX_CBF_CHROMA_DEEP] = v.cbf_chroma[2]; init[KVZ_HIP_CX_CBF_CHROMA_DEEP + 1] = v.cbf_chroma[3];
  slice_residual_init_values(slice_type, init + KVZ_HIP_CX_SIG_CG);
  init[KVZ_HIP_CX_SAO_MERGE] = v.sao_merge; init[KVZ_HIP_CX_SAO_TYPE] = v.sao_type;
  init[KVZ_EB_CX_MERGE_FLAG] = v.merge_flag; init[KVZ_EB_CX_MERGE_IDX] = v.merge_idx; init[KVZ_EB_CX_PRED_MODE] = v.pred_mode;
  init[KVZ_EB_CX_MVD] = v.mvd[0]; init[KVZ_EB_CX_MVD + 1] = v.mvd[1]; init[KVZ_EB_CX_MVP_IDX] = v.mvp_idx;
  for (int i = 0; i < 5; i++) init[KVZ_EB_CX_INTER_DIR + i] = v.inter_dir[i];
  init[KVZ_EB_CX_ROOT_CBF] = v.root_cbf;
  if (refs) { init[KVZ_EB_CX_REF_IDX] = v.ref_idx[0]; init[KVZ_EB_CX_REF_IDX + 1] = v.ref_idx[1]; }
  for (int i = 0; i < KVZ_ENTROPY_CTXS; i++) out[i] = (uint8_t)inter_ctx_state(qp, init[i]);
}

// INIT_SAO_TYPE_IDX of a slice type (H.265 Table 9-6): what the SAO decision of the loop filters starts from; INIT_SAO_MERGE_FLAG is 153 in every row
inline int sao_type_init_value(int slice_type) { return slice_type == KVZ_HIP_SLICE_B ? 160 : (slice_type == KVZ_HIP_SLICE_P ? 185 : 200); }

}  // namespace kvz
