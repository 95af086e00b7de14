// kvz_ctu_qp_tu.hip -- one instantiation of the CTU kernel that fetches a model per CTU (kvz_ctu_kernels.hpp intra_ctu_ticket_kernel_ctuqp) per translation unit:
// compiled by kvazaar_amd/build.py once per unit of kvz_ctu_qp_builds.hpp, with -DKVZ_CTU_QP_KERNEL_TU=<unit>, in parallel with kvz_hip.hip and the units of kvz_ctu_tu.hip.
#include <hip/hip_runtime.h>

#ifndef KVZ_CTU_QP_KERNEL_TU
#error "compile with -DKVZ_CTU_QP_KERNEL_TU=<unit of kvz_ctu_qp_builds.hpp>"
#endif
#include "kvz_ctu_kernels.hpp"

namespace kvz {
static_assert(KVZ_CTU_QP_KERNEL_TU >= 0 && KVZ_CTU_QP_KERNEL_TU < 64 && (KVZ_CTU_QP_UNIT_MASK >> KVZ_CTU_QP_KERNEL_TU & 1), "KVZ_CTU_QP_KERNEL_TU is no unit of kvz_ctu_qp_builds.hpp");
// Naming a kernel instantiates it (kvz_ctu_tu.hip): the list's build with the unit's number
template <int UNIT> const void *ctu_qp_unit_kernel()
{
  const void *k = nullptr;
#define KVZ_CTU_QP_X(unit, CABAC, S32) if constexpr (unit == UNIT) k = (const void *)&intra_ctu_ticket_kernel_ctuqp<CABAC && unit == UNIT, S32 && unit == UNIT>;
  KVZ_CTU_QP_BUILDS(KVZ_CTU_QP_X)
#undef KVZ_CTU_QP_X
  return k;
}
template const void *ctu_qp_unit_kernel<KVZ_CTU_QP_KERNEL_TU>();
}  // namespace kvz
