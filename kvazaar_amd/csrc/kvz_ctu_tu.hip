// kvz_ctu_tu.hip -- one CTU kernel instantiation per translation unit (see kvz_ctu_kernels.hpp): compiled by kvazaar_amd/build.py once per unit of
// kvz_ctu_builds.hpp, with -DKVZ_CTU_KERNEL_TU=<unit>, in parallel with kvz_hip.hip.
#include <hip/hip_runtime.h>

#ifndef KVZ_CTU_KERNEL_TU
#error "compile with -DKVZ_CTU_KERNEL_TU=<unit of kvz_ctu_builds.hpp>"
#endif
#include "kvz_ctu_kernels.hpp"

namespace kvz {
static_assert(KVZ_CTU_KERNEL_TU >= 0 && KVZ_CTU_KERNEL_TU < 64 && (KVZ_CTU_UNIT_MASK >> KVZ_CTU_KERNEL_TU & 1), "KVZ_CTU_KERNEL_TU is no unit of kvz_ctu_builds.hpp");
// Naming a kernel instantiates it, and unlike an explicit instantiation a name can depend on the unit: the list's build with the unit's number and, behind it so that the
// objects keep their layout, the older schedule's kernel where the unit has one.  (The template arguments depend on UNIT: a discarded statement names nothing.)
template <int UNIT> const void *ctu_unit_kernel(bool older_schedule)
{
  const void *k = nullptr;
#define KVZ_CTU_X(unit, ...) if constexpr (unit == UNIT) k = (const void *)ctu_build_kernel(CtuBuild<UNIT, __VA_ARGS__>{});
  KVZ_CTU_BUILDS(KVZ_CTU_X)
#undef KVZ_CTU_X
#define KVZ_CTU_X(unit, CABAC) if constexpr (unit == UNIT) if (older_schedule) k = (const void *)&intra_ctu_wave_kernel<CABAC && unit == UNIT>;
  KVZ_CTU_WAVE_BUILDS(KVZ_CTU_X)
#undef KVZ_CTU_X
  return k;
}
template const void *ctu_unit_kernel<KVZ_CTU_KERNEL_TU>(bool);
}  // namespace kvz
