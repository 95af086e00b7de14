// kvz_ctu_qp_builds.hpp -- the builds of the all-intra CTU pass that fetch a cost model per CTU (kvz_hip_intra_frames_ctu_models), and which of them a launch
// takes: stated here, once, beside kvz_ctu_builds.hpp, whose list and units stay what they are.  No HIP dependency: kvz_ctu_kernels.hpp and kvz_ctu_qp_tu.hip
// instantiate the kernels from the list, kvz_batch.hpp asks ctu_qp_build_choose and launches through ctu_qp_build_dispatch, kvazaar_amd/build.py reads the unit
// numbers (and is checked: KVZ_CTU_QP_UNITS_BUILT), and the host simulation (tests/hostsim/hostsim_ctu_qp.cpp) picks its instantiation of the program with the same text.
#pragma once
#include "kvz_ctu_builds.hpp"

namespace kvz {

// X(unit, CABAC, S32): the translation unit that holds the build (kvz_ctu_qp_tu.hip with -DKVZ_CTU_QP_KERNEL_TU=<unit>) and the kernel's compile-time switches -- the
// CABAC coefficient cost model and 32x32 CUs searched, as in KVZ_CTU_BUILDS.  Maps exist for the presets without kvz_rdoq, NxN partitions, sign hiding and scaling
// lists, and for a batch on its own: what ctu_models_known (kvz_cu_qp.hpp) refuses never asks here.
#define KVZ_CTU_QP_BUILDS(X) \
  X(0, 0, 0)                 \
  X(1, 1, 0)                 \
  X(2, 0, 1)                 \
  X(3, 1, 1)

#define KVZ_CTU_QP_X(unit, ...) | 1ull << unit
constexpr unsigned long long KVZ_CTU_QP_UNIT_MASK = 0 KVZ_CTU_QP_BUILDS(KVZ_CTU_QP_X);  // the translation units, a bit each
#undef KVZ_CTU_QP_X
#ifdef KVZ_CTU_QP_UNITS_BUILT  // the units build.py compiles: what its pattern finds in the list above
static_assert(KVZ_CTU_QP_UNITS_BUILT == KVZ_CTU_QP_UNIT_MASK, "kvazaar_amd/build.py does not read the units of KVZ_CTU_QP_BUILDS as the compiler does");
#endif

// The unit of the build that serves a launch with a map (search_32x32: the switch every model of the table shares; any_cabac: some model of the table prices
// coefficients with the CABAC model -- that build prices the other CTUs' through its run-time switch).  Every accepted launch has one.
constexpr int ctu_qp_build_choose(bool search_32x32, bool any_cabac)
{
#define KVZ_CTU_QP_X(unit, CABAC, S32) \
  if (any_cabac == bool(CABAC) && search_32x32 == bool(S32)) return unit;
  KVZ_CTU_QP_BUILDS(KVZ_CTU_QP_X)
#undef KVZ_CTU_QP_X
  return KVZ_CTU_BUILD_NONE;
}

// f(CtuBuild<...>{}) for the build of `unit` -- as a row of KVZ_CTU_BUILDS without kvz_rdoq, sign hiding, lists and joint launches, so that what takes such a
// row (the host simulation's run_ctu) takes these; false when the list has none (f is not called)
template <class F> bool ctu_qp_build_dispatch(int unit, F &&f)
{
#define KVZ_CTU_QP_X(u, CABAC, S32) if (unit == u) { f(CtuBuild<u, CABAC, S32, 0, 0, 0, 0>{}); return true; }
  KVZ_CTU_QP_BUILDS(KVZ_CTU_QP_X)
#undef KVZ_CTU_QP_X
  return false;
}

}  // namespace kvz
