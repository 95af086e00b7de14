// kvz_ctu_builds.hpp -- the builds of the all-intra CTU pass's persistent kernel, and which of them a launch takes: stated here, once.
// No HIP dependency: kvz_ctu_kernels.hpp and kvz_ctu_tu.hip instantiate the kernels from the list, kvz_batch.hpp asks ctu_build_choose and launches through
// ctu_build_dispatch, kvazaar_amd/build.py reads the unit numbers (and is checked: KVZ_CTU_UNITS_BUILT), and the host simulation (tests/hostsim) picks its instantiation of the program with the same text.
// A new build is a line of the list, its case in ctu_build_choose and that function's test (tests/test_ctu_builds_sim.py).
#pragma once

namespace kvz {

// X(unit, CABAC, S32, RDOQ, SH, LISTS, JOINT): the translation unit that holds the build (kvz_ctu_tu.hip with -DKVZ_CTU_KERNEL_TU=<unit>; `only_units` of
// build.py's build_variant names them) and the kernel's compile-time switches -- the CABAC coefficient cost model (without it a build carries none of its code,
// registers or context storage), 32x32 CUs searched (--pu-depth-intra 1-3), kvz_rdoq and NxN partitions (preset `medium`), sign data hiding, scaling lists, and the
// drawn picture's batch fetched per ticket (kvz_hip_batch_group).
#define KVZ_CTU_BUILDS(X) \
  X(0, 0, 0, 0, 0, 0, 0)  \
  X(1, 1, 0, 0, 0, 0, 0)  \
  X(3, 0, 1, 0, 0, 0, 0)  \
  X(4, 1, 1, 0, 0, 0, 0)  \
  X(5, 1, 1, 1, 0, 0, 0)  \
  X(6, 1, 0, 0, 1, 0, 0)  \
  X(7, 1, 1, 0, 1, 0, 0)  \
  X(8, 0, 0, 0, 0, 1, 0)  \
  X(9, 1, 0, 0, 0, 1, 0)  \
  X(10, 0, 1, 0, 0, 1, 0) \
  X(11, 1, 1, 0, 0, 1, 0) \
  X(12, 0, 0, 0, 0, 0, 1) \
  X(13, 1, 0, 0, 0, 0, 1) \
  X(14, 0, 1, 0, 0, 0, 1) \
  X(15, 1, 1, 0, 0, 0, 1) \
  X(16, 1, 0, 0, 1, 0, 1) \
  X(17, 1, 1, 0, 1, 0, 1)
// X(unit, CABAC): the two kernels of the older schedule, one launch per anti-diagonal (intra_ctu_wave_kernel<CABAC>), behind unit 0's build and alone in a unit
#define KVZ_CTU_WAVE_BUILDS(X) X(0, 0) X(2, 1)

template <int UNIT, bool CABAC, bool S32, bool RDOQ, bool SH, bool LISTS, bool JOINT> struct CtuBuild {  // a line of the list as a type
  static constexpr int unit = UNIT, cabac = CABAC, s32 = S32, rdoq = RDOQ, sh = SH, lists = LISTS, joint = JOINT;
};

constexpr int KVZ_CTU_BUILD_NONE = -1;
#define KVZ_CTU_X(unit, ...) | 1ull << unit
constexpr unsigned long long KVZ_CTU_UNIT_MASK = 0 KVZ_CTU_BUILDS(KVZ_CTU_X) KVZ_CTU_WAVE_BUILDS(KVZ_CTU_X);  // the translation units, a bit each
#undef KVZ_CTU_X
#ifdef KVZ_CTU_UNITS_BUILT  // the units build.py compiles: what its pattern finds in the two lists above
static_assert(KVZ_CTU_UNITS_BUILT == KVZ_CTU_UNIT_MASK, "kvazaar_amd/build.py does not read the units of KVZ_CTU_BUILDS / KVZ_CTU_WAVE_BUILDS as the compiler does");
#endif

// What a launch knows: the switches every model of the launch shares (kvz_picture_models.hpp), whether any of its pictures prices coefficients with the CABAC model or
// hides sign bits, whether the batch has scaling lists, and whether it is a group's joint launch.
struct CtuLaunch { bool search_32x32, rdoq, search_nxn, any_cabac, any_signhide, lists, joint; };
// The unit of the build that serves the launch, or KVZ_CTU_BUILD_NONE where no build does -- what signhide_known, scaling_lists_known and joint_launch_known refuse,
// with their reasons, before anything asks here.  One build serves the whole launch: a picture that prices with the CABAC model moves it to a CABAC build, which
// prices the others' through its run-time switch; sign hiding anywhere takes a sign-hiding build, all of which carry the CABAC model; kvz_rdoq and NxN partitions
// share the one build that has both, with the 32x32 search and the coefficient cost model switched by the model.
constexpr int ctu_build_choose(const CtuLaunch &l)
{
  const bool rdoq = l.rdoq || l.search_nxn, sh = l.any_signhide, cabac = rdoq || sh || l.any_cabac, s32 = rdoq || l.search_32x32;
#define KVZ_CTU_X(unit, CABAC, S32, RDOQ, SH, LISTS, JOINT) \
  if (cabac == bool(CABAC) && s32 == bool(S32) && rdoq == bool(RDOQ) && sh == bool(SH) && l.lists == bool(LISTS) && l.joint == bool(JOINT)) return unit;
  KVZ_CTU_BUILDS(KVZ_CTU_X)
#undef KVZ_CTU_X
  return KVZ_CTU_BUILD_NONE;
}

// f(CtuBuild<...>{}) for the build of `unit`; false when the list has none (f is not called)
template <class F> bool ctu_build_dispatch(int unit, F &&f)
{
#define KVZ_CTU_X(u, ...) if (unit == u) { f(CtuBuild<u, __VA_ARGS__>{}); return true; }
  KVZ_CTU_BUILDS(KVZ_CTU_X)
#undef KVZ_CTU_X
  return false;
}

}  // namespace kvz
