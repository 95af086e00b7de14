// kvz_inter_builds.hpp -- the builds of the inter CTU pass's persistent kernel, and which of them a launch takes: stated here, once (as kvz_ctu_builds.hpp states the
// all-intra pass's).  No HIP dependency: kvz_inter_kernels.hpp declares the kernels from the list and checks the one a translation unit defines against it, kvz_dev.hpp
// asks inter_build_choose and reaches the kernel through inter_build_kernel, kvazaar_amd/build.py reads the units and their switches (and is checked:
// KVZ_ICTU_UNITS_BUILT), and the host simulation (tests/hostsim) hands the list and the choice to tests/test_inter_builds_sim.py.
#pragma once

namespace kvz {

// X(unit, suffix, CABAC, LISTS, JOINT, ME, P, REFS): the translation unit that holds the build (kvz_inter_tu.hip, object kvz_inter_tu<unit>; `only_units` of
// build.py's build_variant names them), the kernel's name behind inter_ctu_ticket_kernel_, and the program's compile-time switches (-DKVZ_ICTU_<switch>=1):
//   CABAC  the residual coder's contexts in the LDS context sets, for pictures whose coefficients are priced with them; without it (`fast`) the pictures' are priced
//          by kvz_fast_coeff_cost and the sets are small (kvz_inter_ctu.hpp KVZ_ICTU_CABAC).  One build serves a launch: where any picture prices with the contexts
//          the launch takes the CABAC build, which prices the others' through its run-time switch (InterModel::coeff_cabac)
//   LISTS  scaling lists (kvz_hip_dev_inter_ctu_pass_lists): every picture's record carries its rows of the factor table
//   JOINT  pictures of different sizes in one launch (kvz_hip_dev_inter_ctu_pass_groups): the item's picture numbers the pictures across the groups; F holds no
//          geometry, F.pictures the launch's table (kvz_inter_ctu.hpp InterJointPicture / InterJointGroup), and sched.done is indexed by the group's first CTU + the
//          picture's index in the group x the group's CTUs + the CTU
//   ME     a chosen integer motion search (kvz_hip_inter_params me_algorithm / me_max_steps / me_early_termination); these builds raise the launch's error word
//          when a search loop reached its bound (kvz_inter_ctu_pix.inc IC_ME_LOOP_BOUND)
//   P      P pictures (kvz_hip_dev_inter_ctu_pass_slices with KVZ_HIP_SLICE_P): the program without its L1 half (kvz_inter_ctu.hpp KVZ_ICTU_P)
//   REFS   P pictures with reference lists (kvz_hip_dev_inter_ctu_pass_refs), always together with P: F.ref / F.ref_cu are a pool of frames and F.pictures holds
//          InterPictureRefs records (kvz_inter_ctu.hpp KVZ_ICTU_REFS)
// LISTS, JOINT, ME and P exclude one another (kvz_inter_kernels.hpp refuses to compile the combinations).  A new build is a row, its case, and its line in the test.
#define KVZ_ICTU_BUILDS(X)            \
  X(0, fast, 0, 0, 0, 0, 0, 0)        \
  X(1, cabac, 1, 0, 0, 0, 0, 0)       \
  X(2, lists_fast, 0, 1, 0, 0, 0, 0)  \
  X(3, lists_cabac, 1, 1, 0, 0, 0, 0) \
  X(4, joint_fast, 0, 0, 1, 0, 0, 0)  \
  X(5, joint_cabac, 1, 0, 1, 0, 0, 0) \
  X(6, me_fast, 0, 0, 0, 1, 0, 0)     \
  X(7, me_cabac, 1, 0, 0, 1, 0, 0)    \
  X(8, p_fast, 0, 0, 0, 0, 1, 0)      \
  X(9, p_cabac, 1, 0, 0, 0, 1, 0)     \
  X(10, refs_fast, 0, 0, 0, 0, 1, 1)  \
  X(11, refs_cabac, 1, 0, 0, 0, 1, 1)

constexpr int KVZ_ICTU_BUILD_NONE = -1;
#define KVZ_ICTU_X(unit, ...) | 1ull << unit
constexpr unsigned long long KVZ_ICTU_UNIT_MASK = 0 KVZ_ICTU_BUILDS(KVZ_ICTU_X);  // the translation units, a bit each
#undef KVZ_ICTU_X
#ifdef KVZ_ICTU_UNITS_BUILT  // the units build.py compiles: what its pattern finds in the list above
static_assert(KVZ_ICTU_UNITS_BUILT == KVZ_ICTU_UNIT_MASK, "kvazaar_amd/build.py does not read the units of KVZ_ICTU_BUILDS as the compiler does");
#endif

// What a launch knows after its checks have passed: whether any of its pictures prices coefficients with the residual coder's contexts, and its kind
struct InterLaunch { bool any_cabac, lists, joint, me, p_slice, refs; };
// The unit of the build that serves the launch, or KVZ_ICTU_BUILD_NONE where no build does -- what inter_slice_launch_known, inter_refs_launch_known, inter_me_known
// and inter_joint_known refuse, with their reasons, before anything asks here
constexpr int inter_build_choose(const InterLaunch &l)
{
#define KVZ_ICTU_X(unit, suffix, CABAC, LISTS, JOINT, ME, P, REFS) \
  if (l.any_cabac == bool(CABAC) && l.lists == bool(LISTS) && l.joint == bool(JOINT) && l.me == bool(ME) && l.p_slice == bool(P) && l.refs == bool(REFS)) return unit;
  KVZ_ICTU_BUILDS(KVZ_ICTU_X)
#undef KVZ_ICTU_X
  return KVZ_ICTU_BUILD_NONE;
}

// the suffix of a unit's kernel name; "" where the list has no such unit
constexpr const char *inter_build_suffix(int unit)
{
#define KVZ_ICTU_X(u, suffix, ...) if (unit == u) return #suffix;
  KVZ_ICTU_BUILDS(KVZ_ICTU_X)
#undef KVZ_ICTU_X
  return "";
}
// is `suffix` the suffix of unit `unit` of the list?  (the check of the name a translation unit defines: kvz_inter_kernels.hpp)
constexpr bool inter_build_named(int unit, const char *suffix)
{
  const char *s = inter_build_suffix(unit);
  if (!*s) return false;
  while (*s && *s == *suffix) { ++s; ++suffix; }
  return *s == *suffix;
}

}  // namespace kvz
