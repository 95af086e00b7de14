// kvz_select.hpp -- the mode selection of search_intra_rough (search_intra.c:433-530) on a table of 35 SATDs: what a mode's table entry and cost are (one text for
// the host simulation and the device), and the device form of the selection, which one wavefront runs with mode m's values in lane m.  The serial statement of
// the reference's order is CtuProgramT::replay_selection's host form (kvz_ctu.hpp); tests/test_intra_select.py holds the two against a restatement in Python.
#pragma once
#include "kvz_ops.hpp"

namespace kvz {

// SATD_NxN of a CU made of nblk 8x8 blocks: the sum of (block sum + 2) >> 2 (strategies-picture.h:53-69)
KVZ_DEV u32 select_satd_sum(const u32 *blocks, int nblk)
{
  u32 v = 0;
  for (int b = 0; b < nblk; b++) v += (blocks[b] + 2) >> 2;
  return v;
}
// search_intra.c:524-529: a mode's cost is its SATD plus lambda_sqrt * kvz_luma_mode_bits, which only knows three outcomes (price_modes):
// bits[1] the first most probable mode, bits[2] the second or third, bits[0] any other
KVZ_DEV double select_mode_cost(u32 raw, int mode, int p0, int p1, int p2, const double bits[3])
{
  return (double)raw + bits[mode == p0 ? 1 : ((mode == p1 || mode == p2) ? 2 : 0)];
}

#ifndef KVZ_HOSTSIM
// Minimum of v over the wavefront, the same value in every lane's result (it is read from lane 63).  Six DPP steps with the identity as the value of a lane that has
// no source -- row_shr 1 / 2 / 4 / 8 leave the minimum of a row of 16 in its last lane, row_bcast:15 and row_bcast:31 carry it across the rows -- so that the
// compiler folds each step into one v_min_u32_dpp.  Every lane of the wavefront must be here.
KVZ_DEV unsigned wave_min_u32(unsigned v)
{
  int x = (int)v;
#define KVZ_MIN32_STEP(ctrl) { const unsigned o = (unsigned)__builtin_amdgcn_update_dpp(-1, x, ctrl, 0xF, 0xF, false); x = (int)(o < (unsigned)x ? o : (unsigned)x); }
  KVZ_MIN32_STEP(0x111) KVZ_MIN32_STEP(0x112) KVZ_MIN32_STEP(0x114) KVZ_MIN32_STEP(0x118) KVZ_MIN32_STEP(0x142) KVZ_MIN32_STEP(0x143)
#undef KVZ_MIN32_STEP
  return (unsigned)__builtin_amdgcn_readlane(x, 63);
}

// The selection by one whole wavefront: lane m (m < 35) brings mode m's SATD and cost (select_mode_cost); p0..p2 are the most probable modes, log2w the block's
// size (2: a 4x4 PU).  Returns the winner in every lane.  What kvazaar keeps as a list (modes[], costs[]) is only ever read back as "first minimum in append order",
// so an append only records WHEN a mode was appended, in the lane that holds the mode, and the list's minimum is taken once at the end.
//  - The initial pass visits a fixed set of lanes (2, 2 + offset, ... 34) in increasing mode order: its minimum, and the first mode that has it, are ONE wavefront
//    minimum of raw << 6 | mode (an SATD of 8-bit samples stays below 2^21 even for a 32x32 CU: 16 blocks x 8 * 64 * 255 / 4), and min_cost == max_cost is "no
//    candidate lane differs from the minimum".
//  - The refinement compares SATDs as the integers they are: the reference converts both sides to double, which is exact and monotone for a u32.
//  - The final pick: costs are non-negative doubles, which order like their bit patterns.  The minimum of the high words, then of the low words among the lanes that
//    hold it, then of position << 6 | lane among the lanes that hold both -- three 32-bit minima.
KVZ_DEV int select_on_wave(int lane, u32 my_raw, double my_cost, int p0, int p1, int p2, int log2w)
{
  const int lo = log2w == 2 ? 1 : (log2w == 3 ? 2 : 3);  // log2 of the initial offset (search_intra.c:446)
  int offset = 1 << lo;
  // the initial pass's modes as a mask: bit m = mode m
  unsigned long long visited = lo == 1 ? 0x555555554ull : (lo == 2 ? 0x444444444ull : 0x404040404ull);
  const bool cand = (visited >> lane) & 1;
  int my_pos = cand ? (lane - 2) >> lo : 0, n_app = (32 >> lo) + 1;
#define KVZ_SEL_RAW(md) ((u32)__builtin_amdgcn_readlane((int)my_raw, (md)))
#define KVZ_SEL_APPEND(md) { visited |= 1ull << (md); if (lane == (md)) my_pos = n_app; n_app++; }
  const unsigned kmin = wave_min_u32(cand ? (my_raw << 6) | (unsigned)lane : ~0u);
  u32 best_raw = kmin >> 6;
  int best_mode = (int)(kmin & 63);
  if (__builtin_amdgcn_ballot_w64(cand && my_raw != best_raw) != 0) {  // min_cost != max_cost
    while (offset > 1) {
      offset >>= 1;
      const int tm[2] = { best_mode - offset, best_mode + offset };
      for (int i = 0; i < 2; i++) if (tm[i] >= 2 && tm[i] <= 34) {
        const u32 raw = KVZ_SEL_RAW(tm[i]);
        KVZ_SEL_APPEND(tm[i]);
        if (raw < best_raw) { best_raw = raw; best_mode = tm[i]; }
      }
    }
  }
  const int add_modes[5] = { __builtin_amdgcn_readfirstlane(p0), __builtin_amdgcn_readfirstlane(p1), __builtin_amdgcn_readfirstlane(p2), 0, 1 };
  for (int p = 0; p < 5; p++)
    if (!((visited >> add_modes[p]) & 1)) KVZ_SEL_APPEND(add_modes[p]);
#undef KVZ_SEL_APPEND
#undef KVZ_SEL_RAW
  const bool mine = (visited >> lane) & 1;  // (modes stop at 34: no bit from 35 on)
  const unsigned hi = mine ? (unsigned)__double2hiint(my_cost) : ~0u, hi_min = wave_min_u32(hi);
  const bool at_hi = mine && hi == hi_min;
  const unsigned lw = at_hi ? (unsigned)__double2loint(my_cost) : ~0u, lw_min = wave_min_u32(lw);
  return (int)(wave_min_u32((at_hi && lw == lw_min) ? (unsigned)((my_pos << 6) | lane) : ~0u) & 63);
}
#endif

}  // namespace kvz
