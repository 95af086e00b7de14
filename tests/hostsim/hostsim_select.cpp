// hostsim_select.cpp -- TEST INFRASTRUCTURE (see hostsim.cpp, which this unit includes whole).  The serial host form of the intra mode selection
// (CtuProgramT::replay_selection, the statement of search_intra.c:433-530's order) on tables, with the layout of kvz_hip_dev_intra_select: what the device form
// (kvz_select.hpp select_on_wave) has to agree with.  tests/test_intra_select.py builds and uses it.
#include "hostsim.cpp"

// winner[i] of table i: raw + i * 35 * nblk (35 modes x nblk 8x8-block SATDs), preds + 3 i, mode_bits + 3 i.  0, or -1 for a shape the pass does not have.
extern "C" int kvz_hostsim_intra_select(int log2w, int nblk, const uint32_t *raw, const int8_t *preds, const double *mode_bits, int count, int32_t *winner)
{
  if (!((log2w == 3 && nblk == 1) || (log2w == 4 && nblk == 4))) return -1;
  typedef kvz::CtuSharedT<false> Shared;
  Shared *sh = (Shared *)calloc(1, sizeof(Shared));
  kvz::CtuProgramT<false> p;
  p.s = sh;
  for (long i = 0; i < count; i++) {
    for (int m = 0; m < 35; m++)
      for (int b = 0; b < nblk; b++) sh->satd_raw[m][b] = raw[(i * 35 + m) * nblk + b];
    for (int k = 0; k < 3; k++) { sh->preds[k] = preds[3 * i + k]; sh->mode_bits_cost[k] = mode_bits[3 * i + k]; }
    winner[i] = p.replay_selection(0, log2w, nblk);
  }
  free(sh);
  return 0;
}
