// kvz_scaling_lists.hpp -- host side of the per-coefficient scaling lists of the CTU passes (include/kvz_hip_types.h kvz_hip_scaling_lists): the check of
// what kvz_hip_batch_set_scaling_lists / kvz_hip_dev_inter_ctu_pass_lists are handed, and the factor rows the LISTS builds read (kvz_recon.hpp list_index; kvz_ctu.hpp,
// kvz_inter_ctu_pix.inc).  Host code without a HIP
// dependency: kvz_batch.hpp calls it, and the host simulation (tests/hostsim) compiles the same text.
#pragma once
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/kvz_hip_types.h"
#include "kvz_recon.hpp"
#include "kvz_tables.hpp"

namespace kvz {

// kvz_scalinglist_get_default (scalinglist.c:266-282): H.265 table 7-5 (4x4: flat 16) and table 7-6, intra (lists 0-2; list 0 at 32x32) and inter
inline void scaling_lists_default(kvz_hip_scaling_lists *l)
{
  static const uint8_t intra8[64] = { 16, 16, 16, 16, 17, 18, 21, 24, 16, 16, 16, 16, 17, 19, 22, 25, 16, 16, 17, 18, 20, 22, 25, 29, 16, 16, 18, 21, 24, 27, 31, 36,
                                      17, 17, 20, 24, 30, 35, 41, 47, 18, 19, 22, 27, 35, 44, 54, 65, 21, 22, 25, 31, 41, 54, 70, 88, 24, 25, 29, 36, 47, 65, 88, 115 };
  static const uint8_t inter8[64] = { 16, 16, 16, 16, 17, 18, 20, 24, 16, 16, 16, 17, 18, 20, 24, 25, 16, 16, 17, 18, 20, 24, 25, 28, 16, 17, 18, 20, 24, 25, 28, 33,
                                      17, 18, 20, 24, 25, 28, 33, 41, 18, 20, 24, 25, 28, 33, 41, 54, 20, 24, 25, 28, 33, 41, 54, 71, 24, 25, 28, 33, 41, 54, 71, 91 };
  memset(l, 0, sizeof *l);
  l->struct_size = (uint32_t)sizeof *l;
  for (int size = 0; size < 4; size++)
    for (int list = 0; list < (size == 3 ? 2 : 6); list++) {
      const bool inter = size == 3 ? list > 0 : list > 2;
      for (int i = 0; i < (size == 0 ? 16 : 64); i++) l->coeff[size][list][i] = size == 0 ? 16 : (inter ? inter8[i] : intra8[i]);
      l->dc[size][list] = 16;
    }
}

// Everything kvz_hip_batch_set_scaling_lists and kvz_hip_dev_inter_ctu_pass_lists refuse (ticket_schedule: the batch does not run under KVZ_HIP_SCHED=wave)
inline bool scaling_list_sets_known(const kvz_hip_scaling_lists *sets, int n_sets, const uint16_t *set_of_picture, int n_frames, bool ticket_schedule, const char *who)
{
  if (n_sets == 0) return true;  // clears the state
  if (n_sets < 0 || n_sets > 65535 || !sets) { fprintf(stderr, "%s: 0 .. 65535 scaling list sets (n_sets %d)\n", who, n_sets); return false; }
  for (int k = 0; k < n_sets; k++) {
    const kvz_hip_scaling_lists &l = sets[k];
    if (l.struct_size != sizeof(kvz_hip_scaling_lists)) {  // (a set of another size would also shift every set behind it)
      fprintf(stderr, "%s: kvz_hip_scaling_lists.struct_size %u of set %d is not this library's %zu\n", who, l.struct_size, k, sizeof(kvz_hip_scaling_lists));
      return false;
    }
    for (int size = 0; size < 4; size++)
      for (int list = 0; list < (size == 3 ? 2 : 6); list++) {
        for (int i = 0; i < (size == 0 ? 16 : 64); i++)
          if (l.coeff[size][list][i] < 13 || l.coeff[size][list][i] > 255) {
            fprintf(stderr, "%s: scaling list set %d, size %d list %d entry %d is %d: entries lie in 13 .. 255\n", who, k, size, list, i, l.coeff[size][list][i]);
            return false;
          }
        if (l.dc[size][list] != 0 && (l.dc[size][list] < 13 || l.dc[size][list] > 255)) {
          fprintf(stderr, "%s: scaling list set %d, size %d list %d DC term is %d: 0 (= 16) or 13 .. 255\n", who, k, size, list, l.dc[size][list]);
          return false;
        }
      }
  }
  for (int f = 0; set_of_picture && f < n_frames; f++)
    if (set_of_picture[f] != 0xffff && set_of_picture[f] >= n_sets) { fprintf(stderr, "%s: set_of_picture[%d] = %u of %d scaling list sets\n", who, f, (unsigned)set_of_picture[f], n_sets); return false; }
  if (!ticket_schedule) { fprintf(stderr, "%s: scaling lists need the ticket schedule (not KVZ_HIP_SCHED=wave)\n", who); return false; }
  return true;
}

// One plane of a row: the factors of list `list` (0-2 intra Y, U, V; 3-5 inter Y, U, V) at qp % 6 = r, KVZ_LIST_PLANE words laid out as list_index addresses them.
// scalinglist.c:289-342: the forward factor (kvz_g_quant_scales[r] << 4) / entry -- the division the device does not have --, the inverse one
// kvz_g_inv_quant_scales[r] * entry; :375-391: the DC term in place of entry 0 for coefficient (0, 0) at 16x16 and 32x32.  The 32x32 size has two lists, intra
// and inter: the reference reads list 3 there through its alias quant_coeff[3][3] = quant_coeff[3][1] (scalinglist.c:104); no chroma block is that large, its
// planes hold the list of their kind.  set == nullptr: the flat list.
inline void scaling_list_plane(const kvz_hip_scaling_lists *set, int r, int list, uint32_t *plane)
{
  auto word = [&](int entry) { return (uint32_t)((quant_scale(r) << 4) / entry) | (uint32_t)(inv_quant_scale(r) * entry) << 16; };
  for (int i = 0; i < KVZ_LIST_PLANE; i++) plane[i] = 0;
  for (int size = 0; size < 4; size++) {
    const int l = size == 3 ? (list >= 3 ? 1 : 0) : list, at = list_index(size + 2, size < 2 ? 0 : 1);  // where the size's entries start (from 16x16 on element 0 has the DC term, element 1 entry 0)
    for (int i = 0; i < (size == 0 ? 16 : 64); i++) plane[at + i] = word(set ? set->coeff[size][l][i] : 16);
    if (size >= 2) plane[at + 64] = word(set && set->dc[size][l] ? set->dc[size][l] : 16);
  }
}
// The six rows (qp % 6 = 0 .. 5) of one set, or of the flat list (set == nullptr), for the all-intra pass: rows[6][KVZ_LIST_ROW], a row = the planes of the intra
// lists 0, 1, 2 (Y, U, V; list 0 at 32x32).
inline void scaling_list_rows(const kvz_hip_scaling_lists *set, uint32_t *rows)
{
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 3; c++) scaling_list_plane(set, r, c, rows + r * KVZ_LIST_ROW + c * KVZ_LIST_PLANE);
}
// ... and for the inter pass (kvz_inter_ctu_pix.inc quantize_tu): rows[6][KVZ_LIST_ROW_INTER], a row = the planes of all six lists, Y, U, V intra -- the intra CUs
// of a B slice -- then Y, U, V inter: a block reads plane (intra CU ? 0 : 3) + {Y 0, U 1, V 2} (quant-generic.c:59, :312), list_plane_of.  The one statement of
// the layout: the kernel, the library's staging (kvz_dev.hpp) and the host simulation all go through this function and list_plane_of.
inline void scaling_list_rows_inter(const kvz_hip_scaling_lists *set, uint32_t *rows)
{
  for (int r = 0; r < 6; r++)
    for (int list = 0; list < 6; list++) scaling_list_plane(set, r, list, rows + r * KVZ_LIST_ROW_INTER + list * KVZ_LIST_PLANE);
}
// the row of a picture's set (0xffff: the flat list, which follows the n_sets sets) at a QP -- luma: the picture's, chroma: scaled_qp(2, qp, 0) -- in a table of six
// rows per set; up to 6 * 65536 rows: an index of its own, not half a word
inline uint32_t scaling_list_row(int set, int n_sets, int qp_of_plane) { return (uint32_t)(set == 0xffff ? n_sets : set) * 6u + (uint32_t)(qp_of_plane % 6); }
// a picture's rows in a table of n_sets sets followed by the flat list: its luma row | its chroma row << 16 (set 0xffff: flat)
inline uint32_t scaling_list_rows_of_picture(int set, int n_sets, int qp)
{
  const int k = set == 0xffff ? n_sets : set;
  return (uint32_t)(k * 6 + qp % 6) | (uint32_t)(k * 6 + scaled_qp(2, qp, 0) % 6) << 16;
}

}  // namespace kvz
