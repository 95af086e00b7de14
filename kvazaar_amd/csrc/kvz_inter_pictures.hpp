// kvz_inter_pictures.hpp -- which per-picture (QP, POC) tables (include/kvz_hip_types.h kvz_hip_inter_pictures) the inter entry points accept, and how the QPs of a
// launch become rows: the checks kvz_hip_dev_inter_ctu_pass_pictures, kvz_hip_dev_loop_filters_inter_pictures and kvz_hip_dev_entropy_code_inter_pictures make before
// they queue anything.  Host code without a HIP dependency (kvz_picture_models.hpp is its pattern): kvz_dev.hpp calls it, and the host simulation (tests/hostsim)
// compiles the same text.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "../../include/kvz_hip_types.h"

namespace kvz {

// a host array of n picture QPs (the loop filters take it bare)
inline bool inter_picture_qps_known(const int32_t *qp, int n_pictures, const char *who)
{
  if (!qp) { fprintf(stderr, "%s: the per-picture QP array is NULL\n", who); return false; }
  for (int i = 0; i < n_pictures; i++)
    if (qp[i] < 0 || qp[i] > 51) { fprintf(stderr, "%s: picture %d has QP %d outside 0..51\n", who, i, qp[i]); return false; }
  return true;
}

// Is this a table a launch of n_pictures pictures can run?  Everything an entry point refuses is refused here, before anything is queued.
inline bool inter_pictures_known(const kvz_hip_inter_pictures *ip, int n_pictures, const char *who)
{
  if (!ip || ip->struct_size != sizeof(kvz_hip_inter_pictures)) {
    fprintf(stderr, "%s: kvz_hip_inter_pictures.struct_size %u is not this library's %zu (zero the struct, set struct_size = sizeof, build against the library's headers)\n", who, ip ? ip->struct_size : 0u, sizeof(kvz_hip_inter_pictures));
    return false;
  }
  if (ip->n_pictures != n_pictures) { fprintf(stderr, "%s: kvz_hip_inter_pictures.n_pictures %d is not the call's %d\n", who, ip->n_pictures, n_pictures); return false; }
  if (!ip->qp || !ip->poc) { fprintf(stderr, "%s: kvz_hip_inter_pictures needs a QP and a POC per picture (%s is NULL)\n", who, !ip->qp ? "qp" : "poc"); return false; }
  if (!inter_picture_qps_known(ip->qp, n_pictures, who)) return false;
  for (int i = 0; i < n_pictures; i++)
    if (ip->poc[i] < 1) { fprintf(stderr, "%s: picture %d has POC %d below 1\n", who, i, ip->poc[i]); return false; }
  return true;
}

// The distinct QPs of a launch in ascending order: a launch keeps one row of everything that follows from the QP (cost model, context states, SAO prices) per distinct
// QP, at most 52.  row_of_qp[q]: the row of QP q, -1 where no picture has it.  Returns the number of rows.
inline int inter_qp_rows(const int32_t *qp, int n_pictures, int row_of_qp[52], int qp_of_row[52])
{
  for (int q = 0; q < 52; q++) row_of_qp[q] = -1;
  for (int i = 0; i < n_pictures; i++) row_of_qp[qp[i]] = 0;
  int rows = 0;
  for (int q = 0; q < 52; q++) if (row_of_qp[q] == 0) { qp_of_row[rows] = q; row_of_qp[q] = rows++; }
  return rows;
}

// rdo.c:311-340 kvz_get_coeff_cost: coefficients are priced with the residual coder's contexts unless the picture QP lies below cfg.fast_residual_cost_limit and below
// MAX_FAST_COEFF_COST_QP
inline bool inter_qp_prices_with_cabac(int qp, int fast_residual_cost) { return !(qp < fast_residual_cost && qp < 50); }
}  // namespace kvz
