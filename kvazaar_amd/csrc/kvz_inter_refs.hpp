// kvz_inter_refs.hpp -- reference picture lists of P pictures (include/kvz_hip_types.h kvz_hip_inter_refs; the kvz_hip_dev_*_refs entry points): the scaling of a
// motion vector by POC distances (inter.c:1078-1103 get_scaled_mv / apply_mv_scaling_pocs), stated ONCE for the inter CTU pass (kvz_inter_ctu_cand.inc), the
// entropy coder (kvz_entropy.hpp mv_candidates) and the host simulation; the record a picture's list travels in; and what the entry points refuse of a
// kvz_hip_inter_refs before anything is queued.
// The reference divides: scale = clip(-4096, 4095, (tb * ((0x4000 + |td| / 2) / td) + 32) >> 6) with tb, td clipped to -128 .. 127.  There is no integer division
// in hardware, and tb and td follow from POCs the HOST knows: it lays the scale of every pair a picture can meet beside the picture's list (inter_refs_record), the
// kernels multiply (mv_scale).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "../../include/kvz_hip_types.h"
#include "kvz_ops.hpp"

namespace kvz {

#define KVZ_MV_SCALE_NONE 256  /* (256 * mv + 127 + (mv < 0)) >> 8 == mv for every int16 mv: the scale of "not scaled" */

// get_scaled_mv (inter.c:1078-1082) of one component
KVZ_HD int mv_scale(int mv, int scale)
{
  const int scaled = scale * mv;  // |scale| <= 4096, |mv| <= 32768: 28 bits
  const int v = (scaled + 127 + (scaled < 0)) >> 8;
  return v < -32768 ? -32768 : (v > 32767 ? 32767 : v);
}
// ... of a vector packed x | y << 16
KVZ_HD uint32_t mv_scale_packed(uint32_t mv, int scale)
{
  if (scale == KVZ_MV_SCALE_NONE) return mv;
  const int x = mv_scale((int)(int16_t)(mv & 0xffffu), scale), y = mv_scale((int)(int16_t)(mv >> 16), scale);
  return (uint32_t)(uint16_t)x | (uint32_t)(uint16_t)y << 16;
}

// apply_mv_scaling_pocs (inter.c:1084-1103): the scale for diff_current = POC - POC of the picture referred to, diff_neighbor = the same of the vector's owner.
// Equal distances leave the vector alone; so does a zero diff_neighbor (search_inter.c:1221 -- inter.c would divide by it; no valid list produces it)
inline int mv_scale_of_distances(long long diff_current, long long diff_neighbor)
{
  if (diff_current == diff_neighbor || diff_neighbor == 0) return KVZ_MV_SCALE_NONE;
  const int tb = (int)(diff_current < -128 ? -128 : (diff_current > 127 ? 127 : diff_current)), td = (int)(diff_neighbor < -128 ? -128 : (diff_neighbor > 127 ? 127 : diff_neighbor));
  const int tx = (0x4000 + ((td < 0 ? -td : td) >> 1)) / td;
  const int scale = (tb * tx + 32) >> 6;
  return scale < -4096 ? -4096 : (scale > 4095 ? 4095 : scale);
}

// What a picture's list is on the device: the pool frames of its entries and the scales of every vector it can meet, [target reference index][...]:
//  spatial[r][c]   a neighbour's vector that refers to entry c, for a predictor of entry r (inter.c:1105-1121)
//  temporal[r][j]  a vector of the co-located picture (entry 0) whose own reference index is j, for entry r (inter.c:1171-1181)
//  start[r][j]     a vector of entry r's co-located CU whose own reference index is j, as the start of the search of entry r (search_inter.c:1320-1332)
struct InterRefsRecord {
  int32_t n_refs;
  int32_t pool_frame[KVZ_HIP_MAX_REFS];
  int16_t spatial[KVZ_HIP_MAX_REFS][4], temporal[KVZ_HIP_MAX_REFS][4], start[KVZ_HIP_MAX_REFS][4];
};
static_assert(sizeof(InterRefsRecord) == 116, "the record is copied as 29 words");

inline InterRefsRecord inter_refs_record(const kvz_hip_inter_refs *refs, int picture, int poc)
{
  InterRefsRecord rec;
  rec.n_refs = refs->n_refs[picture];
  long long P[KVZ_HIP_MAX_REFS] = { 0, 0, 0, 0 };
  for (int r = 0; r < KVZ_HIP_MAX_REFS; r++) {
    rec.pool_frame[r] = r < rec.n_refs ? refs->ref_frame[picture * KVZ_HIP_MAX_REFS + r] : 0;
    P[r] = refs->frame_poc[rec.pool_frame[r]];
  }
  for (int r = 0; r < KVZ_HIP_MAX_REFS; r++)
    for (int k = 0; k < 4; k++) {
      const bool there = r < rec.n_refs;
      rec.spatial[r][k] = (int16_t)(there && k < rec.n_refs ? mv_scale_of_distances(poc - P[r], poc - P[k]) : KVZ_MV_SCALE_NONE);
      rec.temporal[r][k] = (int16_t)(there ? mv_scale_of_distances(poc - P[r], P[0] - refs->frame_ref_poc[rec.pool_frame[0] * 4 + k]) : KVZ_MV_SCALE_NONE);
      rec.start[r][k] = (int16_t)(there ? mv_scale_of_distances(poc - P[r], P[r] - refs->frame_ref_poc[rec.pool_frame[r] * 4 + k]) : KVZ_MV_SCALE_NONE);
    }
  return rec;
}

// Is this a table a launch of n_pictures P pictures can run?  poc: the POC of every picture (kvz_hip_inter_pictures::poc), or NULL where the entry point has none
// (the loop filters: the order of the POCs is then not checked).  Everything an entry point refuses of the struct is refused here, before anything is queued.
inline bool inter_refs_known(const kvz_hip_inter_refs *refs, int n_pictures, const int32_t *poc, const char *who)
{
  if (!refs || refs->struct_size != sizeof(kvz_hip_inter_refs)) {
    fprintf(stderr, "%s: kvz_hip_inter_refs.struct_size %u is not this library's %zu (zero the struct, set struct_size = sizeof, build against the library's headers)\n", who, refs ? refs->struct_size : 0u, sizeof(kvz_hip_inter_refs));
    return false;
  }
  if (refs->n_pictures != n_pictures) { fprintf(stderr, "%s: kvz_hip_inter_refs.n_pictures %d is not the call's %d\n", who, refs->n_pictures, n_pictures); return false; }
  if (!refs->frame_poc || !refs->frame_ref_poc || !refs->n_refs || !refs->ref_frame) { fprintf(stderr, "%s: kvz_hip_inter_refs needs frame_poc, frame_ref_poc, n_refs and ref_frame (one is NULL)\n", who); return false; }
  if (refs->n_frames < 1) { fprintf(stderr, "%s: kvz_hip_inter_refs.n_frames %d: the pool is empty\n", who, refs->n_frames); return false; }
  for (int i = 0; i < n_pictures; i++) {
    const int n = refs->n_refs[i];
    if (n < 1 || n > KVZ_HIP_MAX_REFS) { fprintf(stderr, "%s: picture %d has a list of %d references, outside 1..%d\n", who, i, n, KVZ_HIP_MAX_REFS); return false; }
    for (int r = 0; r < n; r++) {
      const int f = refs->ref_frame[i * KVZ_HIP_MAX_REFS + r];
      if (f < 0 || f >= refs->n_frames) { fprintf(stderr, "%s: picture %d, reference %d: frame %d is outside the pool of %d\n", who, i, r, f, refs->n_frames); return false; }
      if (poc && refs->frame_poc[f] >= poc[i]) { fprintf(stderr, "%s: picture %d (POC %d), reference %d: frame %d has POC %d, which is not below the picture's\n", who, i, poc[i], r, f, refs->frame_poc[f]); return false; }
      for (int q = 0; q < r; q++)
        if (refs->frame_poc[refs->ref_frame[i * KVZ_HIP_MAX_REFS + q]] == refs->frame_poc[f]) { fprintf(stderr, "%s: picture %d: references %d and %d both have POC %d\n", who, i, q, r, refs->frame_poc[f]); return false; }
    }
  }
  return true;
}

}  // namespace kvz
