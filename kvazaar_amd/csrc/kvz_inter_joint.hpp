// kvz_inter_joint.hpp -- B pictures of different sizes in ONE persistent launch of the inter CTU pass (kvz_hip_dev_inter_ctu_pass_groups, include/kvz_hip_dev.h): what
// a joint launch is refused for, its two ticket lists and the table a workgroup reads for the picture it drew.  Host code without a HIP dependency, on the pattern
// of kvz_joint.hpp (the all-intra pass's joint launches) and kvz_inter_pictures.hpp: kvz_dev.hpp calls it, and the host simulation
// (tests/hostsim/hostsim_inter_joint.cpp) compiles the same text.
//
// A joint launch numbers its pictures across the groups, group after group, and keeps the item word of the ticket schedule: picture << 16 | y << 8 | x.  Everything
// else a CTU needs hangs off its picture (kvz_inter_ctu.hpp InterJointPicture / InterJointGroup): the picture's group -- geometry, the six buffers, the group's slice
// of the launch-wide context scratch and its first index into the launch-wide `done` flags --, its index inside the group, its InterModel row and its POC.
// `done`, the context scratch and the levels are indexed by (group's CTU base) + (picture in group) x (group's CTUs) + (y x wc + x).
//
// Invariant of both lists (inter_joint_ticket_lists), checked by tests/test_inter_joint_sim.py: a CTU's left neighbour, its above-right neighbour -- the above one at
// the right edge of the picture, as the kernel's wait clamps it -- and, in the list without WPP, the last CTU of the row above all hold LOWER tickets than the CTU
// itself.  That is all the in-order ticket protocol needs to be free of deadlock for any number of resident workgroups: geometry plays no part in it.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "kvz_inter_host.hpp"

namespace kvz {

struct InterJointGeometry { int wc, hc, n_pictures; };

// The ticket lists of a joint launch -- the shape of joint_ticket_lists (kvz_joint.hpp).  wpp: every picture's CTUs in ascending x + 2y, all pictures of all groups
// interleaved (one anti-diagonal of everybody, then the next; inside a diagonal row after row, picture after picture, as inter_ticket_items has it: a launch of one
// group gets exactly that function's list).  raster: CTU i of every picture in raster order of its own grid, then CTU i + 1 of every picture.
inline void inter_joint_ticket_lists(const InterJointGeometry *g, int n, std::vector<uint32_t> *wpp, std::vector<uint32_t> *raster)
{
  int waves = 0, most = 0, rows = 0;
  for (int b = 0; b < n; b++) {
    if ((g[b].wc - 1) + 2 * (g[b].hc - 1) + 1 > waves) waves = (g[b].wc - 1) + 2 * (g[b].hc - 1) + 1;
    if (g[b].wc * g[b].hc > most) most = g[b].wc * g[b].hc;
    if (g[b].hc > rows) rows = g[b].hc;
  }
  if (wpp) {
    wpp->clear();
    for (int wave = 0; wave < waves; wave++)
      for (int y = 0; y < rows; y++) {
        const int x = wave - 2 * y;
        if (x < 0) break;
        uint32_t picture = 0;
        for (int b = 0; b < n; picture += (uint32_t)g[b].n_pictures, b++) {
          if (y >= g[b].hc || x >= g[b].wc) continue;
          for (int f = 0; f < g[b].n_pictures; f++) wpp->push_back((picture + (uint32_t)f) << 16 | (uint32_t)y << 8 | (uint32_t)x);
        }
      }
  }
  if (raster) {
    raster->clear();
    for (int i = 0; i < most; i++) {
      uint32_t picture = 0;
      for (int b = 0; b < n; picture += (uint32_t)g[b].n_pictures, b++) {
        if (i >= g[b].wc * g[b].hc) continue;
        for (int f = 0; f < g[b].n_pictures; f++) raster->push_back((picture + (uint32_t)f) << 16 | (uint32_t)(i / g[b].wc) << 8 | (uint32_t)(i % g[b].wc));
      }
    }
  }
}

// Everything kvz_hip_dev_inter_ctu_pass_groups refuses, before anything is queued: true = the launch can run
inline bool inter_joint_known(const kvz_hip_inter_group *groups, int n_groups, const kvz_hip_inter_params *p, const char *who)
{
  kvz_hip_inter_params full;
  if (!inter_params_full(p, &full, who)) return false;
  p = &full;
  if (n_groups < 1 || !groups) { fprintf(stderr, "%s: a joint launch needs at least one group (n_groups %d)\n", who, n_groups); return false; }
  if (p->ref_width || p->ref_height || p->tile_x || p->tile_y) {
    fprintf(stderr, "%s: ref_width / ref_height / tile_x / tile_y are %d / %d / %d / %d: tiles are not part of joint launches\n", who, p->ref_width, p->ref_height, p->tile_x, p->tile_y);
    return false;
  }
  if (p->fme_level < 0 || p->fme_level > 4 || p->pu_depth_inter_max < 1 || p->pu_depth_inter_max > 3 || p->fast_residual_cost < 0 || p->fast_residual_cost > 51) {
    fprintf(stderr, "%s: unsupported parameters (fme_level %d, pu_depth_inter_max %d, fast_residual_cost %d)\n", who, p->fme_level, p->pu_depth_inter_max, p->fast_residual_cost);
    return false;
  }
  if (!inter_me_known(p, "a joint launch", who)) return false;
  long pictures = 0, ctus = 0;
  for (int i = 0; i < n_groups; i++) {
    const kvz_hip_inter_group &g = groups[i];
    if (g.struct_size != sizeof(kvz_hip_inter_group)) {
      fprintf(stderr, "%s: group %d: kvz_hip_inter_group.struct_size %u is not this library's %zu (zero the struct, set struct_size = sizeof, build against the library's headers)\n", who, i, g.struct_size, sizeof(kvz_hip_inter_group));
      return false;
    }
    if (g.n_pictures < 1 || inter_pass_geometry_refused(g.width, g.height, g.n_pictures, 0, 0, 0, 0)) {
      fprintf(stderr, "%s: group %d: bad geometry (%d pictures of %dx%d; multiples of 8, at most 255 CTUs a side, fewer than 2^23 4x4 units)\n", who, i, g.n_pictures, g.width, g.height);
      return false;
    }
    const char *null = !g.src ? "src" : !g.ref ? "ref" : !g.ref_cu ? "ref_cu" : !g.rec ? "rec" : !g.cu ? "cu" : nullptr;
    if (null) { fprintf(stderr, "%s: group %d: %s is NULL (only coeff may be)\n", who, i, null); return false; }
    if (g.pictures) {
      if (!inter_pictures_known(g.pictures, g.n_pictures, who)) { fprintf(stderr, "%s: ... the table of group %d\n", who, i); return false; }
    } else if (p->qp < 0 || p->qp > 51 || p->poc < 1) {
      fprintf(stderr, "%s: group %d has no table and params holds QP %d (0..51) / POC %d (>= 1)\n", who, i, p->qp, p->poc);
      return false;
    }
    for (int k = 0; k < i; k++)
      if (groups[k].rec == g.rec || groups[k].cu == g.cu) {
        fprintf(stderr, "%s: group %d has the %s buffer of group %d (two pictures would be written to one place)\n", who, i, groups[k].rec == g.rec ? "rec" : "cu", k);
        return false;
      }
    pictures += g.n_pictures;
    ctus += (long)((g.width + 63) / 64) * ((g.height + 63) / 64) * g.n_pictures;
  }
  if (pictures >= 65536) { fprintf(stderr, "%s: %ld pictures in all; the ticket word numbers fewer than 65536\n", who, pictures); return false; }
  if (ctus >= (1l << 31)) { fprintf(stderr, "%s: %ld CTUs in all; the hand-off flags are indexed with 32 bits\n", who, ctus); return false; }
  return true;
}

// The table of a joint launch as the device holds it (InterFrames::pictures of the JOINT builds): [pictures] InterJointPicture, [groups] InterJointGroup, then one
// InterModel row per distinct QP of the launch.  init_row(m, qp): the launch's model at that QP -- made WITHOUT a picture size (rows are shared across groups: the
// kernel takes ref_w / ref_h from the group record).  ctx: the launch-wide context scratch (a device pointer; only its address enters the image).  The caller copies
// `image` to the device as it is.
struct InterJointTable {
  std::vector<uint64_t> image;
  std::vector<InterJointGeometry> geometry;
  std::vector<long> ctu_base;  // [groups]
  long ctus = 0;               // of the launch
  int n_pictures = 0, n_rows = 0;
  size_t rows_at = 0;
  bool any_cabac = false;
  size_t bytes() const { return image.size() * sizeof(uint64_t); }
  const InterModel *model_of_picture(const void *base, int picture) const { return (const InterModel *)((const uint8_t *)base + ((const InterJointPicture *)image.data())[picture].model_at); }
};
template <class InitRow> inline InterJointTable inter_joint_table(const kvz_hip_inter_group *groups, int n_groups, const kvz_hip_inter_params *p, ICtx *ctx, const InitRow &init_row)
{
  static_assert(sizeof(InterJointPicture) == 16 && sizeof(InterJointGroup) % 8 == 0 && alignof(InterJointGroup) <= 8, "records and rows share a buffer of 8-byte words");
  InterJointTable t;
  std::vector<int32_t> qp, poc;
  for (int b = 0; b < n_groups; b++) {
    const kvz_hip_inter_group &g = groups[b];
    t.geometry.push_back(InterJointGeometry{ (g.width + 63) / 64, (g.height + 63) / 64, g.n_pictures });
    for (int f = 0; f < g.n_pictures; f++) { qp.push_back(g.pictures ? g.pictures->qp[f] : p->qp); poc.push_back(g.pictures ? g.pictures->poc[f] : p->poc); }
  }
  t.n_pictures = (int)qp.size();
  int row_of_qp[52], qp_of_row[52];
  t.n_rows = inter_qp_rows(qp.data(), t.n_pictures, row_of_qp, qp_of_row);
  const size_t groups_at = (size_t)t.n_pictures * sizeof(InterJointPicture);
  t.rows_at = groups_at + (size_t)n_groups * sizeof(InterJointGroup);
  t.image.assign((t.rows_at + (size_t)t.n_rows * sizeof(InterModel)) / sizeof(uint64_t), 0);
  uint8_t *base = (uint8_t *)t.image.data();
  for (int r = 0; r < t.n_rows; r++) {
    InterModel *m = (InterModel *)(base + t.rows_at) + r;
    init_row(m, qp_of_row[r]);
    t.any_cabac = t.any_cabac || m->coeff_cabac;
  }
  int picture = 0;
  for (int b = 0; b < n_groups; b++) {
    const kvz_hip_inter_group &g = groups[b];
    const InterJointGeometry &geo = t.geometry[b];
    InterJointGroup *jg = (InterJointGroup *)(base + groups_at) + b;
    jg->W = g.width; jg->H = g.height; jg->wc = geo.wc; jg->hc = geo.hc;
    jg->frame_px = (long)g.width * g.height * 3 / 2; jg->cells = (long)(g.width / 4) * (g.height / 4);
    jg->src = g.src; jg->ref = g.ref; jg->ref_cu = g.ref_cu; jg->rec = g.rec; jg->cu = g.cu; jg->coeff = g.coeff;
    jg->ctx_out = ctx + t.ctus; jg->ctu_base = t.ctus;
    t.ctu_base.push_back(t.ctus);
    for (int f = 0; f < g.n_pictures; f++, picture++)
      ((InterJointPicture *)base)[picture] = InterJointPicture{ (uint32_t)(groups_at + (size_t)b * sizeof(InterJointGroup)), (uint32_t)f,
                                                               (uint32_t)(t.rows_at + (size_t)row_of_qp[qp[picture]] * sizeof(InterModel)), poc[picture] };
    t.ctus += (long)geo.wc * geo.hc * g.n_pictures;
  }
  return t;
}

}  // namespace kvz
