// kvz_joint.hpp -- batches of different picture sizes in ONE persistent launch of the all-intra CTU pass (kvz_hip_batch_group): the records a workgroup reads for the
// picture it drew, the two ticket lists and the hand-off error tag (a batch on its own uses both as well), what a group and a joint launch are refused for, and how a timed-out hand-off reaches every batch of the group.
// No HIP dependency: kvz_ctu_kernels.hpp reads the records on the device, kvz_batch.hpp lays them out, and the host simulation (tests/hostsim/hostsim_joint.cpp)
// compiles the same text.
//
// A joint launch numbers the pictures of its batches across the group, batch after batch, and keeps the item word of the ticket schedule: picture << 16 | y << 8 | x.
// Everything else a CTU needs hangs off its picture: the geometry and buffers of the picture's batch, the picture's index inside that batch, the batch's hand-off
// flags and the pass number they are compared with (every batch counts its own passes: a joint launch is pass epoch + 1 of each of its batches, so solo passes
// between joint ones need no care), and the batch's model table.
//
// Invariant of both lists (joint_ticket_lists), checked by tests/test_joint_pass_sim.py: a CTU's left neighbour, its above-right neighbour -- the above one at the
// right edge of the picture, as ticket_loop clamps it -- and, in the list without WPP, the last CTU of the row above all hold LOWER tickets than the CTU itself.
// That is all the in-order ticket protocol needs to be free of deadlock for any number of resident workgroups (kvz_ctu_kernels.hpp): geometry plays no part in it.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "kvz_ctu.hpp"
#include "kvz_picture_models.hpp"

namespace kvz {

// One per batch of the group, in device memory during a launch; uniform per workgroup and constant during the launch.
struct JointBatch {
  CtuFrames F;           // the batch's geometry and buffers
  CtuModelTable models;  // its model table (rows and the row of every picture of the batch)
  unsigned *done;        // its hand-off flags [n_frames * wc * hc] ...
  unsigned epoch;        // ... and the number of this pass on the batch
  int index;             // the batch's place in the group
};
static_assert(sizeof(JointBatch) % 4 == 0, "fetched word by word");
struct JointTable {
  const uint32_t *batch_of_picture = nullptr;  // [pictures of the group]: batch << 16 | the picture's index inside its batch
  const JointBatch *batches = nullptr;
};
// the record of group picture `picture`, and its index inside the record's batch
KVZ_HD const JointBatch *joint_record(const JointTable &t, uint32_t word) { return t.batches + (word >> 16); }
KVZ_HD int joint_frame(uint32_t word) { return (int)(word & 0xffffu); }

struct JointGeometry { int wc, hc, n_frames; };

// batch << 16 | frame for every picture of the group, batch after batch
inline std::vector<uint32_t> joint_pictures(const JointGeometry *g, int n)
{
  std::vector<uint32_t> words;
  for (int b = 0; b < n; b++)
    for (int f = 0; f < g[b].n_frames; f++) words.push_back((uint32_t)b << 16 | (uint32_t)f);
  return words;
}

// The hand-off error tag: what the first CTU to give up a wait leaves in the error word (kvz_ctu_kernels.hpp wait_done, under bit 31) -- the CTU it waited FOR, as in
// the item word but with the picture modulo 8192, and which neighbour of its own that is.
enum : unsigned { KVZ_WAIT_LEFT = 0u, KVZ_WAIT_ABOVE_RIGHT = 0x20000000u, KVZ_WAIT_ROW_END = 0x40000000u };
#define KVZ_HANDOFF_TAG(neighbour, picture, y, x) ((neighbour) | (((unsigned)(picture) << 16 | (unsigned)(y) << 8 | (unsigned)(x)) & 0x1fffffffu))  // (a macro: ticket_loop's code stays what it was, to the order of its instructions)
struct HandoffTag { unsigned x, y, picture; const char *neighbour; };
inline HandoffTag handoff_tag_read(unsigned err) { return { err & 0xffu, (err >> 8) & 0xffu, (err >> 16) & 0x1fffu, (err & KVZ_WAIT_ABOVE_RIGHT) ? "its above-right neighbour" : ((err & KVZ_WAIT_ROW_END) ? "the end of the row above" : "its left neighbour") }; }

// The ticket lists of a group -- and of a batch on its own, a group of one.  wpp: every picture's CTUs in ascending x + 2y, all pictures of all batches interleaved (one anti-diagonal of everybody, then the next: a small
// picture's CTUs sit among the first diagonals of the large ones).  raster: CTU i of every picture in raster order of its own grid, then CTU i + 1 of every picture.
inline void joint_ticket_lists(const JointGeometry *g, int n, std::vector<uint32_t> *wpp, std::vector<uint32_t> *raster)
{
  wpp->clear(); raster->clear();
  int waves = 0, most = 0;
  for (int b = 0; b < n; b++) {
    if ((g[b].wc - 1) + 2 * (g[b].hc - 1) + 1 > waves) waves = (g[b].wc - 1) + 2 * (g[b].hc - 1) + 1;
    if (g[b].wc * g[b].hc > most) most = g[b].wc * g[b].hc;
  }
  for (int wave = 0; wave < waves; wave++) {
    uint32_t picture = 0;
    for (int b = 0; b < n; b++)
      for (int f = 0; f < g[b].n_frames; f++, picture++)
        for (int y = 0; y < g[b].hc; y++) {
          const int x = wave - 2 * y;
          if (x >= 0 && x < g[b].wc) wpp->push_back(picture << 16 | (uint32_t)y << 8 | (uint32_t)x);
        }
  }
  for (int i = 0; i < most; i++) {
    uint32_t picture = 0;
    for (int b = 0; b < n; b++)
      for (int f = 0; f < g[b].n_frames; f++, picture++)
        if (i < g[b].wc * g[b].hc) raster->push_back(picture << 16 | (uint32_t)(i / g[b].wc) << 8 | (uint32_t)(i % g[b].wc));
  }
}

// What a group is made of, as far as the checks go
struct JointBatchInfo {
  const void *batch;  // identity
  int device, ticket_schedule, n_frames, has_lists, failed;
};
// kvz_hip_batch_group_create: n >= 1 distinct batches of one device under the ticket schedule, fewer than 65 536 pictures in all
inline bool joint_group_known(const JointBatchInfo *b, int n, const char *who)
{
  if (n < 1 || !b) { fprintf(stderr, "%s: a group needs at least one batch (n %d)\n", who, n); return false; }
  long pictures = 0;
  for (int i = 0; i < n; i++) {
    if (!b[i].batch) { fprintf(stderr, "%s: batch %d is NULL\n", who, i); return false; }
    for (int k = 0; k < i; k++) if (b[k].batch == b[i].batch) { fprintf(stderr, "%s: batch %d is batch %d again (a picture would be searched twice in one launch)\n", who, i, k); return false; }
    if (b[i].device != b[0].device) { fprintf(stderr, "%s: batch %d lives on device %d, batch 0 on device %d (one launch runs on one device)\n", who, i, b[i].device, b[0].device); return false; }
    if (!b[i].ticket_schedule) { fprintf(stderr, "%s: batch %d does not run the ticket schedule (KVZ_HIP_SCHED=wave, or a CTU grid beyond 255 a side)\n", who, i); return false; }
    pictures += b[i].n_frames;
  }
  if (pictures >= 65536) { fprintf(stderr, "%s: %ld pictures in all; the ticket word numbers fewer than 65536\n", who, pictures); return false; }
  return true;
}
// kvz_hip_batch_group_intra_frames: everything the joint launch refuses, before anything is queued on any batch.  One kernel build serves the launch, so the tables
// agree on what picks the build and the list (search_32x32, no_wpp); coeff_cabac and signhide are run-time switches of the build that has them.
inline bool joint_launch_known(const JointBatchInfo *b, int n, const kvz_hip_picture_models *const *models, const char *who)
{
  if (!models) { fprintf(stderr, "%s: no model tables\n", who); return false; }
  for (int i = 0; i < n; i++) {
    if (b[i].failed) { fprintf(stderr, "%s: batch %d is invalid since a hand-off wait timed out: kvz_hip_batch_reset it first\n", who, i); return false; }
    if (!picture_models_known(models[i], b[i].n_frames, b[i].ticket_schedule != 0, who)) { fprintf(stderr, "%s: ... the table of batch %d\n", who, i); return false; }
    const kvz_hip_intra_cost_model &m = models[i]->models[0], &m0 = models[0]->models[0];
    if (m.rdoq || m.search_nxn) { fprintf(stderr, "%s: the table of batch %d has rdoq / search_nxn: that kernel is not part of joint launches\n", who, i); return false; }
    if (b[i].has_lists) { fprintf(stderr, "%s: batch %d has scaling lists: not part of joint launches\n", who, i); return false; }
    if (!m.search_32x32 != !m0.search_32x32 || !m.no_wpp != !m0.no_wpp) {
      fprintf(stderr, "%s: the tables of batch %d and batch 0 disagree in search_32x32 / no_wpp (they pick the one kernel build and the one ticket list of the launch)\n", who, i);
      return false;
    }
  }
  return true;
}

// A hand-off wait that timed out inside a joint pass poisons the launch: tickets are only drained from then on, so NO batch of the group has results.  err: the three
// words the pass leaves (kvz_ctu_kernels.hpp wait_done: the CTU waited FOR, its flag, the tickets drawn).  Marks every batch failed and says which batch the CTU
// belongs to; returns that batch's index (-1: the tag's 13 picture bits do not name one picture of this group), or -2 when the word is clear and nothing was marked.
inline int joint_error_fan_out(const unsigned err[3], const uint32_t *batch_of_picture, unsigned n_pictures, int n_batches, int *failed, char *msg, size_t msg_len)
{
  if (msg && msg_len) msg[0] = 0;
  if (!err[0]) return -2;
  for (int i = 0; i < n_batches; i++) failed[i] = 1;
  const HandoffTag tag = handoff_tag_read(err[0]);
  const unsigned picture = tag.picture;
  const bool named = n_pictures <= 0x2000u && picture < n_pictures;
  const int batch = named ? (int)(batch_of_picture[picture] >> 16) : -1;
  if (msg && msg_len)
    snprintf(msg, msg_len, "a CTU hand-off wait timed out inside a joint pass (KVZ_HIP_WAIT_MS to raise the bound) -- the results of ALL %d batches of the group are invalid "
             "[first to give up waited for CTU x %u y %u of picture %d of batch %d (group picture %u%s; %s); that CTU's flag read at the memory side then: %u; tickets drawn then: %u]",
             n_batches, tag.x, tag.y, named ? joint_frame(batch_of_picture[picture]) : -1, batch, picture, named ? "" : " modulo 8192",
             tag.neighbour, err[1], err[2]);
  return batch;
}

}  // namespace kvz
