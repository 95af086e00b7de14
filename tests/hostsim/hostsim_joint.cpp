// hostsim_joint.cpp -- TEST INFRASTRUCTURE (see hostsim.cpp; this unit includes hostsim_signhide.cpp whole: one library with everything of libkvz_hostsim_signhide.so
// plus the joint pass).  kvz_hip_batch_group_intra_frames on the host: the joint ticket list of the group (kvz_joint.hpp, the text the library builds it with) is walked
// in ticket order; for every item the record of the drawn picture's batch is found through the functions the device uses (joint_record / joint_frame), the waits of
// ticket_loop are checked instead of waited for -- a list that put a CTU before one of its dependencies ends the walk with -3 -- and CtuProgramT::run() runs on that
// record's frames with the picture's model from that record's table.  A record with a wrong offset, or a list in a wrong order, then gives wrong pictures on the CPU.
// tests/test_joint_pass_sim.py builds and uses it.
#include "hostsim_signhide.cpp"
#include "../../kvazaar_amd/csrc/kvz_joint.hpp"

namespace {
std::vector<kvz::JointGeometry> joint_geometry(int n, const int *widths, const int *heights, const int *n_frames)
{
  std::vector<kvz::JointGeometry> g;
  for (int i = 0; i < n; i++) g.push_back({ (widths[i] + 63) / 64, (heights[i] + 63) / 64, n_frames[i] });
  return g;
}
}  // namespace

// the two joint lists and the picture words of a group of n batches; every output holds sum(n_frames x CTUs) / sum(n_frames) words.  Returns the number of items
extern "C" long kvz_hostsim_joint_lists(int n, const int *widths, const int *heights, const int *n_frames, uint32_t *wpp, uint32_t *raster, uint32_t *pictures)
{
  const std::vector<kvz::JointGeometry> g = joint_geometry(n, widths, heights, n_frames);
  std::vector<uint32_t> a, b;
  kvz::joint_ticket_lists(g.data(), n, &a, &b);
  const std::vector<uint32_t> p = kvz::joint_pictures(g.data(), n);
  if (a.size() != b.size()) return -1;
  memcpy(wpp, a.data(), a.size() * sizeof(uint32_t));
  memcpy(raster, b.data(), b.size() * sizeof(uint32_t));
  memcpy(pictures, p.data(), p.size() * sizeof(uint32_t));
  return (long)a.size();
}

// what kvz_hip_batch_group_create checks: ids name the batches (equal ids: the same batch twice; 0: NULL).  0 accepted, -1 refused
extern "C" int kvz_hostsim_joint_group_check(int n, const uintptr_t *ids, const int *devices, const int *ticket_schedule, const int *n_frames)
{
  std::vector<kvz::JointBatchInfo> info;
  for (int i = 0; i < n; i++) info.push_back({ (const void *)ids[i], devices[i], ticket_schedule[i], n_frames[i], 0, 0 });
  return kvz::joint_group_known(n > 0 ? info.data() : nullptr, n, "kvz_hostsim_joint_group_check") ? 0 : -1;
}

// how the error words of a joint pass reach the batches (kvz_batch.hpp joint_check calls the same function): failed [n] is set for every batch when err[0] is set.
// Returns the batch the diagnostic names, -1 when it cannot name one, -2 for a clear word
extern "C" int kvz_hostsim_joint_fan_out(const unsigned *err, int n, const int *widths, const int *heights, const int *n_frames, int *failed, char *msg, size_t msg_len)
{
  const std::vector<kvz::JointGeometry> g = joint_geometry(n, widths, heights, n_frames);
  const std::vector<uint32_t> p = kvz::joint_pictures(g.data(), n);
  return kvz::joint_error_fan_out(err, p.data(), (unsigned)p.size(), n, failed, msg, msg_len);
}

// the hand-off error tag (kvz_joint.hpp): the word ticket_loop writes for a wait for CTU (x, y) of `picture`, `neighbour` of the waiting CTU (a KVZ_WAIT_* value), and
// in *read what both diagnostics read out of the error word that holds it
extern "C" unsigned kvz_hostsim_handoff_tag(unsigned neighbour, int picture, int y, int x, kvz::HandoffTag *read)
{
  const unsigned tag = KVZ_HANDOFF_TAG(neighbour, picture, y, x);
  *read = kvz::handoff_tag_read(0x80000000u | tag);
  return tag;
}

// what the entry points check of a launch before they ask for its build: signhide_known for every model of the table, scaling_lists_known for a batch with lists, and
// for a joint launch joint_launch_known on a group of this one batch.  0 accepted, -1 refused
extern "C" int kvz_hostsim_ctu_launch_check(const kvz_hip_picture_models *pm, int n_frames, int lists, int joint)
{
  const char *who = "kvz_hostsim_ctu_launch_check";
  for (int i = 0; i < pm->n_models; i++) if (!kvz::signhide_known(&pm->models[i], true, who)) return -1;
  if (!kvz::scaling_lists_known(pm, lists != 0, who)) return -1;
  const kvz::JointBatchInfo info{ pm, 0, 1, n_frames, lists, 0 };
  return !joint || kvz::joint_launch_known(&info, 1, &pm, who) ? 0 : -1;
}

// kvz_hip_batch_group_intra_frames on the host.  Per batch i: its table, geometry, and its buffers in the batch's layouts (pictures back to back).  has_lists / failed
// (may be null): the state of the batches the launch refuses.  Returns 0; -1 refused (nothing computed); -3 the list drew a CTU before one of its dependencies.
extern "C" int kvz_hostsim_joint_intra_frames(int n, const kvz_hip_picture_models *const *models, const int *widths, const int *heights, const int *n_frames,
                                              const uint8_t *const *src, uint8_t *const *rec, int16_t *const *coeff, uint8_t *const *cu_depth, uint8_t *const *cu_mode,
                                              double *const *ctu_cost, const int *has_lists, const int *failed)
{
  std::vector<kvz::JointBatchInfo> info;
  for (int i = 0; i < n; i++) info.push_back({ rec ? (const void *)rec[i] : nullptr, 0, 1, n_frames[i], has_lists ? has_lists[i] : 0, failed ? failed[i] : 0 });
  if (!kvz::joint_group_known(n > 0 ? info.data() : nullptr, n, "kvz_hostsim_joint_intra_frames")) return -1;
  if (!kvz::joint_launch_known(info.data(), n, models, "kvz_hostsim_joint_intra_frames")) return -1;
  const std::vector<kvz::JointGeometry> geo = joint_geometry(n, widths, heights, n_frames);
  std::vector<uint32_t> wpp, raster;
  kvz::joint_ticket_lists(geo.data(), n, &wpp, &raster);
  const std::vector<uint32_t> pictures = kvz::joint_pictures(geo.data(), n);
  // the records, as kvz_hip_batch_group_intra_frames lays them out (host pointers)
  std::vector<kvz::JointBatch> records((size_t)n);
  std::vector<HostModelTable> tables;
  tables.reserve((size_t)n);
  std::vector<HostFrames> frames;
  frames.reserve((size_t)n);
  std::vector<std::vector<unsigned>> done((size_t)n);
  for (int i = 0; i < n; i++) {
    tables.emplace_back(models[i]);
    frames.emplace_back(widths[i], heights[i], n_frames[i], src[i], rec[i], coeff[i], cu_depth[i], cu_mode[i], ctu_cost[i]);
    kvz::JointBatch &r = records[(size_t)i];
    memset(&r, 0, sizeof r);
    r.F = frames[(size_t)i].F;
    done[(size_t)i].assign((size_t)geo[i].wc * geo[i].hc * n_frames[i], 0);
    r.models = tables[(size_t)i].table; r.done = done[(size_t)i].data(); r.epoch = 7u + (unsigned)i; r.index = i;  // (every batch counts its own passes)
  }
  kvz::JointTable jt;
  jt.batch_of_picture = pictures.data(); jt.batches = records.data();
  const kvz_hip_intra_cost_model &m0 = models[0]->models[0];
  const std::vector<uint32_t> &items = m0.no_wpp ? raster : wpp;
  void *sh = frames[0].shared.data();
  int rc = 0;
  const int build = kvz::picture_models_build(models, n, false, true);  // ONE for the launch, as the library asks for it
  if (build == kvz::KVZ_CTU_BUILD_NONE) return -1;
  for (size_t t = 0; t < items.size() && rc == 0; t++) {
    const uint32_t item = items[t];
    const int picture = (int)(item >> 16), y = (int)((item >> 8) & 0xff), x = (int)(item & 0xff);
    const uint32_t word = jt.batch_of_picture[picture];
    const kvz::JointBatch *jb = kvz::joint_record(jt, word);
    const int frame = kvz::joint_frame(word);
    const kvz::CtuFrames &F = jb->F;
    const int ctus = F.wc * F.hc;
    unsigned *flags = jb->done + (long)frame * ctus;
    // ticket_loop's waits: on the host an unmet one is an error of the list
    if (x > 0 && flags[y * F.wc + x - 1] != jb->epoch) rc = -3;
    if (y > 0 && flags[(y - 1) * F.wc + (x + 1 < F.wc ? x + 1 : x)] != jb->epoch) rc = -3;
    if (m0.no_wpp && x == 0 && y > 0 && flags[(y - 1) * F.wc + F.wc - 1] != jb->epoch) rc = -3;
    if (flags[y * F.wc + x] == jb->epoch) rc = -3;  // drawn twice
    if (rc) break;
    const kvz::CtuModel *cm = kvz::picture_model(jb->models, frame);
    kvz::ctu_build_dispatch(build, [&](auto bt) { if constexpr (bt.joint) run_ctu(bt, cm, host_tables(), F, sh, frame, x, y); });
    flags[y * F.wc + x] = jb->epoch;
  }
  for (int i = 0; i < n && rc == 0; i++)
    for (unsigned v : done[(size_t)i]) if (v != records[(size_t)i].epoch) rc = -3;  // a CTU the list left out
  return rc;
}
