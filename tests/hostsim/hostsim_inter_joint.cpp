// hostsim_inter_joint.cpp -- TEST INFRASTRUCTURE (see hostsim.cpp and hostsim_inter_models.cpp, which this unit includes whole: one library with everything of
// libkvz_hostsim_inter_models.so plus the twin of kvz_hip_dev_inter_ctu_pass_groups).  B pictures of different sizes in one launch of the inter CTU pass on the host:
// the device compiles the program with KVZ_ICTU_JOINT 0 and 1; here the switch is a variable (as hostsim_inter_lists.cpp has KVZ_ICTU_LISTS), so that this one
// library holds both forms of the same text -- the plain one behind every entry point of the units it includes, the JOINT one behind a launch of groups.  ONE program
// state walks the launch's real ticket list, as a persistent workgroup does: consecutive CTUs belong to pictures of different sizes, QPs and POCs, and whatever
// the program keeps from one CTU to the next meets another picture's geometry.  The launch is checked by the text the library checks it with and its lists and
// its table are made by the functions the library makes them with (kvz_inter_joint.hpp), and the table is read by the kernel's own begin_ctu.
// tests/test_inter_joint_sim.py builds and uses it.
static int g_kvz_ictu_joint = 0;
#define KVZ_ICTU_JOINT g_kvz_ictu_joint
#include "hostsim_inter_models.cpp"
#include "../../kvazaar_amd/csrc/kvz_inter_joint.hpp"

// 0 when kvz_hip_dev_inter_ctu_pass_groups accepts the launch, -1 when it refuses it (with its message)
extern "C" int kvz_hostsim_inter_joint_check(const kvz_hip_inter_group *groups, int n_groups, const kvz_hip_inter_params *p)
{
  return kvz::inter_joint_known(groups, n_groups, p, "kvz_hostsim_inter_joint_check") ? 0 : -1;
}

// the ticket list of a joint launch of n groups, geometry[3 * i ..] = { wc, hc, n_pictures } of group i: the WPP list, or with no_wpp the raster one.  Returns the
// number of items (out may be NULL to ask for it)
extern "C" long kvz_hostsim_inter_joint_tickets(const int32_t *geometry, int n_groups, int no_wpp, uint32_t *out)
{
  std::vector<kvz::InterJointGeometry> g;
  for (int i = 0; i < n_groups; i++) g.push_back(kvz::InterJointGeometry{ geometry[3 * i], geometry[3 * i + 1], geometry[3 * i + 2] });
  std::vector<uint32_t> items;
  if (no_wpp) kvz::inter_joint_ticket_lists(g.data(), n_groups, nullptr, &items);
  else kvz::inter_joint_ticket_lists(g.data(), n_groups, &items, nullptr);
  if (out) memcpy(out, items.data(), items.size() * sizeof(uint32_t));
  return (long)items.size();
}
// ... and the list of a launch of one size (kvz_inter_host.hpp inter_ticket_items), which a joint launch of one group must have
extern "C" long kvz_hostsim_inter_ticket_items(int wc, int hc, int n_pictures, int no_wpp, uint32_t *out)
{
  std::vector<uint32_t> items;
  kvz::inter_ticket_items(wc, hc, n_pictures, no_wpp, items);
  if (out) memcpy(out, items.data(), items.size() * sizeof(uint32_t));
  return (long)items.size();
}

// kvz_hip_dev_inter_ctu_pass_groups on the host: the groups' buffers are host arrays in the pass's layouts (coeff may be NULL, group by group).
// coeff_weights_of_qp[52] / fbits: the constants the library has built in.  Returns 0, or -1 for what the library refuses (nothing is computed then).
extern "C" int kvz_hostsim_inter_pass_groups(const kvz_hip_inter_group *groups, int n_groups, const kvz_hip_inter_params *p, const uint64_t *coeff_weights_of_qp, const float *fbits)
{
  if (!kvz::inter_joint_known(groups, n_groups, p, "kvz_hostsim_inter_pass_groups")) return -1;
  static kvz::Tables tb;
  kvz::build_tables(&tb);
  long total = 0;
  for (int i = 0; i < n_groups; i++) total += (long)((groups[i].width + 63) / 64) * ((groups[i].height + 63) / 64) * groups[i].n_pictures;
  kvz::ICtx *ctx = (kvz::ICtx *)calloc((size_t)total, sizeof(kvz::ICtx));
  const kvz::InterJointTable table = kvz::inter_joint_table(groups, n_groups, p, ctx, [&](kvz::InterModel *row, int qp) {
    kvz::inter_model_init(row, qp, p->poc, coeff_weights_of_qp[qp], fbits, p->mv_constraint, p->sao, p->deblock, p->fme_level, p->pu_depth_inter_max, p->no_wpp, p->fast_residual_cost,
                          0, 0, 0, 0, 0, 0, p->no_tmvp, 0);
  });
  kvz::InterSlab *slab = (kvz::InterSlab *)calloc(1, sizeof(kvz::InterSlab));
  kvz::InterFrames F;
  memset(&F, 0, sizeof F);  // no geometry, no picture buffers: begin_ctu takes them from the records
  F.ctx_out = ctx; F.slabs = slab;
  F.pictures = (const kvz::InterPicture *)table.image.data();
  for (int i = 0; i < n_groups; i++) memset(groups[i].cu, 0, (size_t)(groups[i].width / 4) * (groups[i].height / 4) * groups[i].n_pictures * sizeof(kvz_hip_cu_info));  // (as the twin of the _pictures entry point)
  std::vector<uint32_t> items;
  if (p->no_wpp) kvz::inter_joint_ticket_lists(table.geometry.data(), n_groups, nullptr, &items);
  else kvz::inter_joint_ticket_lists(table.geometry.data(), n_groups, &items, nullptr);
  g_kvz_ictu_joint = 1;
  kvz::InterCtu::begin_launch(F, table.model_of_picture(table.image.data(), 0), &tb, slab);
  for (const uint32_t item : items) {
    kvz::InterCtu::begin_ctu((int)(item >> 16), (int)(item & 0xff) * 64, (int)((item >> 8) & 0xff) * 64);
    kvz::InterCtu::run();
  }
  g_kvz_ictu_joint = 0;
  free(ctx); free(slab);
  return 0;
}
