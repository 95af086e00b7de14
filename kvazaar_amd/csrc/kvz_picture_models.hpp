// kvz_picture_models.hpp -- which cost models and model tables (include/kvz_hip_types.h) the library accepts: the checks every entry point makes before it queues anything.
// Host code without a HIP dependency: kvz_batch.hpp and kvz_dev.hpp call it, and the host simulation (tests/hostsim) compiles the same text.
#pragma once
#include <stdio.h>
#include <string.h>

#include "../../include/kvz_hip_types.h"
#include "kvz_ctu_builds.hpp"

namespace kvz {

// the struct versions this library knows (include/kvz_hip_types.h struct_size): the current one
inline bool cost_model_known(const kvz_hip_intra_cost_model *m, const char *who)
{
  if (m && m->struct_size == sizeof(kvz_hip_intra_cost_model)) return true;
  fprintf(stderr, "%s: kvz_hip_intra_cost_model.struct_size %u is not this library's %zu (caller built against other headers, or the struct was not set up by kvz_hip_intra_cost_model_init)\n",
          who, m ? m->struct_size : 0u, sizeof(kvz_hip_intra_cost_model));
  return false;
}
// Sign data hiding (kvz_hip_intra_cost_model::signhide) exists for kvz_quant's levels under the ticket schedule: kvz_rdoq's own hiding step (rdo.c:971) works on the
// rate deltas of its chain and is not on the device, and NxN partitions only occur in the preset that has RDOQ.
inline bool signhide_known(const kvz_hip_intra_cost_model *m, bool ticket_schedule, const char *who)
{
  if (!m->signhide) return true;
  if (m->rdoq) { fprintf(stderr, "%s: signhide together with rdoq is not supported (kvz_rdoq's own sign hiding is not on the device)\n", who); return false; }
  if (m->search_nxn) { fprintf(stderr, "%s: signhide together with search_nxn is not supported\n", who); return false; }
  if (!ticket_schedule) { fprintf(stderr, "%s: signhide needs the ticket schedule (not KVZ_HIP_SCHED=wave)\n", who); return false; }
  return true;
}
// Scaling lists are state of the batch (kvz_hip_batch_set_scaling_lists); while it has them (`lists`) the pass quantises with kvz_quant under a factor per position:
// kvz_rdoq would need the per-coefficient error scales (scalinglist.c:351-367) and the hiding rule a factor per position in its rounding remainders -- not built.
inline bool scaling_lists_known(const kvz_hip_intra_cost_model *m, bool lists, const char *who)
{
  if (!lists) return true;
  if (m->rdoq) { fprintf(stderr, "%s: the batch has scaling lists: rdoq is not supported with them (kvz_rdoq's per-coefficient error scales are not on the device)\n", who); return false; }
  if (m->search_nxn) { fprintf(stderr, "%s: the batch has scaling lists: search_nxn is not supported with them\n", who); return false; }
  if (m->signhide) { fprintf(stderr, "%s: the batch has scaling lists: signhide is not supported with them (the hiding rule takes one quantiser factor per block)\n", who); return false; }
  return true;
}
inline bool scaling_lists_known(const kvz_hip_picture_models *pm, bool lists, const char *who)
{
  for (int i = 0; lists && i < pm->n_models; i++) if (!scaling_lists_known(&pm->models[i], true, who)) return false;
  return true;
}

// Is this a table a batch of n_frames pictures can run (ticket_schedule: the batch does not run under KVZ_HIP_SCHED=wave)?  Everything an entry point refuses is refused here, before anything is queued.
inline bool picture_models_known(const kvz_hip_picture_models *pm, int n_frames, bool ticket_schedule, const char *who)
{
  if (!pm || pm->struct_size != sizeof(kvz_hip_picture_models)) {
    fprintf(stderr, "%s: kvz_hip_picture_models.struct_size %u is not this library's %zu\n", who, pm ? pm->struct_size : 0u, sizeof(kvz_hip_picture_models));
    return false;
  }
  if (pm->n_models < 1 || pm->n_models > 65536 || !pm->models || !pm->model_of_picture) { fprintf(stderr, "%s: a model table needs 1 .. 65536 models and a model index per picture (n_models %d)\n", who, pm->n_models); return false; }
  for (int i = 0; i < pm->n_models; i++)  // (a model of another size would also shift every model behind it)
    if (!cost_model_known(&pm->models[i], who)) return false;
  const kvz_hip_intra_cost_model &m0 = pm->models[0];
  for (int i = 0; i < pm->n_models; i++) {
    const kvz_hip_intra_cost_model &m = pm->models[i];
    // these select the kernel instantiation, the ticket list and the one price table of the launch
    if (!m.adaptive != !m0.adaptive || !m.no_wpp != !m0.no_wpp || !m.search_32x32 != !m0.search_32x32 || !m.rdoq != !m0.rdoq || !m.search_nxn != !m0.search_nxn ||
        memcmp(m.entropy_fbits, m0.entropy_fbits, sizeof m.entropy_fbits) != 0) {
      fprintf(stderr, "%s: model %d differs from model 0 in adaptive / no_wpp / search_32x32 / rdoq / search_nxn / entropy_fbits (the models of one launch may differ in qp, lambda, lambda_sqrt, coeff_weights, ctx_init and coeff_cabac)\n", who, i);
      return false;
    }
    if (m.rdoq && !m.coeff_cabac) { fprintf(stderr, "%s: model %d has rdoq without coeff_cabac\n", who, i); return false; }
    if (!signhide_known(&m, true, who)) return false;  // (the schedule is asked about below, for every table)
  }
  for (int f = 0; f < n_frames; f++)
    if (pm->model_of_picture[f] >= pm->n_models) { fprintf(stderr, "%s: model_of_picture[%d] = %u of %d models\n", who, f, (unsigned)pm->model_of_picture[f], pm->n_models); return false; }
  if (!ticket_schedule) { fprintf(stderr, "%s: per-picture models need the ticket schedule (not KVZ_HIP_SCHED=wave)\n", who); return false; }
  return true;
}
inline bool picture_models_any_cabac(const kvz_hip_picture_models *pm)
{
  for (int i = 0; i < pm->n_models; i++) if (pm->models[i].coeff_cabac) return true;
  return false;
}
inline bool picture_models_any_signhide(const kvz_hip_picture_models *pm)
{
  for (int i = 0; i < pm->n_models; i++) if (pm->models[i].signhide) return true;
  return false;
}
// the build that serves a launch of these tables (checked; a group's: one per batch), as ctu_build_choose picks it
inline int picture_models_build(const kvz_hip_picture_models *const *models, int n, bool lists, bool joint)
{
  const kvz_hip_intra_cost_model &m0 = models[0]->models[0];
  bool any_cabac = false, any_signhide = false;
  for (int i = 0; i < n; i++) { any_cabac |= picture_models_any_cabac(models[i]); any_signhide |= picture_models_any_signhide(models[i]); }
  return ctu_build_choose({ m0.search_32x32 != 0, m0.rdoq != 0, m0.search_nxn != 0, any_cabac, any_signhide, lists, joint });
}
}  // namespace kvz
