// kvz_ctu_kernels.hpp -- the __global__ entry points of the batched CTU pass (the program itself is kvz_ctu.hpp) and their scheduling protocol.
//
// Build layout: the instantiations (kvz_ctu_builds.hpp lists them) are the bulk of the library's compile time, so kvazaar_amd/build.py compiles each of them in a
// translation unit of its own (kvz_ctu_tu.hip with -DKVZ_CTU_KERNEL_TU=<unit>), in parallel, next to kvz_hip.hip compiled with -DKVZ_CTU_SEPARATE_TUS -- which then
// only sees DECLARATIONS here and launches the kernels through their host stubs.  Without that define kvz_hip.hip is self-contained as before.
#pragma once
#include <hip/hip_runtime.h>

#include "kvz_ctu.hpp"
#include "kvz_ctu_builds.hpp"
#include "kvz_ctu_qp_builds.hpp"
#include "kvz_joint.hpp"

#if defined(KVZ_CTU_SEPARATE_TUS) && !defined(KVZ_CTU_KERNEL_TU) && !defined(KVZ_CTU_QP_KERNEL_TU)
#define KVZ_CTU_KERNEL_BODIES 0
#else
#define KVZ_CTU_KERNEL_BODIES 1
#endif

namespace kvz {

// One workgroup per CTU of the anti-diagonal `wave` (x + 2y == wave) of every frame.
#ifdef KVZ_CTU_NUM_VGPR  /* register-cap experiments */
#define KVZ_CTU_VGPR_ATTR __attribute__((amdgpu_num_vgpr(KVZ_CTU_NUM_VGPR)))
#else
#define KVZ_CTU_VGPR_ATTR
#endif
#ifndef KVZ_CTU_WAVES_PER_EU
#define KVZ_CTU_WAVES_PER_EU 4  /* 8 workgroups of 128 lanes per CU = 4 wavefronts per SIMD at 128 VGPRs (LDS 16.5 KB would allow 9, but 96 VGPRs cost more than the ninth workgroup gives: profiles/experiments/r01_ab13*) */
#endif
template <bool CABAC> __global__ void __launch_bounds__(KVZ_CTU_THREADS) __attribute__((amdgpu_waves_per_eu(KVZ_CTU_WAVES_PER_EU))) intra_ctu_wave_kernel(const CtuFrames F, const CtuModel model, const Tables *tb,
                                                                        const int wave, const int y_min, const int n_diag)
#if !KVZ_CTU_KERNEL_BODIES
;
#else
{
  __shared__ CtuSharedT<CABAC> shared;
  __shared__ CtuModel m;  // scalars in LDS; its price table stays in HBM (kvz_hip_batch::d_entropy)
  if (threadIdx.x == 0) m = model;
  __syncthreads();
  CtuProgramT<CABAC> p;
  p.m = &m; p.tb = tb; p.F = F; p.s = &shared;
  p.frame = blockIdx.x / n_diag;
  const int y = y_min + (int)(blockIdx.x % n_diag);
  p.cx = (wave - 2 * y) * 64;
  p.cy = y * 64;
  p.run();
}
#endif

// ---- single-launch schedule: in-order tickets --------------------------------------------------------------------
// Work items (one CTU each) are listed in an order in which every CTU comes after the CTUs it depends on (anti-diagonal
// x + 2y ascending, all frames interleaved).  Workgroups draw tickets from an atomic counter and process the item behind
// the ticket; before touching neighbour data they wait for the `done` flags of the left and the above-right CTU.
// Deadlock-free for ANY number of resident workgroups: an item only ever waits for items with smaller tickets, and every
// smaller ticket has been drawn by a workgroup that is running (induction over the ticket order) -- no co-residency of
// the whole grid is assumed.  Hand-off follows the agent-scope release/acquire recipe of the CDNA guide (G16): producer
// drains its stores, one lane releases at agent scope and stores the flag; consumer polls relaxed, one lane acquires,
// then the workgroup barrier.  Compared with one launch per diagonal this removes the per-launch tail (a diagonal of
// n CTUs x F frames rarely is a multiple of the resident workgroup count) and 61 of 62 launches.
enum { KVZ_SCHED_MODEL_TABLE = 2 /* bit of CtuSched::no_wpp */, KVZ_SCHED_TABLE_AT = 4 /* words behind CtuSched::ticket */, KVZ_SCHED_LISTS_AT = 8 /* likewise */, KVZ_SCHED_CTU_MAP_AT = 12 /* likewise */, KVZ_SCHED_TICKET_WORDS = 16 };
// The map of a launch with a model per CTU (kvz_hip_intra_frames_ctu_models), read by the CTUQP instantiations alone, behind the ticket words beside the model table
// it indexes: for every CTU of every picture, raster, its row of the table.
struct CtuMapTable {
  const uint16_t *model_of_ctu = nullptr;  // [frames][hc][wc]
};
// The scaling-list factors of a launch on a batch that has lists (kvz_batch.hpp scaling_lists_stage), read by the LISTS instantiations alone, behind the ticket
// words like the model table: rows of KVZ_LIST_ROW words (kvz_recon.hpp), one per list set and qp % 6, and for every picture its luma row | its chroma row << 16.
struct CtuListTable {
  const uint32_t *rows = nullptr;
  const uint32_t *rows_of_picture = nullptr;  // [frames]
};
struct CtuSched {
  const uint32_t *items;  // [total]: frame << 16 | y << 8 | x  (CTU coordinates)
  unsigned *ticket;       // atomic ticket counter, zeroed before every launch; at ticket + KVZ_SCHED_TABLE_AT a CtuModelTable when no_wpp has KVZ_SCHED_MODEL_TABLE
  unsigned *done;         // [frames * ctus_per_frame]: epoch of the last call that completed the CTU
  unsigned *error;        // set when a wait exceeds its spin bound (never in a healthy run)
  unsigned total, epoch;
  int no_wpp;             // bit 0: items in raster order per picture; a row's first CTU also waits for the last CTU of the row above
  unsigned long long wait_ticks;  // bound of one wait in ticks of the 100 MHz constant clock (s_memrealtime): wall-clock, so that counter
                                  // serialisation under rocprof, time slicing or preemption cannot turn a healthy run into a timeout
};

#if KVZ_CTU_KERNEL_BODIES
#ifdef KVZ_CTU_TRACE  /* developer build (tools/chain_stress.py): where every CTU of the pass is -- F.prof holds a word per CTU: epoch << 8 | stage */
#define KVZ_TRACE(stage) do { if (threadIdx.x == 0 && __hip_atomic_load(sched.error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) __hip_atomic_store(&F.prof[(long)frame * ctus + y * F.wc + x], (unsigned long long)sched.epoch << 8 | (stage), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while (0)
#else
#define KVZ_TRACE(stage) do { } while (0)
#endif
__device__ __forceinline__ bool wait_done(unsigned *flag, unsigned epoch, unsigned *error, unsigned long long wait_ticks, unsigned tag)
{
  unsigned long long t0 = 0;
  for (unsigned spins = 0;; ++spins) {
    if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch) return true;
    if ((spins & 1023u) == 1023u) {  // bounded: a lost hand-off must not hang the GPU
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // (every half millisecond of waiting: whatever this XCD's L2 holds of the flags' lines goes -- insurance, the poll is an agent-scope load)
      const unsigned long long now = __builtin_amdgcn_s_memrealtime();
      if (!t0) t0 = now;
      else if (now - t0 > wait_ticks) {
        if (atomicCAS(error, 0u, 0x80000000u | tag) == 0u) {  // the first to give up leaves what it can see: the flag as a read-modify-write at the memory side returns it, and how far the tickets are
          error[1] = atomicAdd(flag, 0u);
          error[2] = __hip_atomic_load(error - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return false;
      }  // the first CTU that gave up: the CTU waited FOR and which neighbour it is (kvz_joint.hpp KVZ_HANDOFF_TAG)
    }
    // back off after the first half millisecond: a wait that long is on nobody's critical path (hand-offs arrive within microseconds), and where a pass has stalled --
    // tools/chain_stress.py, profiles/README.md round 6: an eighth of the workgroups standing still in their searches for seconds -- the other seven eighths
    // should not poll the memory system two thousand times a microsecond meanwhile
    if (spins < 1024u) __builtin_amdgcn_s_sleep(16);
    else { __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127); }
  }
}

// The persistent loop of the ticket schedule; the kernels below differ in their register budget only.
// sched.no_wpp & KVZ_SCHED_MODEL_TABLE: the pictures of the launch have models of their own (kvz_hip_intra_frames_models) -- `m` is loaded per CTU from the drawn picture's
// row of the table behind the ticket words.  (A bit of a word the loop keeps anyway and a pointer it keeps anyway: a kernel argument of its own stayed live across the
// whole program and cost the instantiations that spill a register more.)
//
// JOINT (kvz_hip_batch_group, kvz_joint.hpp): the pictures of the launch belong to batches of different geometry.  The item's picture is numbered across the group; the
// workgroup fetches the record of that picture's batch -- frames, model table, hand-off flags and the pass number they hold -- through uniform pointers into registers
// (not LDS: the CABAC builds sit at exactly 20 480 B) and runs the program on it with the picture's index inside its batch.  The table's two pointers take the
// model table's place behind the ticket words; F_arg, `model`, sched.done and sched.epoch are not read.
template <class T> __device__ __forceinline__ T uniform_fetch(const T *p)  // *p, the same for every lane, as scalars
{
  static_assert(sizeof(T) % 4 == 0, "whole words");
  int w[sizeof(T) / 4];
  __builtin_memcpy(w, p, sizeof(T));
  for (unsigned i = 0; i < sizeof(T) / 4; i++) w[i] = __builtin_amdgcn_readfirstlane(w[i]);
  T v;
  __builtin_memcpy(&v, w, sizeof(T));
  return v;
}
//
// CTUQP (kvz_hip_intra_frames_ctu_models): `m` is the row the map behind the ticket words names for the drawn CTU -- its qp, lambda, lambda_sqrt, coeff_weights and
// coeff_cabac -- with the initial context states of the picture's own (slice) row; the switches are the same in every row of a table.
template <bool CABAC, bool S32, bool RDOQ, bool SH = false, bool LISTS = false, bool JOINT = false, bool CTUQP = false> __device__ __forceinline__ void ticket_loop(const CtuFrames &F_arg, const CtuModel &model, const Tables *tb, const CtuSched &sched)
{
  static_assert(!(JOINT && (RDOQ || LISTS)), "joint launches: the ultrafast / fast builds");
  static_assert(!(CTUQP && (RDOQ || SH || LISTS || JOINT)), "a model per CTU: the ultrafast / fast builds of a batch on its own");
  CtuFrames F_joint;  // JOINT: the frames of the drawn picture's batch
  const CtuFrames &F = JOINT ? F_joint : F_arg;
  __shared__ CtuSharedT<CABAC> shared;
  __shared__ CtuModel m;  // scalars in LDS; its price table stays in HBM (kvz_hip_batch::d_entropy)
  // The ticket is broadcast through a field of `shared` that is dead between two CTUs: with the CABAC contexts the block is exactly 20 480 B,
  // and one more word would cost the eighth workgroup per CU (160 KB of LDS).
#ifndef KVZ_CTU_PROFILE
  static_assert(sizeof(CtuSharedT<CABAC>) + sizeof(CtuModel) <= 20480, "eight workgroups per CU");
#endif
  if constexpr (!JOINT && !CTUQP) { if (threadIdx.x == 0 && !(sched.no_wpp & KVZ_SCHED_MODEL_TABLE)) m = model; }
  int ctus = 0;
  if constexpr (!JOINT) ctus = F.wc * F.hc;
  for (;;) {
    __syncthreads();  // previous item fully retired (and m visible on the first trip)
    if (threadIdx.x == 0) shared.best_mode = (int)atomicAdd(sched.ticket, 1u);
    __syncthreads();
    const unsigned t = (unsigned)shared.best_mode;
    if (t >= sched.total) break;
    uint32_t item = sched.items[t];
    if constexpr (JOINT) item = (uint32_t)__builtin_amdgcn_readfirstlane((int)item);
    const int picture = item >> 16, y = (item >> 8) & 0xff, x = item & 0xff;  // picture: what the item numbers, in the diagnostics below
    int frame = picture;
    unsigned *done_flags = sched.done;
    unsigned epoch = sched.epoch;
    CtuModelTable models;
    if constexpr (JOINT) {
      const JointTable jt = uniform_fetch(reinterpret_cast<const JointTable *>(sched.ticket + KVZ_SCHED_TABLE_AT));
      const uint32_t word = (uint32_t)__builtin_amdgcn_readfirstlane((int)jt.batch_of_picture[picture]);
      const JointBatch *jb = joint_record(jt, word);
      F_joint = uniform_fetch(&jb->F);
      models = uniform_fetch(&jb->models);
      done_flags = uniform_fetch(&jb->done);
      epoch = (unsigned)__builtin_amdgcn_readfirstlane((int)jb->epoch);
      frame = joint_frame(word);
      ctus = F.wc * F.hc;
    }
    KVZ_TRACE(1);  // ticket drawn
    if (threadIdx.x == 0) {
      if constexpr (JOINT) m = *picture_model(models, frame);
      else if constexpr (CTUQP) {
        const CtuModelTable table = *reinterpret_cast<const CtuModelTable *>(sched.ticket + KVZ_SCHED_TABLE_AT);
        const CtuMapTable map = *reinterpret_cast<const CtuMapTable *>(sched.ticket + KVZ_SCHED_CTU_MAP_AT);
        m = table.models[map.model_of_ctu[(long)frame * ctus + y * F.wc + x]];
        m.ctx_init = picture_model(table, frame)->ctx_init;
      } else if (sched.no_wpp & KVZ_SCHED_MODEL_TABLE) m = *picture_model(*reinterpret_cast<const CtuModelTable *>(sched.ticket + KVZ_SCHED_TABLE_AT), frame);  // no lane reads m between the barrier above and the one below; the table is constant during the launch
      unsigned *done = done_flags + (long)frame * ctus;
      // a hand-off that timed out anywhere (this launch or an earlier one: the word is sticky until kvz_hip_batch_reset) poisons the pass: from then on
      // tickets are only drained -- no search on stale neighbour data, no further 30-second waits -- and every CTU still publishes its flag
      bool ok = __hip_atomic_load(sched.error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
      if (ok && x > 0) ok = wait_done(&done[y * F.wc + x - 1], epoch, sched.error, sched.wait_ticks, KVZ_HANDOFF_TAG(KVZ_WAIT_LEFT, picture, y, x - 1));
      if (ok && y > 0) ok = wait_done(&done[(y - 1) * F.wc + (x + 1 < F.wc ? x + 1 : x)], epoch, sched.error, sched.wait_ticks, KVZ_HANDOFF_TAG(KVZ_WAIT_ABOVE_RIGHT, picture, y - 1, x + 1 < F.wc ? x + 1 : x));  // above-right implies above and above-left
      if (ok && (sched.no_wpp & 1) && x == 0 && y > 0) ok = wait_done(&done[(y - 1) * F.wc + F.wc - 1], epoch, sched.error, sched.wait_ticks, KVZ_HANDOFF_TAG(KVZ_WAIT_ROW_END, picture, y - 1, F.wc - 1));  // its contexts come from there
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      shared.best_mode = ok ? 1 : 0;
    }
    __syncthreads();
    KVZ_TRACE(2);  // neighbours there
    const bool run_it = shared.best_mode != 0;  // uniform.  (run() first writes the field behind several barriers of its own: no lane can still be reading it here)
    if (run_it) {
      CtuProgramT<CABAC, S32, RDOQ, SH, LISTS, CTUQP> p;
      p.m = &m; p.tb = tb; p.F = F; p.s = &shared;
      if constexpr (LISTS) {  // the picture's two factor rows, as scalars (the table is constant during the launch)
        const CtuListTable lt = *reinterpret_cast<const CtuListTable *>(sched.ticket + KVZ_SCHED_LISTS_AT);
        const uint32_t rows = (uint32_t)__builtin_amdgcn_readfirstlane((int)lt.rows_of_picture[frame]);
        p.lf_y = lt.rows + (size_t)(rows & 0xffffu) * KVZ_LIST_ROW;
        p.lf_c = lt.rows + (size_t)(rows >> 16) * KVZ_LIST_ROW;
      }
      if constexpr (RDOQ) { __shared__ RdoqLds rdoq_lds; p.rl = &rdoq_lds; }
      p.frame = frame; p.cx = x * 64; p.cy = y * 64;
      p.lane_rot = (t * 64) & (KVZ_CTU_THREADS - 1);
      p.run();
    }
    KVZ_TRACE(3);  // searched
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave drains its stores (reconstruction, CU info, coefficients)
    __syncthreads();
    KVZ_TRACE(4);  // stores drained, both wavefronts there
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      KVZ_TRACE(5);  // released
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(&done_flags[(long)frame * ctus + y * F.wc + x], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      KVZ_TRACE(6);  // flag stored
    }
  }
}

#endif  // KVZ_CTU_KERNEL_BODIES

template <bool CABAC, bool S32 = false, bool RDOQ = false> __global__ void __launch_bounds__(KVZ_CTU_THREADS) __attribute__((amdgpu_waves_per_eu(KVZ_CTU_WAVES_PER_EU))) KVZ_CTU_VGPR_ATTR intra_ctu_ticket_kernel(const CtuFrames F, const CtuModel model, const Tables *tb,
                                                                        const CtuSched sched)
#if !KVZ_CTU_KERNEL_BODIES
;
#else
{
  ticket_loop<CABAC, S32, RDOQ>(F, model, tb, sched);
}
#endif
// Sign data hiding (kvz_hip_intra_cost_model::signhide): the program with the hiding stage between kvz_quant and whatever reads levels (kvz_ctu.hpp hide_signs), with
// and without the 32x32 search.  Both carry the CABAC coefficient model; what prices a picture's levels -- and whether its signs are hidden at all -- is its model's
// business at run time, so the pictures of a mixed launch (kvz_hip_picture_models) each come out as in a launch of their own.
template <bool S32> __global__ void __launch_bounds__(KVZ_CTU_THREADS) __attribute__((amdgpu_waves_per_eu(KVZ_CTU_WAVES_PER_EU))) KVZ_CTU_VGPR_ATTR intra_ctu_ticket_kernel_signhide(const CtuFrames F, const CtuModel model, const Tables *tb,
                                                                        const CtuSched sched)
#if !KVZ_CTU_KERNEL_BODIES
;
#else
{
  ticket_loop<true, S32, false, true>(F, model, tb, sched);
}
#endif
// Scaling lists (kvz_hip_batch_set_scaling_lists): the program that quantises and dequantises under a factor per coefficient position (kvz_ctu.hpp LISTS), for the
// two coefficient cost models with and without the 32x32 search.  Launched only on a batch that has lists: every other launch takes the kernels above, unchanged.
template <bool CABAC, bool S32> __global__ void __launch_bounds__(KVZ_CTU_THREADS) __attribute__((amdgpu_waves_per_eu(KVZ_CTU_WAVES_PER_EU))) KVZ_CTU_VGPR_ATTR intra_ctu_ticket_kernel_lists(const CtuFrames F, const CtuModel model, const Tables *tb,
                                                                        const CtuSched sched)
#if !KVZ_CTU_KERNEL_BODIES
;
#else
{
  ticket_loop<CABAC, S32, false, false, true>(F, model, tb, sched);
}
#endif
// A cost model per CTU (kvz_hip_intra_frames_ctu_models, kvz_ctu_qp_builds.hpp): the first kernel above with the drawn CTU's row fetched through the map, for the two
// coefficient cost models with and without the 32x32 search, and the program's CTUQP form (kvz_ctu.hpp: the residual contexts go through every CTU).  Instantiations of their own, in translation units of their own (kvz_ctu_qp_tu.hip): every other launch
// takes the kernels it took.  `model` is not read.
template <bool CABAC, bool S32> __global__ void __launch_bounds__(KVZ_CTU_THREADS) __attribute__((amdgpu_waves_per_eu(KVZ_CTU_WAVES_PER_EU))) KVZ_CTU_VGPR_ATTR intra_ctu_ticket_kernel_ctuqp(const CtuFrames F, const CtuModel model, const Tables *tb,
                                                                        const CtuSched sched)
#if !KVZ_CTU_KERNEL_BODIES
;
#else
{
  ticket_loop<CABAC, S32, false, false, false, false, true>(F, model, tb, sched);
}
#endif
// Joint launches over the batches of a group (kvz_hip_batch_group_intra_frames): the builds above that a group may ask for -- fast estimate or CABAC coefficient model,
// with and without the 32x32 search, and the two sign-hiding ones (SH: CABAC is implied) -- with the drawn picture's batch record fetched per ticket.  Instantiations of
// their own: the kernels above are what they were.
template <bool CABAC, bool S32, bool SH> __global__ void __launch_bounds__(KVZ_CTU_THREADS) __attribute__((amdgpu_waves_per_eu(KVZ_CTU_WAVES_PER_EU))) KVZ_CTU_VGPR_ATTR intra_ctu_joint_kernel(const Tables *tb, const CtuSched sched)
#if !KVZ_CTU_KERNEL_BODIES
;
#else
{
  const CtuFrames no_frames = {};
  const CtuModel no_model = {};
  ticket_loop<CABAC || SH, S32, false, SH, false, true>(no_frames, no_model, tb, sched);
}
#endif
// --rdoq / NxN partitions: its own register budget.  Round 3: kvz_rdoq runs as ONE out-of-line wavefront-cooperative routine (kvz_rdoq.hpp rdoq_block_wave), so the
// instantiation no longer needs the 168 registers the inlined one-lane routine did: 128 registers = 4 wavefronts per SIMD, and with 23.4 KB of LDS seven workgroups
// per CU.  Measured at 1080p QP 27 `medium-pu13`: 3 wavefronts per SIMD 130.4 k CTUs/s, 4: 135.4 k (141.4 k with 320 pictures in flight) -- the pass is still partly
// latency-bound (profiles/r03_*).  (Round 2, one lane per block: 1 wavefront per SIMD 22.5 k, 2: 41.0 k, 3: 54.3 k, 4 with thousands of spills: 17.5 k.)
#ifndef KVZ_RDOQ_WAVES_PER_EU
#define KVZ_RDOQ_WAVES_PER_EU 4
#endif
#define KVZ_CTU_UNIT_HAS_RDOQ(unit, CABAC, S32, RDOQ, SH, LISTS, JOINT) || ((unit) == KVZ_CTU_KERNEL_TU && (RDOQ))
__global__ void __launch_bounds__(KVZ_CTU_THREADS) __attribute__((amdgpu_waves_per_eu(KVZ_RDOQ_WAVES_PER_EU, KVZ_RDOQ_WAVES_PER_EU))) intra_ctu_ticket_kernel_rdoq(const CtuFrames F, const CtuModel model, const Tables *tb, const CtuSched sched)
#if !KVZ_CTU_KERNEL_BODIES || defined(KVZ_CTU_QP_KERNEL_TU) || (defined(KVZ_CTU_KERNEL_TU) && !(0 KVZ_CTU_BUILDS(KVZ_CTU_UNIT_HAS_RDOQ)))  // (not a template: its body goes where its build is)
;
#else
{
  ticket_loop<true, true, true>(F, model, tb, sched);
}
#endif

// the kernel of a build (naming it instantiates it: kvz_ctu_tu.hip)
template <class B> constexpr auto ctu_build_kernel(B)
{
  if constexpr (B::joint) return &intra_ctu_joint_kernel<B::cabac, B::s32, B::sh>;
  else if constexpr (B::rdoq) return &intra_ctu_ticket_kernel_rdoq;
  else if constexpr (B::lists) return &intra_ctu_ticket_kernel_lists<B::cabac, B::s32>;
  else if constexpr (B::sh) return &intra_ctu_ticket_kernel_signhide<B::s32>;
  else return &intra_ctu_ticket_kernel<B::cabac, B::s32, false>;
}
}  // namespace kvz

