// kvz_inter_kernels.hpp -- the __global__ entry point of the inter CTU pass (kvz_inter_ctu.hpp) under the in-order ticket schedule of kvz_ctu_kernels.hpp: one
// persistent workgroup per resident slot draws CTUs (picture, x, y) from a list in which every CTU follows the ones it depends on (its left and above-right
// neighbours in the same picture: CU info, reconstruction and the row coder's contexts), waits for their `done` flags and runs the program on the slab of its slot.
// Compiled in a translation unit of its own (kvz_inter_tu.hip); kvz_hip.hip only sees the declaration.
#pragma once
#include <hip/hip_runtime.h>

#include "kvz_inter_ctu.hpp"

namespace kvz {

struct InterSched {
  const uint32_t *items;  // [total]: picture << 16 | y << 8 | x
  unsigned *ticket;       // zeroed before the launch
  unsigned *done;         // [pictures * CTUs], zeroed before the launch
  unsigned *error;
  unsigned total;
  int no_wpp;
  unsigned long long wait_ticks;
};

// two builds of the kernel (kvz_inter_ctu.hpp KVZ_ICTU_CABAC): `_fast` for pictures whose coefficients are priced by kvz_fast_coeff_cost (small context sets: 20 KB of LDS,
// eight workgroups per CU), `_cabac` for those priced with the residual coder's contexts; and the same two for launches with scaling lists
// (-DKVZ_ICTU_LISTS=1, kvz_inter_ctu.hpp: kvz_hip_dev_inter_ctu_pass_lists), `_lists_fast` / `_lists_cabac`; and the same two for joint launches of pictures of
// different sizes (-DKVZ_ICTU_JOINT=1: kvz_hip_dev_inter_ctu_pass_groups), `_joint_fast` / `_joint_cabac`.  In a joint launch the item's picture numbers the pictures
// across the groups; F holds no geometry, F.pictures the launch's table (kvz_inter_ctu.hpp InterJointPicture / InterJointGroup), and sched.done is indexed by the
// group's first CTU + the picture's index in the group x the group's CTUs + the CTU; and the same two for launches that choose the integer motion search
// (-DKVZ_ICTU_ME=1: kvz_hip_inter_params me_algorithm / me_max_steps / me_early_termination), `_me_fast` / `_me_cabac`, which raise the launch's error word when a
// search loop reached its bound (kvz_inter_ctu_pix.inc IC_ME_LOOP_BOUND); and the same two for launches of P pictures (-DKVZ_ICTU_P=1:
// kvz_hip_dev_inter_ctu_pass_slices with KVZ_HIP_SLICE_P), `_p_fast` / `_p_cabac`, the program without its L1 half (kvz_inter_ctu.hpp KVZ_ICTU_P); and the same two for launches of P pictures with
// reference lists (-DKVZ_ICTU_P=1 -DKVZ_ICTU_REFS=1: kvz_hip_dev_inter_ctu_pass_refs), `_refs_fast` / `_refs_cabac`: F.ref / F.ref_cu are a pool of frames and
// F.pictures holds InterPictureRefs records (kvz_inter_ctu.hpp KVZ_ICTU_REFS)
#define KVZ_ICTU_KERNEL(name) __global__ void __launch_bounds__(KVZ_ICTU_THREADS) __attribute__((amdgpu_waves_per_eu(KVZ_ICTU_WAVES_PER_EU, KVZ_ICTU_WAVES_PER_EU))) name(const InterFrames F, const InterModel *model, const Tables *tb, const InterSched sched)
#ifndef KVZ_INTER_KERNEL_BODY
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_fast);
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_cabac);
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_lists_fast);
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_lists_cabac);
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_joint_fast);
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_joint_cabac);
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_me_fast);
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_me_cabac);
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_p_fast);
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_p_cabac);
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_refs_fast);
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_refs_cabac);
#else
#if KVZ_ICTU_JOINT && KVZ_ICTU_LISTS
#error "scaling lists are not part of joint launches"
#endif
#if KVZ_ICTU_ME && (KVZ_ICTU_JOINT || KVZ_ICTU_LISTS)
#error "the choice of the integer motion search is not part of joint launches or of launches with scaling lists"
#endif
#if KVZ_ICTU_P && (KVZ_ICTU_LISTS || KVZ_ICTU_JOINT || KVZ_ICTU_ME)
#error "P pictures are not part of launches with scaling lists, of joint launches or of launches that choose the integer motion search"
#endif
#if KVZ_ICTU_REFS && !KVZ_ICTU_P
#error "reference lists are built for P pictures only"
#endif
#if KVZ_ICTU_REFS && KVZ_ICTU_CABAC
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_refs_cabac)
#elif KVZ_ICTU_REFS
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_refs_fast)
#elif KVZ_ICTU_P && KVZ_ICTU_CABAC
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_p_cabac)
#elif KVZ_ICTU_P
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_p_fast)
#elif KVZ_ICTU_ME && KVZ_ICTU_CABAC
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_me_cabac)
#elif KVZ_ICTU_ME
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_me_fast)
#elif KVZ_ICTU_JOINT && KVZ_ICTU_CABAC
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_joint_cabac)
#elif KVZ_ICTU_JOINT
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_joint_fast)
#elif KVZ_ICTU_LISTS && KVZ_ICTU_CABAC
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_lists_cabac)
#elif KVZ_ICTU_LISTS
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_lists_fast)
#elif KVZ_ICTU_CABAC
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_cabac)
#else
KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_fast)
#endif
{
  __shared__ int s_ticket;
#if KVZ_ICTU_JOINT
  __shared__ unsigned s_done_at;  // the drawn CTU's own `done` flag: lane 0 finds it in the records once per CTU, before the wait
#else
  const int ctus = F.wc * F.hc;
#endif
  InterCtu::begin_launch(F, model, tb, F.slabs + blockIdx.x);  // the program's state and constants: workgroup-scope variables in LDS (kvz_inter_ctu.hpp)
  for (;;) {
    __syncthreads();
    if (threadIdx.x == 0) s_ticket = (int)atomicAdd(sched.ticket, 1u);
    __syncthreads();
    const unsigned t = (unsigned)s_ticket;
    if (t >= sched.total) break;
    const uint32_t item = sched.items[t];
    const int frame = item >> 16, y = (item >> 8) & 0xff, x = item & 0xff;
    __syncthreads();
    if (threadIdx.x == 0) {
#if KVZ_ICTU_JOINT
      // the picture's own flags under the picture's own width: the group record, before the wait (wavefront-uniform; the program's begin_ctu reads it again for the rest)
      const InterJointPicture *jp = (const InterJointPicture *)F.pictures + frame;
      const InterJointGroup *jg = (const InterJointGroup *)((const uint8_t *)F.pictures + jp->group_at);
      const unsigned wc = (unsigned)jg->wc, first = (unsigned)jg->ctu_base + jp->index * (wc * (unsigned)jg->hc);
      unsigned *done = sched.done + first;
      s_done_at = first + y * wc + x;
#else
      unsigned *done = sched.done + (long)frame * ctus;
#endif
      auto wait = [&](unsigned *flag) -> bool {
        unsigned long long t0 = 0;
        for (unsigned spins = 0;; ++spins) {
          if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 1u) return true;
          if ((spins & 1023u) == 1023u) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // (as in the intra pass: kvz_ctu_kernels.hpp wait_done)
            const unsigned long long now = __builtin_amdgcn_s_memrealtime();
            if (!t0) t0 = now;
            else if (now - t0 > sched.wait_ticks) { atomicExch(sched.error, 1u); return false; }
          }
          if (spins < 1024u) __builtin_amdgcn_s_sleep(16);  // (backs off as the intra pass does: kvz_ctu_kernels.hpp wait_done)
          else { __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127); }
        }
      };
      bool ok = __hip_atomic_load(sched.error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
#if KVZ_ICTU_JOINT
      if (ok && x > 0) ok = wait(&done[y * wc + x - 1]);
      if (ok && y > 0) ok = wait(&done[(y - 1) * wc + ((unsigned)x + 1 < wc ? x + 1 : x)]);
      if (ok && sched.no_wpp && x == 0 && y > 0) ok = wait(&done[(y - 1) * wc + wc - 1]);
#else
      if (ok && x > 0) ok = wait(&done[y * F.wc + x - 1]);
      if (ok && y > 0) ok = wait(&done[(y - 1) * F.wc + (x + 1 < F.wc ? x + 1 : x)]);
      if (ok && sched.no_wpp && x == 0 && y > 0) ok = wait(&done[(y - 1) * F.wc + F.wc - 1]);
#endif
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      s_ticket = ok ? 1 : 0;
    }
    __syncthreads();
    if (s_ticket != 0) {
      InterCtu::begin_ctu(frame, x * 64, y * 64);
      InterCtu::run();
#if KVZ_ICTU_ME
      if (threadIdx.x == 0 && g_ic.me_overrun) atomicExch(sched.error, 1u);
#endif
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#if KVZ_ICTU_JOINT
      __hip_atomic_store(&sched.done[s_done_at], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
      __hip_atomic_store(&sched.done[(long)frame * ctus + y * F.wc + x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
    }
  }
}
#endif

}  // namespace kvz
