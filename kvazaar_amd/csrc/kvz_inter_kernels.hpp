// kvz_inter_kernels.hpp -- the __global__ entry point of the inter CTU pass (kvz_inter_ctu.hpp) under the in-order ticket schedule of kvz_ctu_kernels.hpp: one
// persistent workgroup per resident slot draws CTUs (picture, x, y) from a list in which every CTU follows the ones it depends on (its left and above-right
// neighbours in the same picture: CU info, reconstruction and the row coder's contexts), waits for their `done` flags and runs the program on the slab of its slot.
// Compiled in a translation unit of its own (kvz_inter_tu.hip); kvz_hip.hip only sees the declaration.
#pragma once
#include <hip/hip_runtime.h>

#include "kvz_inter_builds.hpp"
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

// the kernel's builds: kvz_inter_builds.hpp lists them -- unit, name and switches -- and says what each switch means
#define KVZ_ICTU_KERNEL(name) __global__ void __launch_bounds__(KVZ_ICTU_THREADS) __attribute__((amdgpu_waves_per_eu(KVZ_ICTU_WAVES_PER_EU, KVZ_ICTU_WAVES_PER_EU))) name(const InterFrames F, const InterModel *model, const Tables *tb, const InterSched sched)
#ifndef KVZ_INTER_KERNEL_BODY
#define KVZ_ICTU_X(unit, suffix, ...) KVZ_ICTU_KERNEL(inter_ctu_ticket_kernel_##suffix);
KVZ_ICTU_BUILDS(KVZ_ICTU_X)
#undef KVZ_ICTU_X
// the kernel of a unit of the list, for the occupancy query and the launch; nullptr where the list has no such unit
inline const void *inter_build_kernel(int unit)
{
#define KVZ_ICTU_X(u, suffix, ...) if (unit == u) return (const void *)inter_ctu_ticket_kernel_##suffix;
  KVZ_ICTU_BUILDS(KVZ_ICTU_X)
#undef KVZ_ICTU_X
  return nullptr;
}
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
// the name this unit defines, from its switches: the kind, then how coefficients are priced.  The body holds the name and the switches against the list
#if KVZ_ICTU_REFS
#define KVZ_ICTU_KIND refs_
#elif KVZ_ICTU_P
#define KVZ_ICTU_KIND p_
#elif KVZ_ICTU_ME
#define KVZ_ICTU_KIND me_
#elif KVZ_ICTU_JOINT
#define KVZ_ICTU_KIND joint_
#elif KVZ_ICTU_LISTS
#define KVZ_ICTU_KIND lists_
#else
#define KVZ_ICTU_KIND
#endif
#if KVZ_ICTU_CABAC
#define KVZ_ICTU_THIS KVZ_ICTU_PASTE(KVZ_ICTU_KIND, cabac)
#else
#define KVZ_ICTU_THIS KVZ_ICTU_PASTE(KVZ_ICTU_KIND, fast)
#endif
#define KVZ_ICTU_PASTE_(a, b) a##b
#define KVZ_ICTU_PASTE(a, b) KVZ_ICTU_PASTE_(a, b)
#define KVZ_ICTU_STR_(x) #x
#define KVZ_ICTU_STR(x) KVZ_ICTU_STR_(x)
KVZ_ICTU_KERNEL(KVZ_ICTU_PASTE(inter_ctu_ticket_kernel_, KVZ_ICTU_THIS))
{
  static_assert(inter_build_named(inter_build_choose({ KVZ_ICTU_CABAC != 0, KVZ_ICTU_LISTS != 0, KVZ_ICTU_JOINT != 0, KVZ_ICTU_ME != 0, KVZ_ICTU_P != 0, KVZ_ICTU_REFS != 0 }), KVZ_ICTU_STR(KVZ_ICTU_THIS)),
                "this unit's switches are no row of KVZ_ICTU_BUILDS (kvz_inter_builds.hpp), or the kernel it defines does not carry that row's name");
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
