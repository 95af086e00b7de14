// kvz_ctu_tu.hip -- one CTU kernel instantiation per translation unit (see kvz_ctu_kernels.hpp): compiled eighteen times by kvazaar_amd/build.py with
// -DKVZ_CTU_KERNEL_TU=0..17, in parallel with kvz_hip.hip.
#include <hip/hip_runtime.h>

#ifndef KVZ_CTU_KERNEL_TU
#error "compile with -DKVZ_CTU_KERNEL_TU=<0..17>"
#endif
#include "kvz_ctu_kernels.hpp"

namespace kvz {
#define KVZ_TICKET_ARGS const CtuFrames, const CtuModel, const Tables *, const CtuSched
#if KVZ_CTU_KERNEL_TU == 0    // no CABAC coefficient model (QP < 28 of `ultrafast`), both schedules
template __global__ void intra_ctu_ticket_kernel<false, false, false>(KVZ_TICKET_ARGS);
template __global__ void intra_ctu_wave_kernel<false>(const CtuFrames, const CtuModel, const Tables *, const int, const int, const int);
#elif KVZ_CTU_KERNEL_TU == 1  // CABAC coefficient model
template __global__ void intra_ctu_ticket_kernel<true, false, false>(KVZ_TICKET_ARGS);
#elif KVZ_CTU_KERNEL_TU == 2  // the older schedule with the CABAC coefficient model
template __global__ void intra_ctu_wave_kernel<true>(const CtuFrames, const CtuModel, const Tables *, const int, const int, const int);
#elif KVZ_CTU_KERNEL_TU == 3  // 32x32 CUs searched
template __global__ void intra_ctu_ticket_kernel<false, true, false>(KVZ_TICKET_ARGS);
#elif KVZ_CTU_KERNEL_TU == 4
template __global__ void intra_ctu_ticket_kernel<true, true, false>(KVZ_TICKET_ARGS);
#elif KVZ_CTU_KERNEL_TU == 5  // RDOQ / NxN: intra_ctu_ticket_kernel_rdoq's body (kvz_ctu_kernels.hpp)
#elif KVZ_CTU_KERNEL_TU == 6  // sign data hiding
template __global__ void intra_ctu_ticket_kernel_signhide<false>(KVZ_TICKET_ARGS);
#elif KVZ_CTU_KERNEL_TU == 7  // ... with 32x32 CUs searched
template __global__ void intra_ctu_ticket_kernel_signhide<true>(KVZ_TICKET_ARGS);
#elif KVZ_CTU_KERNEL_TU == 8  // scaling lists: fast estimate
template __global__ void intra_ctu_ticket_kernel_lists<false, false>(KVZ_TICKET_ARGS);
#elif KVZ_CTU_KERNEL_TU == 9  // ... CABAC coefficient model
template __global__ void intra_ctu_ticket_kernel_lists<true, false>(KVZ_TICKET_ARGS);
#elif KVZ_CTU_KERNEL_TU == 10  // ... and both with 32x32 CUs searched
template __global__ void intra_ctu_ticket_kernel_lists<false, true>(KVZ_TICKET_ARGS);
#elif KVZ_CTU_KERNEL_TU == 11
template __global__ void intra_ctu_ticket_kernel_lists<true, true>(KVZ_TICKET_ARGS);
#elif KVZ_CTU_KERNEL_TU == 12  // joint launches (kvz_hip_batch_group): fast estimate
template __global__ void intra_ctu_joint_kernel<false, false, false>(const Tables *, const CtuSched);
#elif KVZ_CTU_KERNEL_TU == 13  // ... CABAC coefficient model
template __global__ void intra_ctu_joint_kernel<true, false, false>(const Tables *, const CtuSched);
#elif KVZ_CTU_KERNEL_TU == 14  // ... both with 32x32 CUs searched
template __global__ void intra_ctu_joint_kernel<false, true, false>(const Tables *, const CtuSched);
#elif KVZ_CTU_KERNEL_TU == 15
template __global__ void intra_ctu_joint_kernel<true, true, false>(const Tables *, const CtuSched);
#elif KVZ_CTU_KERNEL_TU == 16  // ... sign data hiding
template __global__ void intra_ctu_joint_kernel<true, false, true>(const Tables *, const CtuSched);
#elif KVZ_CTU_KERNEL_TU == 17
template __global__ void intra_ctu_joint_kernel<true, true, true>(const Tables *, const CtuSched);
#else
#error "KVZ_CTU_KERNEL_TU out of range"
#endif
}  // namespace kvz
